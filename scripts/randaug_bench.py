"""Time of the RandAugment launch alone, on one GPU (profiles/randaug.md): the eager launch
between two events, `reps` back-to-back launches per event pair after a warm-up, the best and
the median of `batches` pairs, in us per launch.  For CIFAR (N x 3 x 32 x 32) and ImageNet
(N x 224 x 224 x 3): each op forced by a one-entry table, the default two-op chain over all
ops, four ops twice in a row, and as the yardstick that batch's input launch (cifar_augment /
imagenet_u8_pack).
The image contents are uniform random bytes; a forced op's sign still varies per image.
Prints one markdown table row per configuration with its share of the step time given.

    python scripts/randaug_bench.py [N] [reps] [batches]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd as dtr  # noqa: E402
from distributed_tensorflow_resnet_amd.data import randaug as ra  # noqa: E402

STEP_MS = {"cifar": 0.74, "imagenet": 10.3}   # README: CIFAR RN50 bs128, ImageNet RN50 bs128


def time_us(launch, reps, batches):
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return min(out), statistics.median(out)


def main():
    N, reps, batches = (int(v) for v in (sys.argv[1:4] + ["128", "200", "7"][len(sys.argv) - 1:]))
    nat, dev = dtr.native(required=True), torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    gstep = torch.tensor([5], dtype=torch.int64, device=dev)
    print("| batch | configuration | best us | median us | share of step |")
    print("|---|---|---|---|---|")
    for name, hwc, H, W in (("cifar", 0, 32, 32), ("imagenet", 1, 224, 224)):
        shape = (N, H, W, 3) if hwc else (N, 3, H, W)
        src = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
        dst = torch.zeros_like(src)
        x_in = torch.zeros((N, H, W, 8), dtype=torch.bfloat16, device=dev)
        tab = torch.from_numpy(ra.randaug_tables(9, H, W)).to(dev)

        def aug(ops, k):
            return lambda: nat.randaug(src.data_ptr(), dst.data_ptr(), N, H, W, hwc, 1234,
                                       gstep.data_ptr(), k, tab.data_ptr(), tab.numel(), ops, 0,
                                       st)
        if hwc:
            feed = lambda: nat.imagenet_u8_pack(src.data_ptr(), x_in.data_ptr(), N, H, W,  # noqa: E731
                                                1234, gstep.data_ptr(), 1, 0, 0, 0, st)
        else:
            feed = lambda: nat.cifar_augment(src.data_ptr(), x_in.data_ptr(), N, H, W, 8, 4,  # noqa: E731
                                             1234, gstep.data_ptr(), 1, 0, 0, 0, st)
        rows = [("input launch", feed)] + [(ra.RA_OPS[op], aug([op], 1)) for op in range(14)]
        rows.append(("all ops, 2 per image", aug(list(range(14)), 2)))
        # the same op twice: the second one finds the image where the first one left it (for
        # the moving ops of the ImageNet kernel, in global memory)
        rows += [(ra.RA_OPS[op] + " twice", aug([op], 2)) for op in (5, 8, 9, 13)]
        for what, launch in rows:
            best, med = time_us(launch, reps, batches)
            print(f"| {name} N={N} | {what} | {best:.1f} | {med:.1f} | "
                  f"{med / (STEP_MS[name] * 1e3) * 100:.2f} % |", flush=True)


if __name__ == "__main__":
    main()
