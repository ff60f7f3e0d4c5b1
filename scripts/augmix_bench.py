"""Time of the AugMix launch alone, on one GPU (profiles/augmix.md): the eager launch between
two events, `reps` back-to-back launches per event pair (ten times as many for the short CIFAR
launches, so that a window is tens to hundreds of milliseconds) after a warm-up, the best and
the median of `batches` pairs, in us per launch.  For CIFAR (N x 3 x 32 x 32) and ImageNet
(N x 224 x 224 x 3): widths 1, 3 and 4 at the drawn depth and at depth 1 and 3, the paper's op
list at severity 3, and beside them, on the same box and buffers, RandAugment's k = 3 launch
over all ops and that batch's input launch (cifar_augment / imagenet_u8_pack).
The image contents are uniform random bytes.  Prints one markdown table row per configuration
with its share of the step time given.

    python scripts/augmix_bench.py [N] [reps] [batches]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd as dtr  # noqa: E402
from distributed_tensorflow_resnet_amd.data import augmix as am  # noqa: E402
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
    defaults = ["128", "2000", "7"]
    N, reps, batches = (int(v) for v in (sys.argv[1:4] + defaults[len(sys.argv) - 1:]))
    nat, dev = dtr.native(required=True), torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    gstep = torch.tensor([5], dtype=torch.int64, device=dev)
    ops = [int(i) for i in am.augmix_op_table()]
    print("| batch | configuration | best us | median us | share of step |")
    print("|---|---|---|---|---|")
    for name, hwc, H, W in (("cifar", 0, 32, 32), ("imagenet", 1, 224, 224)):
        shape = (N, H, W, 3) if hwc else (N, 3, H, W)
        src = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
        dst = torch.zeros_like(src)
        x_in = torch.zeros((N, H, W, 8), dtype=torch.bfloat16, device=dev)
        acc = torch.zeros((N, 3 * H * W), dtype=torch.int16, device=dev)
        tab9 = torch.from_numpy(ra.randaug_tables(9, H, W)).to(dev)
        mixes = {w: torch.from_numpy(am.augmix_tables(w, 1.0, 1234)).to(dev) for w in (1, 3, 4)}

        def mix(width, depth):
            m = mixes[width]
            return lambda: nat.augmix(src.data_ptr(), dst.data_ptr(), N, H, W, hwc, 1234,
                                      gstep.data_ptr(), width, depth, tab9.data_ptr(),
                                      tab9.numel(), m.data_ptr(), m.numel(), ops,
                                      acc.data_ptr() if hwc else 0, 0, st)

        def randaug():
            nat.randaug(src.data_ptr(), dst.data_ptr(), N, H, W, hwc, 1234, gstep.data_ptr(), 3,
                        tab9.data_ptr(), tab9.numel(), list(range(14)), 0, st)
        if hwc:
            feed = lambda: nat.imagenet_u8_pack(src.data_ptr(), x_in.data_ptr(), N, H, W,  # noqa: E731
                                                1234, gstep.data_ptr(), 1, 0, 0, 0, st)
        else:
            feed = lambda: nat.cifar_augment(src.data_ptr(), x_in.data_ptr(), N, H, W, 8, 4,  # noqa: E731
                                             1234, gstep.data_ptr(), 1, 0, 0, 0, st)
        rows = [("input launch", feed), ("randaug, all ops, 3 per image", randaug)]
        rows += [(f"augmix w{w} depth {'drawn' if d < 0 else d}", mix(w, d))
                 for w in (1, 3, 4) for d in (-1, 1, 3)]
        for what, launch in rows:
            best, med = time_us(launch, reps if hwc else 10 * reps, batches)
            print(f"| {name} N={N} | {what} | {best:.1f} | {med:.1f} | "
                  f"{med / (STEP_MS[name] * 1e3) * 100:.2f} % |", flush=True)


if __name__ == "__main__":
    main()
