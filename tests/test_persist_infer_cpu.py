"""Host-side checks of the persistent inference forward (no GPU): the network-shape
predicate, the kernel's compile-time register budget and its tuning key."""
import os
import re

import pytest

import kernel_resources as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shape_predicate():
    from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
    from distributed_tensorflow_resnet_amd.train.persist import shape_check

    for depth in (8, 20, 50, 110):
        for classes in (10, 100):
            assert shape_check(cifar_spec(depth, num_classes=classes)) == "", (depth, classes)
    assert shape_check(imagenet_spec(18)) == "not a CIFAR network"
    assert shape_check(cifar_spec(8, image_hw=64)) != ""
    assert shape_check(cifar_spec(8), stem_s2d=True) != ""


@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
def test_inference_kernel_resources():
    rows = kr.prn_resources()
    inf = {n: r for n, r in rows.items() if "prn_infer_kernel" in n}
    assert len(inf) == 1, sorted(rows)
    (name, r), = inf.items()
    print(name, r)
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["Occupancy [waves/SIMD]"]) >= 2, r
    # the training kernels' count (tests/test_kernel_resources_cpu.py) is unchanged
    prn = [n for n in rows if "prn_fwd_kernel" in n or "prn_bwd_kernel" in n]
    assert len(prn) == 6, sorted(rows)


def test_tune_key():
    from distributed_tensorflow_resnet_amd.utils import tune

    assert "persist_eval" in tune.ENGINE
    text = open(os.path.join(ROOT, "README.md")).read()
    m = re.search(r"^\|\s*`persist_eval`\s*\|\s*([^|]+?)\s*\|", text, re.M)
    assert m, "README.md 'Knobs' has no persist_eval row"
    assert m.group(1) == str(tune.ENGINE["persist_eval"][0])
    assert tune.ENGINE["persist_eval"][0] == -1


def _prn_args():
    """A PrnArgs dict (train/persist.py PersistStep.args' keys) with a valid shape and null
    pointers: recorded into a Plan, never run."""
    ptrs = ("blocks", "bns", "x_in", "stem_w", "pool_acc", "bar", "err", "dense_w", "dense_b",
            "labels", "pooled", "dlogits", "ws", "dpool", "loss_sum", "correct", "dbias",
            "dense_grad", "dx0", "items")
    args = {k: 0 for k in ptrs}
    args.update(nblocks=3, nitems=0, N=4, P=2, classes=10, kpad=16, grad_scale=0.25,
                momentum=0.9, eps=1e-5, update_moving=1, overlap=0,
                bucket_of_stage=(-1, -1, -1), fault_bar=-1, wgrad_wgs=1)
    return args


def test_prn_args_are_named():
    """Plan.prn takes one dict keyed by the PrnArgs member names: a complete dict records
    an op; a missing key and an unknown key each raise, naming the key."""
    from distributed_tensorflow_resnet_amd import _C

    plan = _C.Plan()
    for mode in (0, 1, 2):
        n = plan.size()
        plan.prn(mode, _prn_args())
        assert plan.size() == n + 1
    n = plan.size()
    short = _prn_args()
    del short["dense_grad"]
    with pytest.raises(ValueError, match="dense_grad"):
        plan.prn(1, short)
    extra = _prn_args()
    extra["fault_barr"] = 3
    with pytest.raises(ValueError, match="fault_barr"):
        plan.prn(0, extra)
    assert plan.size() == n
