"""Host-side checks of the persistent inference forward (no GPU): the network-shape
predicate, the kernel's compile-time register budget and its tuning key."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed_tensorflow_resnet_amd", "csrc", "cifar_persist.hip")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_shape_predicate():
    from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
    from distributed_tensorflow_resnet_amd.train.persist import shape_check

    for depth in (8, 20, 50, 110):
        for classes in (10, 100):
            assert shape_check(cifar_spec(depth, num_classes=classes)) == "", (depth, classes)
    assert shape_check(imagenet_spec(18)) == "not a CIFAR network"
    assert shape_check(cifar_spec(8, image_hw=64)) != ""
    assert shape_check(cifar_spec(8), stem_s2d=True) != ""


def _resources(src):
    """tests/test_kernel_resources_cpu.py's recipe: the compiler's resource remarks."""
    cmd = [CLANG, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--offload-device-only",
           "-c", "-x", "hip", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rows, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: +([A-Za-z /\[\]]+?): (\S+) \[", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = rows.setdefault(v, {})
        elif cur is not None:
            cur[k] = v
    return rows


@pytest.mark.skipif(not os.path.exists(CLANG) and shutil.which("hipcc") is None,
                    reason="no ROCm compiler")
def test_inference_kernel_resources():
    rows = _resources(SRC)
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
