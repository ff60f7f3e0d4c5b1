"""The compiler's kernel-resource-usage remarks of the persistent CIFAR kernels (no GPU):
one recipe, applied to the three `csrc/prn_*.hip` translation units, each compiled once per
test session (scripts/reg_usage.py does the same for any file)."""
import functools
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_tensorflow_resnet_amd", "csrc")
PRN_SOURCES = tuple(os.path.join(CSRC, f) for f in ("prn_fwd.hip", "prn_bwd.hip", "prn_infer.hip"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def have_compiler():
    return os.path.exists(CLANG) or shutil.which("hipcc") is not None


@functools.lru_cache(maxsize=None)
def _resources(src):
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


OPTIM_SOURCES = tuple(os.path.join(CSRC, f + ".hip") for f in ("optim", "lars", "clip", "adam", "lamb"))


def optimizer_resources():
    """[(kernel function name, {remark: value})] over the optimizer files: the name demangled
    as far as the identifier, so a template's instantiations share one."""
    rows = []
    for src in OPTIM_SOURCES:
        for name, r in _resources(src).items():
            m = re.match(r"_ZN3dtr\d+([a-z0-9_]+?_kernel)", name)
            rows.append((m.group(1) if m else name, r))
    return rows


def prn_resources():
    """{kernel name: {remark: value}} over the persistent kernels' three files."""
    rows = {}
    for src in PRN_SOURCES:
        rows.update(_resources(src))
    return rows
