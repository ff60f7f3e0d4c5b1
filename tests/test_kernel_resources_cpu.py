"""Register budget of the persistent CIFAR kernels, pinned at compile time (no GPU): every
`prn_*` kernel compiles for gfx950 without VGPR spills or scratch, and the forward and
backward keep one 512-thread workgroup's worth of waves resident (>= 2 waves per SIMD).
A spill inside these kernels is a memory round trip on the critical path of a launch
whose cost is already its round trips (`profiles/cifar_persist_v2.md`: removing the
backward's 9-43 spills took bs32 0.631 -> 0.611 ms).

Uses the compiler's kernel-resource-usage remarks (tests/kernel_resources.py).
"""
import pytest

import kernel_resources as kr


@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
def test_persistent_kernels_have_no_spills():
    rows = kr.prn_resources()
    prn = {n: r for n, r in rows.items() if "prn_fwd_kernel" in n or "prn_bwd_kernel" in n}
    assert len(prn) == 6, sorted(rows)   # forward and backward at 1, 2 and 4 slices
    for name, r in prn.items():
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r)
