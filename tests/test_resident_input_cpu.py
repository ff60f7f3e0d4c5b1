"""The index function of the device-resident CIFAR input (data/cifar.py resident_index):
the specification the cifar_augment_resident kernel is tested against on the GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from distributed_tensorflow_resnet_amd.data.cifar import (resident_half_bits, resident_index,
                                                          resident_key, resident_perm,
                                                          resident_steps_per_epoch, splitmix)
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def _epoch_perm(key_seed, epoch, records):
    key = resident_key(key_seed, epoch)
    return np.array([resident_perm(key, p, records) for p in range(records)])


def test_splitmix_known_values():
    # the first output of splitmix64 seeded with 0 (the generator's public test vector)
    assert splitmix(0) == 0xE220A8397B1DCDAF
    assert 0 <= splitmix((1 << 64) - 1) < 1 << 64


@pytest.mark.parametrize("records", [1, 2, 3, 5, 257, 10000, 50000, 65536, 65537])
def test_shuffled_epoch_is_a_permutation(records):
    perm = _epoch_perm(7, 0, records)
    assert perm.min() == 0 and perm.max() == records - 1
    assert np.array_equal(np.sort(perm), np.arange(records))
    hb = resident_half_bits(records)
    assert records <= 1 << (2 * hb) <= max(4, 4 * records)   # the walk domain: at most 4x


def test_epochs_are_independent():
    a, b = _epoch_perm(7, 0, 50000), _epoch_perm(7, 1, 50000)
    assert (a != b).mean() > 0.99
    assert (a != np.arange(50000)).mean() > 0.99   # and neither is the identity


def test_rank_shards_are_disjoint_and_epochs_wrap():
    world, batch, records = 4, 16, 300
    S = resident_steps_per_epoch(records, batch, world)
    assert S == 4
    shards = []
    for rank in range(world):
        idx = [resident_index(3, step, n, batch, records, rank, world)
               for step in range(S) for n in range(batch)]
        assert len(set(idx)) == S * batch
        shards.append(set(idx))
    for i in range(world):
        for j in range(i + 1, world):
            assert not shards[i] & shards[j]
    union = set().union(*shards)
    assert len(union) == world * S * batch and max(union) < records
    # step S is k = 0 of epoch 1: position rank * per_rank + n of the epoch-1 permutation
    key1 = resident_key(3, 1)
    for rank in range(world):
        for n in (0, 5, 15):
            assert resident_index(3, S, n, batch, records, rank, world) == \
                resident_perm(key1, rank * S * batch + n, records)


def test_unshuffled_is_the_identity_on_positions():
    batch, records = 16, 70
    S = resident_steps_per_epoch(records, batch)
    for step in range(S):
        for n in range(batch):
            assert resident_index(9, step, n, batch, records, shuffle=False) == step * batch + n
    world = 4
    S4 = resident_steps_per_epoch(300, batch, world)
    for rank in range(world):
        for step in (0, S4 - 1, S4, 2 * S4 + 1):
            for n in (0, 15):
                assert resident_index(9, step, n, batch, 300, rank, world, shuffle=False) == \
                    rank * S4 * batch + (step % S4) * batch + n


def test_unshuffled_tail_batch_reads_the_first_record_of_the_batch():
    batch, records = 100, 250   # batches of 100, 100 and 50
    got = [resident_index(0, 2, n, batch, records, shuffle=False) for n in range(batch)]
    assert got[:50] == list(range(200, 250))
    assert got[50:] == [200] * 50
    assert resident_index(0, 3, 0, batch, records, shuffle=False) == 0   # the next pass


def test_validation():
    with pytest.raises(ValueError):
        resident_index(0, 0, 0, 16, 63, rank=0, world=4)   # records < batch * world
    with pytest.raises(ValueError):
        resident_steps_per_epoch(15, 16)
    with pytest.raises(ValueError):
        resident_index(0, 0, 0, 16, 300, rank=4, world=4)
    with pytest.raises(ValueError):
        resident_index(0, 0, 16, 16, 300)
    with pytest.raises(ValueError):
        resident_index(0, 0, 0, 1, 1 << 31)


def test_large_steps_stay_in_range():
    for step in (2 ** 31 + 3, 2 ** 40 + 1):
        idx = [resident_index(5, step, n, 16, 70) for n in range(16)]
        assert len(set(idx)) == 16 and 0 <= min(idx) and max(idx) < 70


CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DATA_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "distributed_tensorflow_resnet_amd", "csrc", "data.hip")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no ROCm compiler")
def test_resident_kernel_has_no_spills():
    """The compiler's kernel-resource-usage remarks (scripts/reg_usage.py): the resident
    input kernel keeps the register budget of cifar_augment_kernel<8> -- no spills, no
    scratch, full occupancy."""
    cmd = [CLANG, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--offload-device-only",
           "-c", "-x", "hip", DATA_HIP, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
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
    res = [r for n, r in rows.items() if "cifar_augment_resident_kernel" in n]
    old = [r for n, r in rows.items() if "cifar_augment_kernelILi8" in n]
    assert len(res) == 1 and len(old) == 1, sorted(rows)
    for r in res + old:
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
        assert int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r["Occupancy [waves/SIMD]"]) == 8, r


def test_resident_data_flag():
    p = build_parser("cifar")
    assert p.parse_args([]).resident_data is False
    assert p.parse_args(["--resident_data"]).resident_data is True
    assert p.parse_args(["--resident_data=false"]).resident_data is False
    assert p.parse_args(["--noresident_data"]).resident_data is False
