"""The optimizer kernels give the recorded bits: every buffer of every case of
tests/optim_bits.py against tests/golden/optim_bits.json (scripts/record_optim_bits.py wrote
it on the commit before the walks were shared in csrc/optim_device.h)."""
import json
import os

import pytest

import optim_bits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_bits.json")


def test_optimizer_kernels_give_the_recorded_bits(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    with open(GOLDEN) as fh:
        want = json.load(fh)["cases"]
    got = optim_bits.run(dtr.native(required=True), gpu)
    assert sorted(got) == sorted(want)
    bad = [(case, buf) for case in want for buf in want[case]
           if got[case].get(buf) != want[case][buf]]
    assert not bad, (len(bad), bad[:12])
    assert all(sorted(got[c]) == sorted(want[c]) for c in want)
