"""--optimizer lars without a GPU: the flags, the CPU backend's update against a
hand-written fp64 one, the CLI end to end (a lars checkpoint resumed by mom) and the
reference-API model wrapper."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import lars_tables
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils import tensor_bundle as tb
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_lars_flags(kind):
    f = build_parser(kind).parse_args([])
    assert (f.optimizer, f.lars_eeta, f.lars_epsilon, f.lars_skip) == ("mom", 0.001, 0.0, "vectors")
    f = build_parser(kind).parse_args(["--optimizer", "lars", "--lars_eeta", "0.02",
                                       "--lars_epsilon", "1e-6", "--lars_skip", "none"])
    assert (f.optimizer, f.lars_eeta, f.lars_epsilon, f.lars_skip) == ("lars", 0.02, 1e-6, "none")
    with pytest.raises(SystemExit):
        build_parser(kind).parse_args(["--lars_skip", "biases"])
    with pytest.raises(SystemExit):
        build_parser(kind).parse_args(["--optimizer", "lamb"])


def test_lars_tables():
    import numpy as np

    from distributed_tensorflow_resnet_amd.train.layout import LARS_CHUNK, SEG_DTYPE

    seg = np.zeros(4, dtype=SEG_DTYPE)
    seg["numel"] = [3, LARS_CHUNK, LARS_CHUNK + 1, 2 * LARS_CHUNK + 5]
    tab, blk = lars_tables(seg, [True, False, False, True])
    assert blk == [0, 1, 2, 2, 3, 3, 3]
    assert tab["chunk0"].tolist() == [0, 1, 2, 4] and tab["nchunks"].tolist() == [1, 1, 2, 3]
    assert tab["skip"].tolist() == [1, 0, 0, 1]


@pytest.mark.parametrize("skip", ["vectors", "none"])
def test_cpu_backend_lars_step_matches_fp64(skip):
    """Two steps (the second from a non-zero accumulator and non-zero betas) against the
    update written out in fp64 from the backend's own fp32 gradient."""
    spec = cifar_spec(8)
    wd, lr, momentum, eeta, eps = 5e-4, 0.1, 0.9, 0.02, 1e-6
    be = CPUBackend(spec, 4, weight_decay=wd, lr_schedule=constant_lr(lr), optimizer="lars",
                    momentum=momentum, lars_eeta=eeta, lars_epsilon=eps, lars_skip=skip)
    assert be.lars_state() is None and be.lars_summary() is None
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 32, 32, 3, generator=gen)
    y = torch.randint(0, 10, (4,), generator=gen)
    for step in range(2):
        w0, m0 = be.store.master.detach().clone().double(), be.mom.clone().double()
        be.set_batch(x, y)
        be.step()
        g = be.store.master.grad.detach().double()
        w1, m1 = w0.clone(), m0.clone()
        adapted = 0
        for s in be.store.train_slots:
            sl = slice(s.offset, s.offset + s.numel)
            wn, gn = float(w0[sl].norm()), float(g[sl].norm())
            trust = 1.0
            if not (skip == "vectors" and len(s.shape) == 1) and wn > 0 and gn > 0:
                trust = eeta * wn / (gn + wd * wn + eps)
                adapted += 1
            m1[sl] = momentum * m0[sl] + g[sl] + wd * w0[sl]
            w1[sl] = w0[sl] - lr * trust * m1[sl]
            wn_b, gn_b, t_b = be.lars_state()[s.name]
            assert t_b == pytest.approx(trust, rel=1e-5) and (trust != 1.0 or t_b == 1.0)
            assert wn_b == pytest.approx(wn, rel=1e-5) and gn_b == pytest.approx(gn, rel=1e-5)
        rank2 = sum(len(s.shape) > 1 for s in be.store.train_slots)
        assert adapted >= (rank2 if skip == "vectors" else rank2 + 1)
        torch.testing.assert_close(be.mom.double(), m1, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(be.store.master.detach().double(), w1, rtol=1e-5, atol=1e-7)
        # the update moved the weights by far more than the tolerance
        assert float((w1 - w0).abs().max()) > 1e-4
        summary = be.lars_summary()
        assert summary["lars_trust_min"] <= summary["lars_trust_median"] <= summary["lars_trust_max"]
    with pytest.raises(ValueError):
        CPUBackend(spec, 4, weight_decay=wd, lr_schedule=constant_lr(lr), optimizer="lamb")


def _cli(args):
    e = dict(os.environ)
    e.update({"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": "", "OMP_NUM_THREADS": "2"})
    return subprocess.run([sys.executable, "resnet_cifar_main.py", "--device", "cpu", "--synthetic",
                           "--resnet_size", "8", "--batch_size", "4", "--log_every", "1",
                           "--summary_every", "1"] + args,
                          cwd=ROOT, capture_output=True, text=True, timeout=600, env=e)


def test_cli_lars_checkpoint_resumed_by_momentum(tmp_path):
    td, ld = str(tmp_path / "train"), str(tmp_path / "log")
    r = _cli(["--optimizer", "lars", "--train_steps", "3", "--train_dir", td, "--log_dir", ld])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert tb.latest_checkpoint(td).endswith("model.ckpt-3")
    assert "lars trust min/median/max" in r.stdout + r.stderr
    rows = [json.loads(line) for line in open(os.path.join(ld, "metrics.jsonl"))]
    assert len(rows) == 3
    for row in rows:
        assert 0 < row["lars_trust_min"] <= row["lars_trust_median"] <= row["lars_trust_max"]
    r = _cli(["--optimizer", "mom", "--train_steps", "5", "--train_dir", td])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Restoring parameters from" in r.stdout + r.stderr
    assert tb.latest_checkpoint(td).endswith("model.ckpt-5")
    assert "lars trust" not in r.stdout + r.stderr


def test_hparams_lars_is_accepted():
    import resnet_model

    hps = resnet_model.HParams(num_classes=10, lrn_rate=0.5, weight_decay_rate=2e-4,
                               optimizer="lars")
    torch.manual_seed(0)
    x = torch.randn(8, 32, 32, 3)
    y = torch.nn.functional.one_hot(torch.randint(0, 10, (8,)), 10).float()
    m = resnet_model.ResNet(hps, x, y, "train", resnet_size=8)
    m.build_graph()
    vs = [v.detach().clone() for v in m.network.trainable_variables()]
    grads_seen = m.train_op()
    assert grads_seen == 1 and m.global_step == 1
    moved = [float((a - b.detach()).norm() / (a.norm() + 1e-12))
             for a, b in zip(vs, m.network.trainable_variables()) if a.dim() > 1]
    # a rank > 1 variable moves by lr * eeta * |acc| / (|g^| + wd |w|) of its norm: about
    # lr * eeta = 5e-4 here, where 'mom' at this rate would move it by far more
    assert all(0 < r < 5.5e-4 for r in moved), moved
