"""Device-resident CIFAR input (csrc/data.hip cifar_augment_resident_kernel; Engine
input_mode='cifar_resident'; GPUInference.attach; --resident_data): the kernel against
the host specification data.cifar.resident_index and against cifar_augment, the
resident training step against the host-fed step, resume continuity, the evaluator and
the CLI."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_resnet_amd.data import cifar
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.ops import functional as F
from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.evaluator import GPUInference, evaluate_checkpoint
from distributed_tensorflow_resnet_amd.utils import tensor_bundle as tb
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEY_SEED, DATA_SEED = 11, 4321
STEPS = list(range(10)) + [2 ** 31 + 3, 2 ** 40 + 1]   # S = 4: two epoch boundaries


@functools.lru_cache(maxsize=None)
def _split(records, seed=0):
    """Random CIFAR-shaped records + labels (host, shared, never modified)."""
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (records, 3, 32, 32), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (records,), generator=g)
    return imgs, labels


def _on_device(records, gpu):
    imgs, labels = _split(records)
    return imgs.to(gpu), labels.to(device=gpu, dtype=torch.int32)


def _pos(step, gpu):
    return torch.tensor([step], dtype=torch.int64, device=gpu)


# ---------------------------------------------------------------- 1. index parity
@pytest.mark.parametrize("records,batch,world,steps", [
    (70, 16, 1, STEPS),          # S = 4, a tail of 6
    (300, 16, 4, STEPS),         # four rank shards (kernel arguments only)
    (65537, 16, 1, [0, 1]),      # the walk domain is 4x the records
])
def test_index_and_labels_match_the_host_function(gpu, records, batch, world, steps):
    rec, lab = _on_device(records, gpu)
    lab_host = _split(records)[1].numpy()
    for rank in range(world):
        for step in steps:
            _, labels, idx = F.cifar_augment_resident(
                rec, lab, _pos(step, gpu), batch, seed=DATA_SEED, key_seed=KEY_SEED, rank=rank,
                world=world, log_index=True)
            ref = cifar.resident_batch(KEY_SEED, step, batch, records, rank, world)
            assert np.array_equal(idx.cpu().numpy(), ref), (rank, step)
            assert np.array_equal(labels.cpu().numpy(), lab_host[ref]), (rank, step)


def test_unshuffled_tail_batch_on_the_device(gpu):
    rec, lab = _on_device(250, gpu)
    for step in (0, 2, 3):
        _, _, idx = F.cifar_augment_resident(rec, lab, _pos(step, gpu), 100, shuffle=False,
                                             train=False, log_index=True)
        ref = cifar.resident_batch(0, step, 100, 250, shuffle=False)
        assert np.array_equal(idx.cpu().numpy(), ref), step


# ---------------------------------------------------------------- 2. bit equality
@pytest.mark.parametrize("train", [1, 0])
def test_output_is_bit_identical_to_cifar_augment(gpu, train):
    records, batch = 70, 16
    rec, lab = _on_device(records, gpu)
    for step in STEPS:
        zero = torch.ones(1024, device=gpu)
        pos = _pos(step, gpu)
        out, _, crops = F.cifar_augment_resident(rec, lab, pos, batch, seed=DATA_SEED,
                                                 key_seed=KEY_SEED, train=train, zero=zero,
                                                 log_crops=True)
        ref_idx = torch.from_numpy(cifar.resident_batch(KEY_SEED, step, batch, records)).to(gpu)
        ref, ref_crops = F.cifar_augment(rec[ref_idx].contiguous(), seed=DATA_SEED, gstep=pos,
                                         train=bool(train), log_crops=True)
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), step
        assert torch.equal(crops, ref_crops), step
        assert not zero.any(), step


# ---------------------------------------------------------------- 3. step equality
N_STEPS, BATCH, RECORDS = 6, 16, 70   # the epoch boundary is crossed at step 4


def _engine(gpu, persist, resident, size=8, use_graph=False):
    kw = dict(weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu, seed=3,
              data_seed=DATA_SEED, use_graph=use_graph)
    old = os.environ.get("DTR_TUNE")
    os.environ["DTR_TUNE"] = f"persist={persist}"
    try:
        if resident:
            eng = Engine(cifar_spec(size), BATCH, input_mode="cifar_resident",
                         resident=_split(RECORDS), shuffle_seed=KEY_SEED, **kw)
        else:
            eng = Engine(cifar_spec(size), BATCH, input_mode="cifar_u8", **kw)
    finally:
        if old is None:
            del os.environ["DTR_TUNE"]
        else:
            os.environ["DTR_TUNE"] = old
    assert eng.persist == (persist == 1)
    return eng


def _state(eng):
    torch.cuda.synchronize()
    assert not eng.persist_error()
    return {"master": eng.params.master.clone(), "mom": eng.mom.clone(),
            "stats": eng.params.stats.clone(), "gstep": eng.gstep.clone()}


def _assert_same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


@functools.lru_cache(maxsize=None)
def _fed_reference(persist, size=8):
    """N_STEPS steps of the host-fed cifar_u8 engine on records[resident_index(step)]."""
    gpu = torch.device("cuda:0")
    eng = _engine(gpu, persist, resident=False, size=size)
    imgs, labels = _split(RECORDS)
    for step in range(N_STEPS):
        idx = cifar.resident_batch(KEY_SEED, step, BATCH, RECORDS)
        eng.set_batch(imgs[idx], labels[idx])
        eng.step()
    return _state(eng)


@functools.lru_cache(maxsize=None)
def _resident_reference(persist):
    eng = _engine(torch.device("cuda:0"), persist, resident=True)
    assert (eng.records, eng.steps_per_epoch) == (RECORDS, 4)
    for _ in range(N_STEPS):
        eng.step()
    return _state(eng)


@pytest.mark.parametrize("persist", [1, 0])
def test_resident_step_equals_host_fed_step(gpu, persist):
    got = _resident_reference(persist)
    assert int(got["gstep"].item()) == N_STEPS
    _assert_same(got, _fed_reference(persist))


def test_resident_step_equals_host_fed_step_resnet14(gpu):
    eng = _engine(gpu, 1, resident=True, size=14)
    for _ in range(N_STEPS):
        eng.step()
    _assert_same(_state(eng), _fed_reference(1, size=14))


def test_resident_step_under_graph_replay(gpu):
    eng = _engine(gpu, 1, resident=True, use_graph=True)
    done = eng.capture(warmup=2)
    for _ in range(N_STEPS - done):
        eng.step()
    assert eng.graph is not None
    _assert_same(_state(eng), _fed_reference(1))


# ---------------------------------------------------------------- 4. resume
def test_resume_continues_the_epoch(gpu, tmp_path):
    first = _engine(gpu, 1, resident=True)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    saver = Saver(str(tmp_path))
    prefix = saver.save(GPUBackend(first).state_tensors(), 3)
    second = GPUBackend(_engine(gpu, 1, resident=True))
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 3
    for _ in range(3):
        second.step()
    _assert_same(_state(second.engine), _resident_reference(1))


# ---------------------------------------------------------------- 5. evaluator
@pytest.mark.parametrize("persist_eval", [1, 0])
def test_evaluator_resident_split_matches_host_fed(gpu, tmp_path, monkeypatch, persist_eval):
    records, bs = 250, 100   # batches of 100, 100 and 50
    imgs, labels = _split(records, seed=5)
    trained = _engine(gpu, 1, resident=True)
    for _ in range(2):
        trained.step()
    prefix = Saver(str(tmp_path)).save(GPUBackend(trained).state_tensors(), 2)
    monkeypatch.setenv("DTR_TUNE", f"persist_eval={persist_eval}")
    model = GPUInference(cifar_spec(8), bs, device=gpu)
    assert model.eval_path == ("persistent" if persist_eval else "per-layer")

    def batches():
        for s in range(0, records, bs):
            yield imgs[s:s + bs], labels[s:s + bs]

    host = evaluate_checkpoint(model, prefix, batches, 50)
    assert not model.attached
    model.attach(imgs.numpy(), labels.numpy())
    assert model.attached and model.resident_batch_sizes() == [100, 100, 50]
    res = evaluate_checkpoint(model, prefix, None, 50)
    print(f"host-fed {host}  resident {res}")
    assert res[0] == host[0] and res[2] == host[2] == 2
    assert abs(res[1] - host[1]) <= 1e-6 * abs(host[1])
    # eval_batch_count caps the resident path too
    two = evaluate_checkpoint(model, prefix, None, 2)
    correct2 = sum(model.run(x, y)[1] for x, y in list(batches())[:2])
    assert two[0] == correct2 / 200


# ---------------------------------------------------------------- 6. driver
def test_driver_resident_data(gpu, tmp_path):
    records, batch = 336, 16   # 21 steps per epoch
    imgs, labels = _split(records, seed=9)
    data = str(tmp_path / "train.bin")
    cifar.write_records(data, imgs.numpy(), labels.numpy())
    td = str(tmp_path / "train")
    r = subprocess.run(
        [sys.executable, "resnet_cifar_main.py", "--device", "gpu", "--resident_data",
         "--mode", "train_and_eval", "--resnet_size", "8", "--batch_size", str(batch),
         "--train_data_path", data, "--eval_data_path", data, "--train_dir", td,
         "--train_steps", "40", "--num_epochs", "1", "--log_every", "7",
         "--eval_batch_size", "100", "--eval_batch_count", "3"],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "resident data: 336 records, 21 steps per epoch, 1032192 bytes" in out, out[-4000:]
    # one epoch of 21 steps ends the run before --train_steps 40
    assert "training done: global_step=21," in out, out[-4000:]
    assert tb.latest_checkpoint(td).endswith("model.ckpt-21")
    assert "resident eval data: 300 records, 3 batches" in out, out[-4000:]
    assert "best precision" in out, out[-4000:]


# ---------------------------------------------------------------- 7. refusals
def test_refusals(gpu):
    eng = _engine(gpu, 1, resident=True)
    imgs, labels = _split(RECORDS)
    with pytest.raises(RuntimeError, match="cifar_resident"):
        eng.set_batch(imgs[:BATCH], labels[:BATCH])
    with pytest.raises(RuntimeError, match="cifar_resident"):
        eng.fill_synthetic(0)
    assert not hasattr(eng, "img_u8")
    rec, lab = _on_device(70, gpu)
    with pytest.raises(ValueError, match="records < batch"):
        F.cifar_augment_resident(rec, lab, _pos(0, gpu), 16, world=8)
    with pytest.raises(ValueError, match="rank"):
        F.cifar_augment_resident(rec, lab, _pos(0, gpu), 16, rank=1, world=1)
    with pytest.raises(ValueError, match="zero_bytes"):
        F.cifar_augment_resident(rec, lab, _pos(0, gpu), 16,
                                 zero=torch.zeros(3, device=gpu))
    with pytest.raises(ValueError, match="batch"):
        Engine(cifar_spec(8), 128, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(),
               device=gpu, input_mode="cifar_resident", resident=_split(RECORDS))
