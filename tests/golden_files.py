"""The reference's trained CIFAR-10 ResNet-50 artefacts, stored with the tests under
tests/golden/resnet50-cifar-ckpt-20190218/ (data only: see tests/golden/README.md).

Two of them are larger than the repository takes in one file, so they are stored
packed and put together here, once per process, in a temporary directory that is
removed at exit:
  - the frozen graph (.pb, weights as Const nodes): consecutive byte ranges
    `<name>.pb.part0 ..`, concatenated in order;
  - the training meta graph (model.ckpt-107738.meta): gzip.
The SHA-256 of each rebuilt file is checked against the one recorded beside it.
"""
import atexit
import glob
import gzip
import hashlib
import os
import shutil
import tempfile

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPT_DIR = os.path.join(GOLDEN, "resnet50-cifar-ckpt-20190218")
EVAL_META = os.path.join(CKPT_DIR, "resnet50_cifar_eval_graph.meta")
INDEXES = sorted(glob.glob(os.path.join(CKPT_DIR, "model.ckpt-*.index")))

_PB = "resnet50_cifar_frozen_model_eval.pb"
_TRAIN_META = "model.ckpt-107738.meta"
_scratch = None
_built = {}


def _scratch_dir() -> str:
    global _scratch
    if _scratch is None:
        _scratch = tempfile.mkdtemp(prefix="dtr_golden_")
        atexit.register(shutil.rmtree, _scratch, ignore_errors=True)
    return _scratch


def _rebuild(name: str, data: bytes) -> str:
    with open(os.path.join(CKPT_DIR, name + ".sha256")) as fh:
        want = fh.read().split()[0]
    got = hashlib.sha256(data).hexdigest()
    assert got == want, f"tests/golden: {name} rebuilt with sha256 {got}, recorded {want}"
    path = os.path.join(_scratch_dir(), name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def frozen_pb() -> str:
    """Path of the reference's frozen eval graph, rebuilt from its parts."""
    if _PB not in _built:
        parts = sorted(glob.glob(os.path.join(CKPT_DIR, _PB + ".part*")),
                       key=lambda p: int(p.rsplit("part", 1)[1]))
        assert parts, f"tests/golden: no parts of {_PB}"
        data = b"".join(open(p, "rb").read() for p in parts)
        _built[_PB] = _rebuild(_PB, data)
    return _built[_PB]


def train_meta() -> str:
    """Path of the reference's training meta graph (step 107738), gunzipped."""
    if _TRAIN_META not in _built:
        with gzip.open(os.path.join(CKPT_DIR, _TRAIN_META + ".gz"), "rb") as fh:
            data = fh.read()
        _built[_TRAIN_META] = _rebuild(_TRAIN_META, data)
    return _built[_TRAIN_META]
