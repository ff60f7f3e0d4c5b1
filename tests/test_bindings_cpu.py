"""The arity surface of the op bindings (no GPU): which positional arities each op with
optional trailing arguments takes, what a call without them means, and the texts of the
argument checks the flat-update ops share.

Makers only check and bind their arguments, so a `Plan` records these ops with dummy
pointers and is never run.  An immediate op (trailing stream) would launch, so the immediate
forms are only called where the call is known to raise first: at an arity that is not
registered, or with an argument the maker rejects.  Their full arity sets are read from the
signatures pybind11 writes into the docstrings."""
import re

import pytest

P = 0x1000              # a non-null, 16-byte aligned dummy pointer
ODD = 0x1008            # non-null, not 16-byte aligned
PIECEWISE = ("piecewise", 0, 0.0, 0.0)

SCHED = [("init", 0.1), ("warm_steps", 0), ("warm_from", 0.0), ("warm_to", 0.1),
         ("bounds", [10]), ("vals", [0.1, 0.01])]
DECAY = [("decay", PIECEWISE)]

LOSS_LS = [("label_smoothing", 0.0), ("topk", 0)]
LOSS_MIX = [("labels_b", 0), ("mix_lam", 0)]
LOSS_KD = [("teacher", 0), ("kd_alpha", 0.0), ("kd_inv_tau", 1.0)]
LOSS_JSD = [("jsd_B", 0), ("jsd_weight", 0.0)]

MIX = [("table", 0), ("table_len", 0), ("labels", 0), ("labels_b", 0), ("mix_lam", 0),
       ("mix_log", 0)]
CUT = [("cut_table", 0), ("cut_thresh", 0), ("cut_log", 0)]

# op -> (argument groups, an override the maker rejects at every arity that has the argument;
# None where the maker checks nothing).
# The first group is the shortest arity; every further group is one more registered arity
# and holds the documented defaults, so the concatenation is a long call with the defaults
# written out.
OPS = {
    "softmax_xent": ([
        [("logits", P), ("ld", 16), ("labels", P), ("N", 6), ("classes", 10), ("loss_sum", P),
         ("correct", P), ("dlogits", P), ("dbias", P), ("grad_scale", 1.0), ("probs", 0),
         ("ws", P)],
        LOSS_LS + [("topk_out", 0)], LOSS_MIX, LOSS_KD, LOSS_JSD], {"label_smoothing": 2.0}),
    "head_fused": ([
        [("x", P), ("bn", [P] * 9), ("momentum", 0.9), ("eps", 1e-5), ("update_moving", 1),
         ("w", P), ("bias", P), ("labels", P), ("shape", [6, 64, 16, 10, 16]),
         ("grad_scale", 1.0), ("out", [P] * 5)],
        LOSS_LS, LOSS_MIX, LOSS_KD, LOSS_JSD], {"bn": [P] * 8}),
    "softmax_xent_reduce": ([
        [("ws", P), ("ld", 16), ("N", 6), ("classes", 10), ("loss_sum", P), ("correct", P),
         ("dbias", P)],
        [("topk_out", 0)]], None),
    "cifar_augment": ([
        [("img", P), ("out", P), ("N", 4), ("H", 32), ("W", 32), ("Cpad", 8), ("pad", 4),
         ("seed", 1), ("gstep", P), ("train", 1), ("crop_log", 0), ("zero", 0),
         ("zero_bytes", 0)],
        MIX, CUT], {"zero_bytes": 8}),
    "cifar_augment_resident": ([
        [("records_u8", P), ("labels_all", P), ("out", P), ("labels_out", P), ("pos", P),
         ("N", 4), ("H", 32), ("W", 32), ("Cpad", 8), ("records", 100), ("rank", 0),
         ("world", 1), ("shuffle", 1), ("key_seed", 1), ("pad", 4), ("seed", 1), ("train", 1),
         ("crop_log", 0), ("idx_log", 0), ("zero", 0), ("zero_bytes", 0)],
        [kv for kv in MIX if kv[0] != "labels"], CUT], {"H": 31}),
    "imagenet_u8_pack": ([
        [("img", P), ("out", P), ("N", 2), ("H", 224), ("W", 224), ("seed", 1), ("gstep", P),
         ("train", 1), ("zero", 0), ("zero_bytes", 0), ("s2d", 1)],
        MIX, CUT], {"zero_bytes": 8}),
    "augmix": ([
        [("img", 0x10000), ("out", 0x100000), ("N", 6), ("H", 32), ("W", 32), ("hwc", 0),
         ("seed", 1), ("gstep", P), ("width", 1), ("depth", -1), ("tables", P),
         ("table_len", 64), ("mix", P), ("mix_ints", 2), ("op_ids", [0, 1]), ("acc", 0),
         ("log", 0)],
        [("fan_B", 0), ("labels", 0)]], {"op_ids": []}),
    "sgd_update_pack": ([
        [("master", P), ("grad", P), ("mom", P), ("n", 64)] + SCHED +
        [("gstep", P), ("momentum", 0.9), ("wd", 1e-4), ("grad_scale", 1.0),
         ("use_momentum", 1), ("segs", P), ("nseg", 1), ("bf", P), ("lr_out", P),
         ("update", 1)],
        DECAY], {"vals": []}),
    "sgd_tiles": ([
        [("master", P), ("grad", P), ("mom", P)] + SCHED +
        [("gstep", P), ("momentum", 0.9), ("wd", 1e-4), ("grad_scale", 1.0),
         ("use_momentum", 1), ("segs", P), ("work", P), ("blk_seg", P), ("nblocks", 1),
         ("bf", P), ("lr_out", P), ("ticket", P), ("gin", 0), ("gout", 0), ("pack", 1)],
        DECAY], {"vals": []}),
    "lars_update_pack": ([
        [("master", P), ("grad", P), ("mom", P), ("n", 64)] + SCHED +
        [("gstep", P), ("momentum", 0.9), ("wd", 1e-4), ("grad_scale", 1.0), ("segs", P),
         ("nseg", 1), ("trust", P), ("bf", P), ("lr_out", P)],
        DECAY], {"vals": []}),
    "sgd_clip_update_pack": ([
        [("master", P), ("grad", P), ("mom", P), ("n", 64)] + SCHED +
        [("gstep", P), ("momentum", 0.9), ("wd", 1e-4), ("clip", P), ("use_momentum", 1),
         ("segs", P), ("nseg", 1), ("bf", P), ("lr_out", P)],
        DECAY], {"vals": []}),
    "adam_update_pack": ([
        [("master", P), ("grad", P), ("m", P), ("v", P), ("n", 64)] + SCHED +
        [("gstep", P), ("start_step", P), ("beta1", 0.9), ("beta2", 0.999), ("epsilon", 1e-8),
         ("grad_scale", 1.0), ("clip", 0), ("decay_mode", "decoupled"), ("segs", P),
         ("nseg", 1), ("wd_seg", P), ("bf", P), ("lr_out", P), ("adam_out", 0)],
        DECAY], {"vals": []}),
    "lion_update_pack": ([
        [("master", P), ("grad", P), ("m", P), ("n", 64)] + SCHED +
        [("gstep", P), ("beta1", 0.9), ("beta2", 0.99), ("grad_scale", 1.0), ("clip", 0),
         ("segs", P), ("nseg", 1), ("wd_seg", P), ("bf", P), ("lr_out", P)],
        DECAY], {"vals": []}),
    "rmsprop_update_pack": ([
        [("master", P), ("grad", P), ("ms", P), ("mg", 0), ("mom", P), ("n", 64)] + SCHED +
        [("gstep", P), ("rho", 0.9), ("momentum", 0.9), ("epsilon", 1e-3),
         ("grad_scale", 1.0), ("clip", 0), ("centered", 0), ("decay_mode", "l2"), ("segs", P),
         ("nseg", 1), ("wd_seg", P), ("bf", P), ("lr_out", P)],
        DECAY], {"vals": []}),
    "muon_update_pack": ([
        [("master", P), ("grad", P), ("mom", P), ("dir", P), ("n", 64)] + SCHED +
        [("gstep", P), ("momentum", 0.9), ("wd", 1e-4), ("aux_scale", 1.0),
         ("grad_scale", 1.0), ("segs", P), ("nseg", 1), ("muon_seg", P), ("q_seg", P),
         ("bf", P), ("lr_out", P)],
        DECAY], {"vals": []}),
    "shampoo_update_pack": ([
        [("master", P), ("grad", P), ("mom", P), ("dir", P), ("n", 64)] + SCHED +
        [("gstep", P), ("momentum", 0.9), ("wd", 1e-4), ("grad_scale", 1.0), ("segs", P),
         ("nseg", 1), ("pre_seg", P), ("graft", P), ("bf", P), ("lr_out", P)],
        DECAY], {"vals": []}),
    "lamb_update_pack": ([
        [("master", P), ("m", P), ("v", P), ("n", 64)] + SCHED +
        [("gstep", P), ("start_step", P), ("beta1", 0.9), ("beta2", 0.999), ("epsilon", 1e-6),
         ("decay_mode", "decoupled"), ("segs", P), ("nseg", 1), ("wd_seg", P), ("trust", P),
         ("bf", P), ("lr_out", P), ("adam_out", 0)],
        DECAY], {"vals": []}),
}

# one arity only, but it shares the flat-update checks
LAMB_MOMENTS_NORMS = [
    ("master", P), ("grad", P), ("m", P), ("v", P), ("gstep", P), ("start_step", P),
    ("beta1", 0.9), ("beta2", 0.999), ("epsilon", 1e-6), ("grad_scale", 1.0), ("clip", 0),
    ("decay_mode", "decoupled"), ("segs", P), ("lsegs", P), ("blk_seg", P), ("nblocks", 1),
    ("wd_seg", P), ("part", P)]

HEADS = {
    "softmax_xent": [12, 15, 17, 20, 22],
    "head_fused": [11, 13, 15, 18, 20],
    "softmax_xent_reduce": [7, 8],
    "cifar_augment": [13, 19, 22],
    "cifar_augment_resident": [21, 26, 29],
    "imagenet_u8_pack": [11, 17, 20],
    "augmix": [17, 19],
    "sgd_update_pack": [20, 21],
    "sgd_tiles": [24, 25],
    "lars_update_pack": [19, 20],
    "sgd_clip_update_pack": [19, 20],
    "adam_update_pack": [25, 26],
    "lion_update_pack": [20, 21],
    "rmsprop_update_pack": [25, 26],
    "muon_update_pack": [22, 23],
    "shampoo_update_pack": [21, 22],
    "lamb_update_pack": [23, 24],
}


@pytest.fixture(scope="module")
def C():
    from distributed_tensorflow_resnet_amd import _C

    return _C


def _pairs(op):
    if op == "lamb_moments_norms":
        return list(LAMB_MOMENTS_NORMS)
    return [kv for group in OPS[op][0] for kv in group]


def _args(op, count=None, /, **over):
    """The first `count` (default: all) arguments of `op`, defaults written out, with
    overrides by name."""
    pairs = _pairs(op)
    unknown = set(over) - {k for k, _ in pairs}
    assert not unknown, (op, unknown)
    vals = [over.get(k, v) for k, v in pairs]
    return vals if count is None else vals[:count]


def _record(C, op, args):
    """Record `op` on a fresh plan; it must add exactly one op."""
    plan = C.Plan()
    getattr(plan, op)(*args)
    assert plan.size() == 1, op


def _rejects(C, op, args, text=None):
    """The recorder raises ValueError (with exactly `text`) and records nothing."""
    plan = C.Plan()
    with pytest.raises(ValueError) as e:
        getattr(plan, op)(*args)
    if text is not None:
        assert str(e.value) == text
    assert plan.size() == 0, op


def _doc_arities(fn, name):
    """Numbers of positional arguments of the signatures in a pybind11 docstring (`self` of
    a method not counted)."""
    sigs = [l for l in fn.__doc__.splitlines()
            if re.match(r"(\d+\. )?%s\(" % re.escape(name), l) and "*args" not in l]
    assert sigs, fn.__doc__
    return sorted(len(re.findall(r"\barg\d+: ", s)) for s in sigs)


def test_tables_agree():
    for op, (groups, _) in OPS.items():
        sizes = [len(g) for g in groups]
        assert HEADS[op] == [sum(sizes[:i + 1]) for i in range(len(sizes))], op


@pytest.mark.parametrize("op", sorted(OPS))
def test_registered_arities(C, op):
    heads = HEADS[op]
    # the whole surface, both forms: the recorder takes H arguments, the immediate op H + 1
    assert _doc_arities(getattr(C.Plan, op), op) == heads
    assert _doc_arities(getattr(C, op), op) == [h + 1 for h in heads]
    bad = OPS[op][1]
    for h in heads:
        _record(C, op, _args(op, h))
        # the immediate form at this arity, stopped by the maker's own check
        if bad and set(bad) <= {k for k, _ in _pairs(op)[:h]}:
            _rejects(C, op, _args(op, h, **bad))
            with pytest.raises(ValueError):
                getattr(C, op)(*_args(op, h, **bad), 0)


@pytest.mark.parametrize("op", sorted(OPS))
def test_unregistered_arities_are_type_errors(C, op):
    heads = HEADS[op]
    full = _args(op)
    filler = [0.5, 1, 0]   # a bare extra scalar or three past the longest arity
    for h in range(heads[0] - 1, heads[-1] + 3):
        if h in heads:
            continue
        args = (full + filler)[:h]
        plan = C.Plan()
        with pytest.raises(TypeError):
            getattr(plan, op)(*args)
        assert plan.size() == 0
        with pytest.raises(TypeError):
            getattr(C, op)(*args, 0)


@pytest.mark.parametrize("op", ["softmax_xent", "head_fused"])
def test_loss_head_defaults(C, op):
    h = HEADS[op]
    for n in h:
        _record(C, op, _args(op, n))
    # label_smoothing, topk(, topk_out) = 0, 0(, null)
    _rejects(C, op, _args(op, h[1], label_smoothing=1.0),
             op + ": label_smoothing in [0, 1), topk >= 0 (> 0 with topk_out)")
    _rejects(C, op, _args(op, h[1], topk=-1))
    _record(C, op, _args(op, h[1], label_smoothing=0.1, topk=5))
    if op == "softmax_xent":
        _rejects(C, op, _args(op, h[1], topk_out=P))
        _record(C, op, _args(op, h[1], topk=5, topk_out=P))
    # labels_b, mix_lam = null, null
    _rejects(C, op, _args(op, h[2], labels_b=P), op + ": labels_b and mix_lam go together")
    _rejects(C, op, _args(op, h[2], mix_lam=P), op + ": labels_b and mix_lam go together")
    _record(C, op, _args(op, h[2], labels_b=P, mix_lam=P))
    # teacher, kd_alpha, kd_inv_tau = null, 0, 1
    kd = op + ": kd_alpha in [0, 1] and kd_inv_tau > 0 with a teacher, kd_alpha 0 without"
    _rejects(C, op, _args(op, h[3], kd_alpha=0.5), kd)
    _rejects(C, op, _args(op, h[3], teacher=P, kd_alpha=0.5, kd_inv_tau=0.0), kd)
    _record(C, op, _args(op, h[3], teacher=P, kd_alpha=0.5))
    _record(C, op, _args(op, h[3], kd_inv_tau=0.0))   # unread without a teacher
    # jsd_B, jsd_weight = 0, 0: N = 6 rows are two triples
    jsd = (op + ": jsd needs N == 3 * jsd_B rows and a finite jsd_weight >= 0 "
           "(jsd_B 0 and jsd_weight 0: off)")
    _rejects(C, op, _args(op, h[4], jsd_B=3, jsd_weight=1.0), jsd)
    _rejects(C, op, _args(op, h[4], jsd_weight=1.0), jsd)
    _record(C, op, _args(op, h[4], jsd_B=2, jsd_weight=1.0))
    _rejects(C, op, _args(op, h[4], jsd_B=2, jsd_weight=1.0, teacher=P),
             op + ": the Jensen-Shannon head takes neither a teacher nor a second (mixup) label")


@pytest.mark.parametrize("op", ["cifar_augment", "cifar_augment_resident", "imagenet_u8_pack"])
def test_input_op_defaults(C, op):
    h = HEADS[op]
    host_fed = op != "cifar_augment_resident"
    for n in h:
        _record(C, op, _args(op, n))
    mix = dict(table=P, table_len=4, labels_b=P, mix_lam=P)
    if host_fed:
        mix["labels"] = P
    _record(C, op, _args(op, h[1], **mix))
    need = (op + ": mixup needs a table of >= 1 entries, " + ("labels, " if host_fed else "") +
            "labels_b and mix_lam")
    _rejects(C, op, _args(op, h[1], table=P), need)                       # table_len 0
    _rejects(C, op, _args(op, h[1], **dict(mix, labels_b=0)), need)
    _rejects(C, op, _args(op, h[1], **dict(mix, mix_lam=0)), need)
    if host_fed:
        _rejects(C, op, _args(op, h[1], **dict(mix, labels=0)), need)
    _rejects(C, op, _args(op, h[1], train=0, **mix), op + ": mixup is a training augmentation")
    # cut_table, cut_thresh, cut_log = null, 0, null
    _rejects(C, op, _args(op, h[2], cut_thresh=100, **mix),
             op + ": cut_thresh > 0 needs a cut_table")
    _rejects(C, op, _args(op, h[2], cut_table=P, cut_thresh=100),
             op + ": cut_thresh > 0 needs the mixup arguments")
    _rejects(C, op, _args(op, h[2], cut_thresh=-1), op + ": cut_thresh must be in [0, 2^24]")
    _record(C, op, _args(op, h[2], cut_table=P, cut_thresh=100, **mix))
    _record(C, op, _args(op, h[2], cut_table=P))    # a table alone is not CutMix


def test_augmix_defaults(C):
    h = HEADS["augmix"]
    for n in h:
        _record(C, "augmix", _args("augmix", n))
    fan = "augmix: the three-view fan-out writes N == 3 * fan_B outputs"
    _rejects(C, "augmix", _args("augmix", fan_B=3), fan)
    _rejects(C, "augmix", _args("augmix", fan_B=-1), fan)
    _record(C, "augmix", _args("augmix", fan_B=2, labels=P))
    _record(C, "augmix", _args("augmix", fan_B=2))


def test_softmax_xent_reduce_default(C):
    _record(C, "softmax_xent_reduce", _args("softmax_xent_reduce", 7))
    _record(C, "softmax_xent_reduce", _args("softmax_xent_reduce", 8))
    _record(C, "softmax_xent_reduce", _args("softmax_xent_reduce", 8, topk_out=P))


SCHEDULE_OPS = sorted(op for op in OPS if OPS[op][0][-1] is DECAY)


def test_schedule_op_list():
    assert len(SCHEDULE_OPS) == 10


@pytest.mark.parametrize("op", SCHEDULE_OPS)
def test_schedule_default_is_piecewise(C, op):
    short, long_ = HEADS[op]
    _record(C, op, _args(op, short))
    _record(C, op, _args(op, long_))                      # ("piecewise", 0, 0, 0) written out
    _record(C, op, _args(op, long_, decay=("cosine", 100, 0.0, 1.0)))
    _record(C, op, _args(op, long_, decay=("poly", 100, 0.001, 2.0)))
    _rejects(C, op, _args(op, long_, decay=("linear", 100, 0.0, 1.0)),
             "lr schedule: decay 'linear' (piecewise, cosine, poly)")
    # a decay schedule checks what the piecewise one does not: the short call is piecewise
    _rejects(C, op, _args(op, long_, decay=("cosine", 0, 0.0, 1.0)),
             "lr schedule: decay_steps > warm_steps >= 0")
    _rejects(C, op, _args(op, long_, decay=("poly", 100, 0.0, 0.0)),
             "lr schedule: power must be positive and finite")
    _rejects(C, op, _args(op, long_, decay=("cosine", 100, -1.0, 1.0)),
             "lr schedule: rates must be finite and >= 0")
    _record(C, op, _args(op, short, warm_steps=-1))       # unchecked by the piecewise schedule
    _rejects(C, op, _args(op, short, vals=[0.1]),
             "lr schedule: <=7 bounds and len(vals)==len(bounds)+1")
    for bare in ("cosine", 0.5):                          # the decay is one tuple
        with pytest.raises(TypeError):
            getattr(C.Plan(), op)(*_args(op, short), bare)


ALIGNED = {
    "adam_update_pack": ("m", "master, grad, m and v"),
    "lion_update_pack": ("m", "master, grad and m"),
    "rmsprop_update_pack": ("ms", "master, grad, ms, mom (and mg)"),
    "muon_update_pack": ("dir", "master, grad, mom and dir"),
    "shampoo_update_pack": ("dir", "master, grad, mom and dir"),
    "lamb_update_pack": ("v", "master, m and v"),
    "lamb_moments_norms": ("grad", "master, grad, m and v"),
}
NULLABLE = {
    "adam_update_pack": "start_step",
    "lion_update_pack": "wd_seg",
    "rmsprop_update_pack": "mom",
    "muon_update_pack": "q_seg",
    "shampoo_update_pack": "graft",
    "lamb_update_pack": "trust",
    "lamb_moments_norms": "blk_seg",
}
COEFS = {
    "adam_update_pack": ("beta1", "beta2"),
    "lion_update_pack": ("beta1", "beta2"),
    "rmsprop_update_pack": ("rho", "momentum"),
    "lamb_update_pack": ("beta1", "beta2"),
    "lamb_moments_norms": ("beta1", "beta2"),
}
DECAY_MODES = {
    "adam_update_pack": "decoupled, l2",
    "rmsprop_update_pack": "l2, decoupled",
    "lamb_update_pack": "decoupled, l2",
    "lamb_moments_norms": "decoupled, l2",
}


@pytest.mark.parametrize("op", sorted(ALIGNED))
def test_flat_update_buffer_checks(C, op):
    arg, names = ALIGNED[op]
    _rejects(C, op, _args(op, **{arg: ODD}), "%s: %s must be 16-byte aligned" % (op, names))
    _rejects(C, op, _args(op, master=ODD), "%s: %s must be 16-byte aligned" % (op, names))
    _rejects(C, op, _args(op, **{NULLABLE[op]: 0}), op + ": null buffer")
    _rejects(C, op, _args(op, master=0), op + ": null buffer")
    _rejects(C, op, _args(op, gstep=0), op + ": null buffer")
    # the first of two failing checks is the one reported
    _rejects(C, op, _args(op, master=ODD, gstep=0),
             "%s: %s must be 16-byte aligned" % (op, names))
    if op == "lamb_moments_norms":
        _rejects(C, op, _args(op, nblocks=-1), "lamb_moments_norms: nblocks >= 0")
        _rejects(C, op, _args(op, gstep=0, nblocks=-1), op + ": null buffer")
    else:
        _rejects(C, op, _args(op, n=-1), op + ": n >= 0 and nseg > 0")
        _rejects(C, op, _args(op, nseg=0), op + ": n >= 0 and nseg > 0")
        _rejects(C, op, _args(op, gstep=0, nseg=0), op + ": null buffer")
        _record(C, op, _args(op, n=0))


def test_rmsprop_mg_only_when_centered(C):
    op = "rmsprop_update_pack"
    _record(C, op, _args(op, mg=ODD))                     # unread: neither null nor alignment
    _rejects(C, op, _args(op, centered=1), op + ": centered needs the mg buffer")
    _rejects(C, op, _args(op, centered=1, mg=ODD),
             op + ": master, grad, ms, mom (and mg) must be 16-byte aligned")
    _record(C, op, _args(op, centered=1, mg=P))
    _rejects(C, op, _args(op, centered=1, nseg=0), op + ": centered needs the mg buffer")


def test_muon_aux_scale(C):
    op = "muon_update_pack"
    _rejects(C, op, _args(op, aux_scale=0.0), op + ": aux_scale > 0")
    _rejects(C, op, _args(op, aux_scale=0.0, nseg=0), op + ": n >= 0 and nseg > 0")


@pytest.mark.parametrize("op", sorted(COEFS))
def test_flat_update_coefficient_checks(C, op):
    a, b = COEFS[op]
    text = "%s: %s and %s in [0, 1)" % (op, a, b)
    for name in (a, b):
        _rejects(C, op, _args(op, **{name: 1.0}), text)
        _rejects(C, op, _args(op, **{name: -0.1}), text)
        _rejects(C, op, _args(op, **{name: float("nan")}), text)
        _record(C, op, _args(op, **{name: 0.0}))
    if op == "lion_update_pack":
        return
    eps = op + ": epsilon must be positive and finite"
    _rejects(C, op, _args(op, epsilon=0.0), eps)
    _rejects(C, op, _args(op, epsilon=float("inf")), eps)
    _rejects(C, op, _args(op, epsilon=float("nan")), eps)
    _rejects(C, op, _args(op, epsilon=0.0, **{a: 1.0}), text)     # coefficients first
    _rejects(C, op, _args(op, decay_mode="L2"),
             "%s: decay mode 'L2' (%s)" % (op, DECAY_MODES[op]))
    _rejects(C, op, _args(op, decay_mode="L2", epsilon=0.0), eps)  # epsilon first
    for mode in ("decoupled", "l2"):
        _record(C, op, _args(op, decay_mode=mode))
    if op != "lamb_moments_norms":
        # the argument checks come before the schedule's
        _rejects(C, op, _args(op, decay_mode="L2", decay=("linear", 0, 0.0, 0.0)),
                 "%s: decay mode 'L2' (%s)" % (op, DECAY_MODES[op]))
