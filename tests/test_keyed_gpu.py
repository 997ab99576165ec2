"""GPU: keyed draws (include/kelpie_hip.h, "Keyed draws") on the device.

  - kp_keyed_draws against the numpy restatement of the definition (keyed_reference.py) on a
    517-entity table: the integer words and the uniform rows bitwise, the normal rows within 1
    float32 ulp.  That bound is derived, not measured: the device and numpy evaluate one
    float64 formula whose results differ by a few float64 ulps, and two such values round to
    float32 values at most one float32 ulp apart.  The count of unequal elements is printed.
  - an armed kp_posttrain_rank (and _topk, _probes, _trace, _marks) against the same batch fed
    with kp_keyed_draws' arrays: every output bitwise equal.
  - the device against the oracle fed the restatement's draws: width_cases' score, rank and
    row rules, unchanged.
  - the engines' order independence, and a rerun on a fresh context, bitwise.
  - the error paths, each with its code and a usable context afterwards.

Run on an MI355X: ``python -m pytest tests -m gpu``."""
import numpy as np
import pytest

import kelpie_amd as ka
import keyed_reference as kr
import width_cases as wc
from keyed_backend import KeyedStandIn
from kelpie_amd import _lib

pytestmark = pytest.mark.gpu

N_ENT, N_REL2 = 517, 80
# the LDS network's edges (one key, one wave, four waves' worth, its last size), the hand-over
# to the global network at 4096 / 4097, one hub-sized slot; padded to 17 slots
RS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 9000, 3, 100, 0, 700, 129)
assert len(RS) == 17


def draw_hp(epochs, batch_size=64):
    hp = _lib.HP()
    hp.epochs, hp.batch_size, hp.neg_ratio = epochs, batch_size, 1
    return hp


def keys_for(n, salt):
    return ([0x0123456789ABCDEF + 977 * salt + i // 2 for i in range(n)],  # pairs of slots share x0
            [0xFEDCBA9876543210 - 31 * salt - i for i in range(n)])


_CTX = {}


def table_ctx(model_name, d):
    """A context over a random 517-entity table of width d (the draws do not read it)."""
    if (model_name, d) not in _CTX:
        g = np.random.default_rng(d)
        E = g.standard_normal((N_ENT, d)).astype(np.float32)
        R = g.standard_normal((N_REL2, d)).astype(np.float32)
        _CTX[model_name, d] = _lib.Context(model_name, E, R)
    return _CTX[model_name, d]


@pytest.mark.parametrize("d", [3, 50, 200, 260])
@pytest.mark.parametrize("model_name", ["TransE", "DistMult"])
def test_keyed_draws_vs_restatement(model_name, d):
    ctx = table_ctx(model_name, d)
    scale = float(np.float32(np.sqrt(2.0 / (d + 1)))) if model_name == "TransE" else 1e-3
    for epochs in (0, 1, 3):
        for rs in ((), RS[:1], RS[11:12], RS):  # 0 slots, 1 slot (R = 0; R = 9000), 17 slots
            row_off = np.concatenate([[0], np.cumsum(rs)]).astype(np.int32)
            ik, sk = keys_for(len(rs), epochs)
            x0, off, rng = ctx.keyed_draws(draw_hp(epochs), row_off, ik, sk, scale, N_ENT + 1)
            rx0, roff, rrng = kr.batch_draws(model_name, d, epochs, 64, row_off, ik, sk, scale, N_ENT + 1)
            assert np.array_equal(off, roff), (epochs, rs)
            words = _lib.keyed_rng_words(model_name, draw_hp(epochs), row_off)
            assert np.array_equal(np.diff(off), words)
            assert np.array_equal(rng, rrng), (epochs, rs, int((rng != rrng).sum()))
            if model_name == "TransE":
                dist = kr.ulp_distance(x0, rx0)
                print(f"TransE d={d} epochs={epochs} slots={len(rs)}: {int((dist > 0).sum())} of {dist.size} "
                      f"normal elements differ, max {int(dist.max()) if dist.size else 0} ulp")
                assert dist.size == 0 or dist.max() <= 1
            else:
                assert np.array_equal(x0.view(np.int32), rx0.view(np.int32))
    # a rerun gives the same bits
    row_off = np.concatenate([[0], np.cumsum(RS)]).astype(np.int32)
    ik, sk = keys_for(len(RS), 9)
    a = ctx.keyed_draws(draw_hp(2), row_off, ik, sk, scale, N_ENT + 1)
    b = ctx.keyed_draws(draw_hp(2), row_off, ik, sk, scale, N_ENT + 1)
    assert all(np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u, v.view(np.int32)
                              if v.dtype == np.float32 else v) for u, v in zip(a, b))


# ----------------------------------------------------------------------------- armed == fed
def same(a, b, path="out"):
    """Bitwise equality of two posttrain_rank results (nested tuples / lists of arrays)."""
    if a is None or b is None:
        assert a is None and b is None, path
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            same(u, v, f"{path}[{i}]")
    else:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, path
        assert a.tobytes() == b.tobytes(), (path, int((a != b).sum()))


class ArmedVsFed:
    """In front of a device context: every armed call also runs unarmed, fed with
    kp_keyed_draws' arrays of the same keys, and the two results must be bitwise equal."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.keys = None
        self.compared = 0
        self.words = 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def arm_keyed(self, *a):
        self.keys = a
        self._ctx.arm_keyed(*a)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, **kw):
        assert x0 is None and rng_off is None and rng is None and self.keys is not None
        armed = self._ctx.posttrain_rank(hp, None, row_off, rows, None, None, pred, filt_off, filt, want_x=True, **kw)
        fx0, foff, frng = self._ctx.keyed_draws(hp, row_off, *self.keys)
        if frng.size == 0:
            frng = np.zeros(1, np.int32)
        fed = self._ctx.posttrain_rank(hp, fx0, row_off, rows, foff, frng, pred, filt_off, filt, want_x=True, **kw)
        same(armed, fed)
        self.compared += 1
        self.words += int(foff[-1])
        self.keys = None
        return armed if want_x else armed[:2] + (None,) + armed[3:]


ARMED = [
    pytest.param(wc._case("ComplEx", 32, seed=4), False, id="ComplEx-row64"),
    pytest.param(wc._case("ComplEx", 32, seed=4), True, id="ComplEx-row64-hub"),
    pytest.param(wc._case("DistMult", 24, seed=4), False, id="DistMult-d24"),
    pytest.param(wc._case("TransE", 50, seed=4), False, id="TransE-d50-L2"),
    pytest.param(wc._case("TransE", 260, norm=1), False, id="TransE-d260-L1"),
]


def keyed_engine(case, ctx_of, hub=False, seed=5, cls=ka.NecessaryPostTrainingEngine):
    _, ds, ordinary, hub_pred = wc.graph(case["n_ent"])
    model = wc.make_model(case)
    model._ctx = ctx_of(model)
    eng = cls(model, ds, dict(wc.hp_of(case), epochs=wc.HUB_EPOCHS if hub else 8))
    eng.draws, eng.seed = "keyed", seed
    pred = hub_pred if hub else ordinary[0]
    cands = sorted(ds.entity_to_training_triples[pred[0]])
    return eng, ds, pred, cands


@pytest.mark.parametrize("case,hub", ARMED)
def test_armed_call_equals_fed_call(case, hub):
    eng, ds, pred, cands = keyed_engine(case, lambda m: ArmedVsFed(m.ctx), hub)
    rules = [[cands[0]]] if hub else [[cands[0]], [cands[1], cands[2]]]
    eng.compute_relevance_batch(pred, rules)
    ctx = eng.model.ctx
    assert ctx.compared == 1
    if hub and case["model"] != "TransE":
        assert wc.hub_rows(case) > 512 and ctx.words > 0  # a multi-step slot: its permutations were generated
    elif case["model"] != "TransE":
        assert ctx.words == 0
    # once each with the lists, the probes, the trace and the marks
    for attr, value in (("top_k", 3), ("side_effects", 4), ("trace", True), ("marks", [0, 1, 3])):
        eng, ds, pred, cands = keyed_engine(case, lambda m: ArmedVsFed(m.ctx), hub)
        setattr(eng, attr, value)
        eng.compute_relevance_batch(pred, rules[:1])
        assert eng.model.ctx.compared == 1, attr


# ----------------------------------------------------------------------------- device against oracle
ORACLE = [wc._case("ComplEx", 32, seed=4), wc._case("DistMult", 40, seed=4), wc._case("TransE", 50, seed=4),
          wc._case("TransE", 260, tag="hub", hub=True, seed=4)]


def run_keyed(case, ctx_of):
    """width_cases.run_necessary in keyed mode: two subjects with two singleton candidates
    each (or the hub subject with one), 8 epochs (the hub: 3)."""
    ds = wc.graph(case["n_ent"])[1]
    model = wc.make_model(case)
    model._ctx = ctx_of(model)
    for pred, epochs, n in wc.subjects(case):
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(wc.hp_of(case), epochs=epochs))
        eng.draws, eng.seed = "keyed", 3
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        eng.compute_relevance_batch(pred, [[c] for c in cands])
    return model.ctx.slots


@pytest.mark.parametrize("case", ORACLE, ids=wc.ids(ORACLE))
def test_device_vs_oracle_on_keyed_draws(case):
    ref = run_keyed(case, lambda m: KeyedStandIn(wc.oracle_context(m), m))
    got = run_keyed(case, wc.device_context)
    exact, row_err = wc.check_slots(got, ref, rows=case["model"] in ("ComplEx", "DistMult"))
    print(f"{case['id']}: exact ranks {exact}/{len(got)}, row error {row_err:.2e} of the row's scale")


# ----------------------------------------------------------------------------- the engines
@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
@pytest.mark.parametrize("case", [wc._case("ComplEx", 32, seed=4), wc._case("TransE", 50, seed=4)],
                         ids=["ComplEx", "TransE"])
def test_engine_order_independence_on_the_device(case, mode):
    cls = ka.NecessaryPostTrainingEngine if mode == "necessary" else ka.SufficientPostTrainingEngine
    _, ds, ordinary, _ = wc.graph(case["n_ent"])
    p1, p2 = ordinary[:2]
    a, b, c = sorted(ds.entity_to_training_triples[p1[0]])[:3]
    rules = [[a], [b, c], [c]]
    ents = [e for e in range(40, 60) if e not in (p1[0], p2[0]) and 4 <= ds.entity_to_degree.get(e, 0) <= 40][:2]
    other = [[sorted(ds.entity_to_training_triples[p2[0]])[0]]]

    def fresh():
        eng = keyed_engine(case, lambda m: m.ctx, cls=cls)[0]
        if mode == "sufficient":
            eng.entities_to_convert = list(ents)
        return eng

    together = fresh().compute_relevance_batch(p1, rules)
    alone = [fresh().compute_relevance_batch(p1, [r])[0] for r in reversed(rules)]
    assert alone[::-1] == together
    assert fresh().compute_relevance_batch(p1, rules) == together  # a rerun on a fresh context
    items = [(p2, other), (p1, rules)] if mode == "necessary" else [(p2, other, ents), (p1, rules, ents)]
    assert fresh().compute_relevance_multi(items)[1] == together
    eng = fresh()
    eng.seed = 6
    assert eng.compute_relevance_batch(p1, rules) != together


@pytest.mark.parametrize("case", [wc._case("ComplEx", 32, seed=4), wc._case("TransE", 50, seed=4)],
                         ids=["ComplEx", "TransE"])
def test_extras_order_independence_on_the_device(case):
    """compute_counterfactuals, compute_side_effects, compute_traces and compute_curves in keyed
    mode: the report of each rule is the same in one batch and alone on a fresh engine (the
    base results included: they are a function of the seed and the prediction)."""
    _, ds, ordinary, _ = wc.graph(case["n_ent"])
    p1 = ordinary[0]
    a, b = sorted(ds.entity_to_training_triples[p1[0]])[:2]
    rules = [[a], [b]]
    calls = (("compute_counterfactuals", (3,)), ("compute_side_effects", ()), ("compute_traces", ()),
             ("compute_curves", ([0, 2, 8],)))
    for name, extra in calls:
        together = getattr(keyed_engine(case, lambda m: m.ctx)[0], name)(p1, rules, *extra)
        for i in (1, 0):
            alone = getattr(keyed_engine(case, lambda m: m.ctx)[0], name)(p1, [rules[i]], *extra)
            assert alone[0] == together[i], (name, i)
        assert together[0]["base"] == together[1]["base"], name


# ----------------------------------------------------------------------------- error paths
def packed_batch(case):
    """A keyed engine's packed batch of one subject, the keys, and the engine."""
    eng, ds, pred, cands = keyed_engine(case, lambda m: m.ctx)
    eng._deferred_error = None
    slots, _, _ = eng._schedule_all(eng._batch_items(pred, [[cands[0]], [cands[1]]]), None)
    return eng, slots, eng._pack(slots)


def usable(ctx):
    s = ctx.all_scores(np.array([1, 2]), np.array([0, 3]))
    assert s.shape == (2, N_ENT) and np.isfinite(s).all()


@pytest.mark.parametrize("case", [wc._case("ComplEx", 32, seed=4), wc._case("TransE", 50, seed=4)],
                         ids=["ComplEx", "TransE"])
def test_error_paths(case):
    eng, slots, packed = packed_batch(case)
    ctx, hp = eng.model.ctx, eng._kp_hp
    scale, bound = eng.model.keyed_params()
    ik, sk = [s.keys[0] for s in slots], [s.keys[1] for s in slots]
    assert len(slots) == 3
    # NULL buffers, unarmed: the error it always was
    with pytest.raises(_lib.KelpieHipError, match="error -22.*missing buffer"):
        ctx.posttrain_rank(hp, *packed)
    usable(ctx)
    # armed with another n_slots
    ctx.arm_keyed(ik[:2], sk[:2], scale, bound)
    with pytest.raises(_lib.KelpieHipError, match="error -22.*n_slots differs"):
        ctx.posttrain_rank(hp, *packed)
    usable(ctx)
    with pytest.raises(_lib.KelpieHipError, match="error -22.*missing buffer"):  # the error disarmed
        ctx.posttrain_rank(hp, *packed)
    # armed, then the fp64 entry point: refused, disarmed
    ctx.arm_keyed(ik, sk, scale, bound)
    with pytest.raises(_lib.KelpieHipError, match="error -95"):
        ctx.posttrain_rank_f64(_lib.HP64(hp, 0.01, 0.9, 0.999, 1e-8, 0.0), np.zeros((3, ctx.dim)), packed[1], packed[2],
                               np.zeros(4, np.int64), np.zeros(1, np.int32), *packed[5:])
    usable(ctx)
    with pytest.raises(_lib.KelpieHipError, match="error -22.*missing buffer"):
        ctx.posttrain_rank(hp, *packed)
    if case["model"] == "TransE":
        ctx.arm_keyed(ik, sk, scale, 0)
        with pytest.raises(_lib.KelpieHipError, match="error -22.*neg_bound"):
            ctx.posttrain_rank(hp, *packed)
        usable(ctx)
    # and a good armed call afterwards
    ctx.arm_keyed(ik, sk, scale, bound)
    s, r, _ = ctx.posttrain_rank(hp, *packed)
    assert np.isfinite(s).all() and (r >= 0).all()


def test_arming_a_conve_context_is_refused():
    model = wc.make_model(wc._case("ConvE", 100))
    with pytest.raises(_lib.KelpieHipError, match="error -95"):
        model.ctx.arm_keyed([1], [2], 1.0, 0)
    usable(model.ctx)
    with pytest.raises(_lib.KelpieHipError, match="error -95"):
        _lib.keyed_rng_words("ConvE", draw_hp(1), np.array([0, 4]))
