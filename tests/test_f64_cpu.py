"""CPU: the fp64 definition (include/kelpie_hip.h, "fp64") on the host side.

1. The numpy float64 restatement (f64_reference.py) equals the reference's own fp64 runs:
   every post-training of tests/golden/complex200_reg_fullwidth.json (none / N3 / N2, the N3
   element whose fp32 run is 1.5e-3 off included) and the fp64 runs of
   tests/golden/distmult_tiny.json -- ranks exact on every element, scores (and rows where
   recorded) within TOL_F64.  The distance itself is printed: MEASURED_F64 (f64_reference.py) is
   what this test measured where the tolerance was derived; numpy's matrix products sum in an
   order that depends on the BLAS build and its threads, and the N3 element amplifies that
   rounding noise several hundred times, so another machine measures another 1e-13.
2. TOL_F64 = 8 x MEASURED_F64 is far below fp32 resolution, and the derived rank bound at
   TOL_F64 is a single rank for every slot of every device case (f64_cases.py).
3. The host protocol on the stand-in: the generators end where the fp32 calls leave them, x0
   is the float64 product, a logging context sees only the new call in fp64 and only the old
   calls, with byte-identical arguments, in fp32; every refusal raises before any draw.
"""
import numpy as np
import pytest
import torch

import distmult_backend as dmb
import f64_cases as fc
import f64_reference as fr
import kelpie_amd as ka
import test_reg_fullwidth as reg_fw
import width_cases as wc
from cpu_backend import OracleBackedContext
from f64_backend import CallLog, F64Context
from golden_io import seed_all


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


# ----------------------------------------------------------------------------- 1. the goldens
@pytest.mark.slow
@pytest.mark.parametrize("reg", reg_fw.REGS)
def test_restatement_equals_reference_fp64_fullwidth(reg):
    rec, ds, w = reg_fw._case()
    hp = dict(rec["hp"]) if reg == "none" else dict(rec["hp"], regularizer_name=reg, regularizer_weight=0.05)
    model = ka.ComplEx(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=rec["init_scale"])
    model._ctx = F64Context(model)
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    eng.precision = "fp64"
    got = []
    for pred, cands in zip(rec["preds"], rec["candidates"]):
        eng.set_cache()
        eng.compute_relevance_batch(tuple(pred), [[tuple(c)] for c in cands])
        got += [(pt["target_rank"], pt["target_score"], b["target_rank"], b["target_score"])
                for pt, b in eng.last_results]
    r64 = reg_fw._ref(rec, reg, "fp64")
    assert len(got) == len(r64) == 12
    worst = max(max(_rel(g[1], b[1]), _rel(g[3], b[3])) for g, b in zip(got, r64))
    print(f"{reg}: largest relative score distance to the reference's fp64 run {worst:.3e}")
    for g, b in zip(got, r64):
        assert g[0] == b[0] and g[2] == b[2], (reg, g, b)  # ranks exact, a condition
    assert worst <= fr.TOL_F64, worst
    if reg == "N3":  # the flagged element is among them: the fp32 run is > 1e-4 off there
        assert reg_fw.ill_conditioned(rec, reg)
    # the derived bound decides every one of these slots
    assert all(s["lo"] == s["hi"] == s["rank"] for s in model.ctx.slots)


def test_restatement_equals_reference_fp64_distmult():
    rec, ds, model = dmb.load_fixture()
    x0 = model.kelpie_init64(np.asarray(rec["init"], np.float32), None)
    assert x0.dtype == np.float64
    trip = np.asarray(rec["kelpie_training_triples"], np.int64)
    rows = np.vstack([trip, ds.invert_triples(trip)])
    ctx = F64Context(model)
    worst_s = worst_x = 0.0
    for slot in rec["slots"]:
        perms = np.asarray(slot["perms"], np.int32).reshape(-1) if slot["perms"] else np.zeros(0, np.int32)
        filt = np.asarray(slot["filter"], np.int64)
        sc, rk, x = ctx.posttrain_rank_f64(model.kp_hp64(slot["hp"]), x0[None], np.array([0, len(rows)]), rows,
                                           np.array([0, len(perms)]), perms, np.array([slot["kelpie_triple"]]),
                                           np.array([0, len(filt)]), filt, want_x=True)
        f64 = slot["fp64"]
        assert int(rk[0]) == f64["rank"], (slot["name"], int(rk[0]), f64["rank"])
        row = np.asarray(f64["row"])
        worst_s = max(worst_s, _rel(float(sc[0]), f64["score"]))
        worst_x = max(worst_x, float(np.abs(x[0] - row).max() / np.abs(row).max()))
        # the restatement's score row is the reference's (the fixture keeps nine digits of it)
        assert np.abs(ctx.slots[-1]["row"] - np.asarray(f64["scores"])).max() <= 1e-9
    print(f"distmult: largest relative score distance {worst_s:.3e}, row distance {worst_x:.3e}")
    assert worst_s <= fr.TOL_F64 and worst_x <= fr.TOL_F64


# ----------------------------------------------------------------------------- 2. the tolerance
def test_tolerance_is_far_below_fp32_resolution():
    assert fr.TOL_F64 == 8 * fr.MEASURED_F64
    assert fr.TOL_F64 < 2.0 ** -24 * 1e-3  # a thousandth of half an fp32 ulp of 1


@pytest.mark.parametrize("case", fc.ALL, ids=wc.ids(fc.ALL))
def test_rank_bound_is_a_single_rank(case):
    ref = fc.reference(case)
    assert len(ref) > 0
    for i, s in enumerate(ref):
        assert s["lo"] == s["hi"] == s["rank"], (i, s["lo"], s["hi"], s["rank"])
    if case in fc.HUB:  # several minibatches per epoch
        assert min(s["n_rows"] for s in ref) > case["batch_size"]
    if case in fc.CRAFTED:
        assert ref[1]["n_rows"] == 0


# ----------------------------------------------------------------------------- 3. host protocol
CASE = wc._case("ComplEx", 8, seed=4)


def _states():
    return torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2]


def _engine(ctx_of, precision=None, cls=ka.NecessaryPostTrainingEngine, case=CASE):
    ds = wc.graph(case["n_ent"])[1]
    model = wc.make_model(case)
    model._ctx = ctx_of(model)
    eng = cls(model, ds, wc.hp_of(case))
    if precision is not None:
        eng.precision = precision
    return eng, ds, model


def _calls(eng, ds):
    out = []
    for pred, _, n in wc.subjects(CASE):
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        out.append(eng.compute_relevance_batch(pred, [[c] for c in cands]))
        out.append([eng.compute_relevance(pred, [cands[0]])])  # the cached base
    return out


def test_generators_end_in_the_same_state():
    seed_all(42)
    eng, ds, _ = _engine(OracleBackedContext)
    _calls(eng, ds)
    s32 = _states()
    seed_all(42)
    eng, ds, model = _engine(lambda m: CallLog(F64Context(m)), "fp64")
    rels = _calls(eng, ds)
    assert _states() == s32
    # only the new call, with a float64 x0 that is the float64 product
    assert {c[0] for c in model.ctx.log} == {"posttrain_rank_f64"}
    assert all(c[1][1][0] == "float64" for c in model.ctx.log)
    assert all(isinstance(r, float) for b in rels for r in b)
    pt, base = eng.last_results[0]
    assert isinstance(pt["target_score"], float)
    # the relevance in float64: no float32 add
    want = float(pt["target_rank"] - base["target_rank"]) + 1 / (1 + np.exp(-(base["target_score"]
                                                                                 - pt["target_score"])))
    assert rels[-1][0] == pytest.approx(want, abs=1e-15) and rels[-1][0] != float(np.float32(rels[-1][0]))


def test_x0_is_the_float64_product():
    model = wc.make_model(CASE)
    init = np.random.default_rng(0).random(model.dimension).astype(np.float32)
    x = model.kelpie_init64(init, None)
    assert x.dtype == np.float64
    assert np.array_equal(x, init.astype(np.float64) * model.init_scale)
    assert not np.array_equal(x, model.kelpie_init(init, None).astype(np.float64))
    hp64 = model.kp_hp64(dict(wc.hp_of(CASE), lr=0.01))
    assert hp64.lr == 0.01 and hp64.hp.lr == np.float32(0.01) and hp64.eps == 1e-10


def test_default_precision_makes_the_old_calls_with_identical_bytes():
    """An engine whose precision was never touched, and one that served fp64 calls in between
    and went back to "fp32": both see only posttrain_rank, with byte-identical arguments (the
    base cache is keyed by precision, so the fp64 calls leave the fp32 ones as they were)."""
    seed_all(42)
    eng, ds, model = _engine(lambda m: CallLog(OracleBackedContext(m)))
    rels = _calls(eng, ds)
    plain = model.ctx.log
    assert {c[0] for c in plain} == {"posttrain_rank"}

    class Both(OracleBackedContext):
        def posttrain_rank_f64(self, *a, **k):
            return F64Context(self.model).posttrain_rank_f64(*a, **k)

    seed_all(42)
    eng, ds, model = _engine(lambda m: CallLog(Both(m)))
    eng.precision = "fp64"
    state = _states()
    pred, _, n = wc.subjects(CASE)[0]
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
    eng.compute_relevance_batch(pred, [[c] for c in cands])
    seed_all(42)  # the fp64 calls advanced the generators as fp32 calls would: start over
    assert state == _states()
    eng.precision = "fp32"
    rels2 = _calls(eng, ds)
    mixed = [c for c in model.ctx.log if c[0] == "posttrain_rank"]
    assert mixed == plain and rels2 == rels
    assert any(c[0] == "posttrain_rank_f64" for c in model.ctx.log)


class _NoCalls:
    def __init__(self, model):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"a refused call reached the context ({name})")


@pytest.mark.parametrize("what", ["top_k", "probes", "trace", "marks", "sharding", "pipeline"])
def test_fp64_refusals_raise_before_any_draw(what):
    seed_all(42)
    eng, ds, model = _engine(_NoCalls, "fp64")
    pred, _, n = wc.subjects(CASE)[0]
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
    rules = [[c] for c in cands]
    if what == "top_k":
        eng.top_k = 3
    elif what == "probes":
        eng.side_effects = 2
    elif what == "trace":
        eng.trace = True
    elif what == "marks":
        eng.marks = [0, 2]
    elif what == "sharding":
        from kelpie_amd.distributed import SlotSharding
        eng.sharding = SlotSharding(rank=0, world=2)
    before = _states()
    with pytest.raises(NotImplementedError, match="fp64"):
        if what == "pipeline":
            eng.compute_relevance_pipeline([[(pred, rules)]])
        else:
            eng.compute_relevance_batch(pred, rules)
    assert _states() == before
    if what != "pipeline":
        with pytest.raises(NotImplementedError, match="fp64"):
            eng.compute_relevance_multi([(pred, rules)])
        with pytest.raises(NotImplementedError, match="fp64"):
            eng.compute_relevance(pred, rules[0])
        assert _states() == before


def test_fp64_refusals_sufficient_engine():
    seed_all(42)
    eng, ds, model = _engine(_NoCalls, "fp64", cls=ka.SufficientPostTrainingEngine)
    pred, _, n = wc.subjects(CASE)[0]
    eng.entities_to_convert = [3, 4]
    eng.top_k = 2
    before = _states()
    with pytest.raises(NotImplementedError, match="fp64"):
        eng.compute_relevance_batch(pred, [[sorted(ds.entity_to_training_triples[pred[0]])[0]]])
    assert _states() == before


@pytest.mark.parametrize("case", [wc._case("TransE", 50, seed=4), wc._case("ConvE", 100)], ids=["TransE", "ConvE"])
def test_other_families_refuse_the_precision(case):
    eng, _, _ = _engine(_NoCalls, case=case)
    assert eng.precision == "fp32"
    with pytest.raises(NotImplementedError, match="fp64"):
        eng.precision = "fp64"
    assert eng.precision == "fp32"
    with pytest.raises(ValueError):
        eng.precision = "fp16"


def test_sufficient_engine_in_fp64_on_the_standin():
    seed_all(42)
    eng, ds, model = _engine(lambda m: CallLog(F64Context(m)), "fp64", cls=ka.SufficientPostTrainingEngine)
    pred, _, n = wc.subjects(CASE)[0]
    eng.entities_to_convert = [e for e in range(ds.num_entities) if ds.entity_to_degree.get(e, 0) >= 8
                               and e != pred[0]][:2]
    cand = sorted(ds.entity_to_training_triples[pred[0]])[0]
    rel = eng.compute_relevance_batch(pred, [[cand]])
    assert {c[0] for c in model.ctx.log} == {"posttrain_rank_f64"}
    det = eng.last_results[0]
    want = [(float(b["target_rank"] - pt["target_rank"]) + 1 / (1 + np.exp(-(pt["target_score"] - b["target_score"]))))
            / float(b["target_rank"]) for pt, b in det]
    assert rel[0] == pytest.approx(sum(want) / len(want), abs=1e-14)
