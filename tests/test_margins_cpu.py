"""Rank margins, CPU tier: ``compute_margins``, ``engine.margin_tol``, the builder's and the
pipeline's ``margins=`` over the oracle-backed stand-ins wrapped to answer margins by the
definition (margins_backend.py on margins_reference.py), for all four families, necessary and
sufficient.  The device side is test_margins_gpu.py, the host check test_margins_check.py.

The last tests state conditions on the inputs the device tests share (margins_cases.py), so
that those can decide: on the 517-entity graph at tol = 1e-4 every family has a rank row with a
band and one without, and no compared column lies within the summation bound of a threshold.
"""
import inspect
import math
import random

import numpy as np
import pytest
import torch

import kelpie_amd as ka
import margins_cases as gc
import margins_reference as mr
import width_cases as wc
from keyed_backend import KeyedStandIn
from kelpie_amd import _lib
from kelpie_amd.pipeline import build_pipeline, run_explain
from margins_backend import MarginsStandIn
from marks_backend import MarksContext

EPOCHS = 3  # the host layers and the definition do not depend on the epoch count
MODES = ("necessary", "sufficient")
SIDE_KEYS = {"score", "rank", "rank_lo", "rank_hi", "ties", "gap_better", "gap_worse", "id_better", "id_worse"}


def _state():
    return (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
            random.getstate())


def standin(model):
    return MarginsStandIn(wc.oracle_context(model))


@pytest.fixture(scope="module")
def runs():
    """Every (case, mode, tol) run once: (batches, model, reports)."""
    cache = {}

    def get(case, mode, tol):
        key = (case["id"], mode, tol)
        if key not in cache:
            cache[key] = gc.run(case, standin, tol=tol, mode=mode, epochs=EPOCHS)
        return cache[key]

    return get


def _sides(reports, mode):
    for rep in reports:
        for o in rep:
            if mode == "necessary":
                yield o["base"], o["post"]
            else:
                for c in o["conversions"]:
                    yield c["base"], c["post"]


# ----------------------------------------------------------------------------- the band
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", gc.FAMILY, ids=gc.ids(gc.FAMILY))
def test_tol_zero_is_the_rank_and_bands_nest(case, mode, runs):
    per_tol = [list(_sides(runs(case, mode, t)[2], mode)) for t in gc.TOLS]
    assert len(per_tol[0]) > 0
    for sides in zip(*per_tol):  # the same post-training pair under the four tolerances
        for which in (0, 1):
            s = [pair[which] for pair in sides]
            assert set(s[0]) == SIDE_KEYS
            assert s[0]["rank_lo"] == s[0]["rank"] == s[0]["rank_hi"]
            for a, b in zip(s, s[1:]):
                assert b["rank_lo"] <= a["rank_lo"] <= a["rank"] <= a["rank_hi"] <= b["rank_hi"]
                # the post-training, the ties and the nearest competitors do not depend on tol
                for k in SIDE_KEYS - {"rank_lo", "rank_hi"}:
                    assert a[k] == b[k], k
            assert s[0]["gap_better"] >= 0 and s[0]["gap_worse"] >= 0
            assert (s[0]["id_better"] == -1) == math.isinf(s[0]["gap_better"])


@pytest.mark.parametrize("case", gc.FAMILY, ids=gc.ids(gc.FAMILY))
def test_tol_one(case, runs):
    """At tol = 1 delta is at least 1: a row none of whose other columns is that much better has
    rank_lo == own, a row all of whose other columns are within delta has rank_hi == the
    unmasked column count; the small scores of ComplEx and DistMult meet both."""
    batches, model, _ = runs(case, "necessary", 1.0)
    mode = gc.mode_of(model)
    lo_hit = hi_hit = rows = 0
    for b in batches:
        slots = gc.margin_rows(b["out"][-1][0])
        for got, (kind, c, masked, o, sat, _, _) in zip(slots, _rows_of(model, b)):
            v = mr.units(mode, c)
            delta = max(1.0, abs(v[o]))
            keep = mr.others(masked, o)
            own = mr.own_count(mode, masked, o)
            sign = -1.0 if mode in mr.MINIMIZERS else 1.0
            ahead = sign * (v[keep] - v[o])  # how much better every other column is, in score units
            rows += 1
            if not (ahead >= delta * (1 - 1e-12)).any() and not (sat is not None and sat[o]):
                assert got["rank_lo"] == own
                lo_hit += 1
            if (ahead >= -delta * (1 - 1e-12)).all():
                assert got["rank_hi"] == own + int(keep.sum())
                hi_hit += 1
    assert rows > 0
    if case["model"] in ("ComplEx", "DistMult"):
        assert lo_hit == rows and hi_hit == rows


def _rows_of(model, batch):
    """The stand-in's logged slot rows of a captured batch (Capture keeps the batches in call
    order, MarginsStandIn its rows)."""
    cap = model.ctx
    return [r for r in cap._ctx.rows[cap.batches.index(batch)] if r[0] == "slot"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", gc.FAMILY, ids=gc.ids(gc.FAMILY))
def test_relevance_is_compute_relevance_batchs(case, mode, runs):
    _, _, reports = runs(case, mode, gc.TOL)
    ds, ordinary = wc.graph(case["n_ent"])[1:3]
    model = wc.make_model(case)
    model._ctx = wc.oracle_context(model)  # no margins stand-in at all: the plain call
    gc.seed_all(42)
    for rep, (pred, _, n) in zip(reports, wc.subjects(case)):
        hp = dict(wc.hp_of(case), epochs=EPOCHS)
        if mode == "necessary":
            eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
        else:
            eng = ka.SufficientPostTrainingEngine(model, ds, hp)
            eng.entities_to_convert = [int(p[0]) for p in ordinary if p[0] != pred[0]][:2]
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        plain = eng.compute_relevance_batch(pred, [[c] for c in cands])
        assert [o["relevance"] for o in rep] == plain  # the same floats
        for o in rep:
            assert o["relevance_lo"] <= o["relevance_hi"]
            # the float32 relevance lies in the float64 band up to its own rounding
            slack = 2.0 ** -23 * max(1.0, abs(o["relevance"]))
            assert o["relevance_lo"] - slack <= o["relevance"] <= o["relevance_hi"] + slack


def _engine(case, mode):
    ds = wc.graph(case["n_ent"])[1]
    model = wc.make_model(case)
    model._ctx = standin(model)
    cls = ka.NecessaryPostTrainingEngine if mode == "necessary" else ka.SufficientPostTrainingEngine
    return cls(model, ds, dict(wc.hp_of(case), epochs=EPOCHS)), ds


def test_band_arithmetic_by_hand():
    sig = lambda d: 1.0 / (1.0 + math.exp(-d))  # noqa: E731
    base = {"score": 0.25, "rank": 10, "rank_lo": 9, "rank_hi": 12}
    post = {"score": 0.75, "rank": 15, "rank_lo": 14, "rank_hi": 15}
    # necessary, maximizer: (post.rank - base.rank) + sigmoid(base.score - post.score)
    nec, _ = _engine(gc.FAMILY[0], "necessary")
    lo, hi = nec._band_of(base, post)
    assert lo == (14 - 12) + sig(-0.5) and hi == (15 - 9) + sig(-0.5)
    # necessary, minimizer: the score worsens upwards
    nec_te, _ = _engine(gc.FAMILY[3], "necessary")
    lo, hi = nec_te._band_of(base, post)
    assert lo == 2 + sig(0.5) and hi == 6 + sig(0.5)
    # sufficient, maximizer: ((base.rank - post.rank) + sigmoid(post.score - base.score)) / base.rank
    # over the corners (9, 14), (9, 15), (12, 14), (12, 15)
    suf, _ = _engine(gc.FAMILY[0], "sufficient")
    corners = [((b - p) + sig(0.5)) / b for b in (9, 12) for p in (14, 15)]
    lo, hi = suf._band_of(base, post)
    assert lo == min(corners) == ((9 - 15) + sig(0.5)) / 9 and hi == max(corners) == ((12 - 14) + sig(0.5)) / 12
    # the means of the lows and of the highs over the conversion entities
    suf.entities_to_convert = [3, 4]
    narrow = {"score": 0.5, "rank": 7, "rank_lo": 7, "rank_hi": 7}
    det = [({"target_score": s["score"], "target_rank": s["rank"], "margins": dict(s, tol=0.5)},
            {"target_score": b["score"], "target_rank": b["rank"], "margins": dict(b, tol=0.5)})
           for s, b in ((post, base), (narrow, narrow))]
    for pt, b in det:
        for m in (pt["margins"], b["margins"]):
            m.update(ties=0, gap_better=1.0, gap_worse=1.0, id_better=1, id_worse=2)
    out = suf._mg_rule(0.125, det, 0.5)
    flat = ((7 - 7) + sig(0.0)) / 7
    assert out["relevance"] == 0.125 and [c["entity"] for c in out["conversions"]] == [3, 4]
    assert out["relevance_lo"] == (min(corners) + flat) / 2 and out["relevance_hi"] == (max(corners) + flat) / 2
    # margins of another tolerance are no margins of this one
    out = suf._mg_rule(0.125, det, 0.25)
    assert out["relevance_lo"] is None and out["conversions"][0]["base"]["rank_lo"] is None
    assert out["conversions"][0]["base"]["rank"] == 10


def test_cached_base_without_margins_gives_none():
    eng, ds = _engine(gc.FAMILY[0], "necessary")
    pred = wc.graph(517)[2][0]
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:2]
    gc.seed_all(42)
    eng.compute_relevance_batch(pred, [[cands[0]]])  # caches the base result, no margins
    out = eng.compute_margins(pred, [[cands[1]]], tol=gc.TOL)[0]
    assert out["base"]["rank_lo"] is None and out["base"]["rank"] > 0 and out["post"]["rank_lo"] is not None
    assert out["relevance_lo"] is None and out["relevance_hi"] is None
    assert eng.margin_tol is None and eng.model.ctx.margin_calls == [None, gc.TOL]


# ----------------------------------------------------------------------------- requests and refusals
def test_tolerance_is_validated():
    eng, ds = _engine(gc.FAMILY[0], "necessary")
    pred = wc.graph(517)[2][0]
    before = _state()
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            eng.compute_margins(pred, [[(1, 2, 3)]], tol=bad)
        with pytest.raises(ValueError, match="tol"):
            eng.margin_tol = bad
    for bad in ("1e-4", None, True, [1e-4]):
        with pytest.raises(TypeError, match="tol"):
            eng.compute_margins(pred, [[(1, 2, 3)]], tol=bad)
    with pytest.raises(ValueError, match="tol"):
        ka.StochasticBuilder(5, eng, margins=2.0)
    assert _state() == before and eng.model.ctx.margin_calls == [] and eng.margin_tol is None
    eng.margin_tol = 0
    assert eng.margin_tol == 0.0
    eng.margin_tol = None
    for f in (ka.StochasticBuilder.__init__, build_pipeline, run_explain):
        assert inspect.signature(f).parameters["margins"].default is None
    assert inspect.signature(_lib.Context.posttrain_rank).parameters["margins"].default is None
    assert inspect.signature(type(eng).compute_margins).parameters["tol"].default == 1e-4


@pytest.mark.parametrize("what", ["fp64", "sharding", "pipeline", "submit_batch", "pipelined builder"])
def test_refusals_leave_the_generators_alone(what):
    eng, ds = _engine(gc.FAMILY[0], "necessary")
    pred = wc.graph(517)[2][0]
    rules = [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]
    gc.seed_all(42)

    class Sharding:
        world, rank = 2, 0

        def __getattr__(self, name):
            raise AssertionError(f"sharding used: {name}")

    if what == "fp64":
        eng.precision = "fp64"
    elif what == "sharding":
        eng.sharding = Sharding()
    before = _state()
    with pytest.raises(NotImplementedError, match="margins"):
        if what == "pipeline":
            eng.margin_tol = gc.TOL
            eng.compute_relevance_pipeline([[(pred, rules)]])
        elif what == "submit_batch":
            eng.margin_tol = gc.TOL
            eng.submit_batch(pred, rules)
        elif what == "pipelined builder":
            ka.StochasticBuilder(5, eng, pipelined=True, margins=gc.TOL)
        else:
            eng.compute_margins(pred, rules)
    assert _state() == before
    assert eng.model.ctx.margin_calls == [] and not wc_calls(eng)
    if what in ("fp64", "sharding"):  # through the attribute as well, and compute_margins restored it
        assert eng.margin_tol is None
        eng.margin_tol = gc.TOL
        with pytest.raises(NotImplementedError, match="margins"):
            eng.compute_relevance_batch(pred, rules)
        assert _state() == before


def wc_calls(eng):
    """The slots the recording stand-in under the margins stand-in has run."""
    return eng.model.ctx.inner.slots


# ----------------------------------------------------------------------------- with the other requests
@pytest.mark.parametrize("name", ["ComplEx", "TransE"])
def test_keyed_mode(name):
    case = gc.FAMILY[0] if name == "ComplEx" else gc.FAMILY[3]
    ds = wc.graph(517)[1]
    pred = wc.graph(517)[2][0]
    rules = [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]

    def engine():
        model = wc.make_model(case)
        model._ctx = KeyedStandIn(standin(model), model)
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(wc.hp_of(case), epochs=EPOCHS))
        eng.draws, eng.seed = "keyed", 7
        return eng

    before = _state()
    eng = engine()
    out = eng.compute_margins(pred, rules)
    assert eng.model.ctx.keyed_calls == 1 and eng.model.ctx.inner.margin_calls == [1e-4]
    assert [o["relevance"] for o in out] == engine().compute_relevance_batch(pred, rules)
    assert all(o["post"]["rank_lo"] <= o["post"]["rank"] <= o["post"]["rank_hi"] for o in out)
    # keyed: a rule's report does not depend on its batch
    alone = engine().compute_margins(pred, [rules[1]])
    assert alone[0] == out[1]
    assert _state() == before


def test_with_marks_and_top_k_in_one_call():
    """margins with marks (whose stand-in serves the mark rows the margins stand-in then
    scores) in one call: the marks' margins at hp.epochs are the slots'."""
    case = gc.FAMILY[0]
    ds = wc.graph(517)[1]
    model = wc.make_model(case)
    model._ctx = ctx = MarginsStandIn(MarksContext(wc.oracle_context(model), model.name))
    eng = ka.NecessaryPostTrainingEngine(model, ds, dict(wc.hp_of(case), epochs=EPOCHS))
    eng.marks = [0, EPOCHS]
    pred = wc.graph(517)[2][0]
    rules = [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]
    gc.seed_all(42)
    out = eng.compute_margins(pred, rules, tol=1e-2)
    assert ctx.margin_calls == [1e-2] and ctx.inner.mark_calls == [[0, EPOCHS]]
    kinds = [r[0] for r in ctx.rows[0]]
    assert kinds.count("slot") == 3 and kinds.count("mark") == 6
    for (pt, base), o in zip(eng.last_results, out):
        assert [m["epoch"] for m in pt["marks"]] == [0, EPOCHS] and pt["marks"][-1]["rank"] == o["post"]["rank"]
    # the definition on a mark row at hp.epochs is the slot's
    slots = [r for r in ctx.rows[0] if r[0] == "slot"]
    marks = [r for r in ctx.rows[0] if r[0] == "mark"]
    for i, s in enumerate(slots):
        assert np.array_equal(marks[2 * i + 1][1], s[1]) and marks[2 * i + 1][3] == s[3]


# ----------------------------------------------------------------------------- builder, pipeline
@pytest.mark.parametrize("mode", MODES)
def test_pipeline_records(mode):
    case = gc.FAMILY[0]
    ds, ordinary = wc.graph(517)[1:3]
    pred = ordinary[0]
    recs = {}
    for margins in (None, gc.TOL):
        model = wc.make_model(case)
        model._ctx = standin(model)
        gc.seed_all(42)
        kw = {} if margins is None else {"margins": margins}
        pipe = build_pipeline(model, ds, dict(wc.hp_of(case), epochs=EPOCHS), mode, xsi=1e9, **kw)
        pipe.builder.length_cap = 1
        if mode == "sufficient":
            recs[margins] = pipe.explain(pred, prefilter_k=3, to_convert_k=2)
        else:
            recs[margins] = pipe.explain(pred, prefilter_k=3)
    plain, rec = recs[None], recs[gc.TOL]
    assert "margins" not in plain and set(rec) == set(plain) | {"margins"}
    assert rec["rule_to_relevance"] == plain["rule_to_relevance"] and rec["#relevances"] == plain["#relevances"]
    assert len(rec["margins"]) == len(rec["rule_to_relevance"]) > 0
    for (_, rel), m in zip(rec["rule_to_relevance"], rec["margins"]):
        assert m["relevance"] == rel
        if mode == "necessary":
            assert set(m) == {"relevance", "relevance_lo", "relevance_hi", "base", "post"}
            assert set(m["post"]) == SIDE_KEYS and m["post"]["rank_lo"] <= m["post"]["rank"] <= m["post"]["rank_hi"]
        else:
            assert set(m) == {"relevance", "relevance_lo", "relevance_hi", "conversions"}
            assert [c["entity"] for c in m["conversions"]] == rec["entities_to_convert"]
        assert m["relevance_lo"] <= m["relevance_hi"]
    assert pipe.engine.margin_tol == gc.TOL and pipe.builder.margins == gc.TOL


# ----------------------------------------------------------------------------- the library's symbol
def test_library_symbol_and_split():
    assert "kp_posttrain_rank_margins" in _lib.EXPORTS
    out = (1, 2, 3, "top", "margins")
    res = _lib.split_rank_result(out, topk=4, margins=0.5)
    assert res.top == "top" and res.margins == "margins" and res.marks is None
    with pytest.raises(ValueError):
        _lib.split_rank_result(out[:4], topk=4, margins=0.0)  # tol 0 is a request
    assert _lib.check_margin_tol(0) == 0.0 and _lib.check_margin_tol(np.float32(1.0)) == 1.0


# ----------------------------------------------------------------------------- conditions on the inputs
@pytest.mark.parametrize("case", gc.FAMILY, ids=gc.ids(gc.FAMILY))
def test_inputs_can_decide(case):
    """On the 517-entity graph at tol = 1e-4 (the device tests' inputs, at their 8 epochs) the
    stand-in's rank rows include one with a band and one without; and, for the families whose
    values numpy recomputes, no compared column lies within the summation bound of a threshold
    at the tolerances the device tests hold against the host."""
    batches, model, _ = gc.run(case, lambda m: MarginsStandIn(MarksContext(wc.oracle_context(m), m.name)),
                               tol=gc.TOL, marks=[0, 3, 8])
    rows = [r for log in model.ctx._ctx.rows for r in log]
    assert len(rows) == 2 * 3 * 4  # two subjects x three slots x (the slot and three marks)
    mode = gc.mode_of(model)
    width = [m["rank_hi"] - m["rank_lo"] for m in (mr.margins(mode, r[1], r[2], r[3], gc.TOL, saturated=r[4]) for r in rows)]
    assert any(w > 0 for w in width) and any(w == 0 for w in width), width
    if case["model"] not in gc.HOST:
        return
    for kind, _, masked, o, _, triple, x in rows:
        c, eps = gc.host_compared(model, triple[1], x)
        for tol in (0.0, gc.TOL, 1e-2):
            for name, (_, _, near) in mr.count_bounds(mode, c, masked, o, tol, 2 * (eps + eps[o])).items():
                assert near == 0, (kind, triple, tol, name)
