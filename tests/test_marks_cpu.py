"""Epoch marks, CPU tier: the host layers -- ``compute_curves``, the engine's ``marks`` -- over
the oracle-backed stand-in contexts wrapped to answer marks by the definition
(marks_backend.py: the same batch with ``hp.epochs = e_j``), on every scheduling path, and the
library's symbol.  The device side is test_marks_gpu.py, the host check test_marks_check.py.
"""
import inspect
import random

import numpy as np
import pytest
import torch

import kelpie_amd as ka
from engine_cases import build_product
from golden_io import seed_all
from kelpie_amd import _lib
from marks_backend import MarksContext

NAMES = ["complex_tiny", "transe_tiny", "conve60_tiny"]


def _state():
    return (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
            random.getstate())


def _marks_of(rec):
    E = int(rec["hp"]["epochs"])
    return sorted({0, 1, max(1, E // 2), E})


def _setup(name, mode, force_epochs=None):
    rec, ds, model = build_product(name, "cpu")
    model._ctx = ctx = MarksContext(model._ctx, model.name, force_epochs=force_epochs)
    block = rec[mode][0]
    pred = tuple(block["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in block["calls"]]

    def engine():
        seed_all(rec["seed"])
        if mode == "necessary":
            return ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
        eng = ka.SufficientPostTrainingEngine(model, ds, rec["hp"])
        eng.select_entities_to_convert(pred, block["k"], block["degree_cap"])
        return eng

    return rec, ctx, pred, rules, engine


def _sides(out, mode):
    """(base, post) of every post-training pair a curve report holds."""
    for o in out:
        if mode == "necessary":
            yield o["base"], o["post"]
        else:
            for c in o["conversions"]:
                yield c["base"], c["post"]


# plain: ComplEx and ConvE, and TransE with checkpoints; fused: TransE's sufficient calls;
# native: TransE's necessary calls without checkpoints (the library's host scheduler)
PATHS = [(n, m, False) for n in NAMES for m in ("necessary", "sufficient")] + \
    [("transe_tiny", m, True) for m in ("necessary", "sufficient")]


@pytest.mark.parametrize("name,mode,checkpoints", PATHS,
                         ids=[f"{n}-{m}" + ("-checkpoints" if c else "") for n, m, c in PATHS])
def test_curves_equal_relevance_batch(name, mode, checkpoints):
    """The same relevances, generator states and batches as compute_relevance_batch; the last
    mark is the final result; every mark sits on its own slot."""
    rec, ctx, pred, rules, engine = _setup(name, mode)
    marks = _marks_of(rec)
    eng = engine()
    cps = [] if checkpoints else None
    plain = eng.compute_relevance_batch(pred, rules, cps) if checkpoints else eng.compute_relevance_batch(pred, rules)
    after_plain = _state()
    calls = list(ctx.calls)
    assert ctx.mark_calls and all(m is None for m in ctx.mark_calls)
    n0 = len(ctx.mark_calls)

    eng = engine()
    if checkpoints:  # compute_curves takes no checkpoints: the property serves that path
        eng.marks = marks
        rels = eng.compute_relevance_batch(pred, rules, [])
        out = [eng._mk_rule(r, d, marks) for r, d in zip(rels, eng.last_results)]
    else:
        out = eng.compute_curves(pred, rules, marks)
        assert eng.marks is None
    assert _state() == after_plain
    assert [o["relevance"] for o in out] == plain
    assert ctx.calls[len(calls):] == calls and all(m == marks for m in ctx.mark_calls[n0:])
    keys = {"relevance", "epochs", "curve"} | ({"base", "post"} if mode == "necessary" else {"conversions"})
    n_pairs = 0
    for o in out:
        assert set(o) == keys and o["epochs"] == marks and len(o["curve"]) == len(marks)
        # the last mark is hp.epochs: the curve ends at the relevance itself
        assert o["curve"][-1] == o["relevance"], (o["curve"], o["relevance"])
    for base, post in _sides(out, mode):
        n_pairs += 1
        for side in (base, post):
            assert set(side) == {"score", "rank", "marks"}
            assert [m["epoch"] for m in side["marks"]] == marks
            assert all(set(m) == {"epoch", "score", "rank"} for m in side["marks"])
            last = side["marks"][-1]
            assert last["score"] == side["score"] and last["rank"] == side["rank"]
        # mark 0 is x0's result, which the edit changes through the filter alone
        assert base["marks"][0]["rank"] >= 1 and post["marks"][0]["rank"] >= 1
    assert n_pairs >= len(rules)
    # the marks move: some post-training has two marks of different rank
    assert any(len({m["rank"] for m in side["marks"]}) > 1 for pair in _sides(out, mode) for side in pair)


@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
@pytest.mark.parametrize("name", NAMES)
def test_curve_is_the_shorter_engines_relevance(name, mode):
    """curve[j] equals the relevance of a stand-in engine whose slots ran e_j epochs on the same
    draws per post-training."""
    rec, ctx, pred, rules, engine = _setup(name, mode)
    marks = _marks_of(rec)
    out = engine().compute_curves(pred, rules, marks)
    for j, e in enumerate(marks):
        _, _, pred_e, rules_e, engine_e = _setup(name, mode, force_epochs=e)
        want = engine_e().compute_relevance_batch(pred_e, rules_e)
        assert [o["curve"][j] for o in out] == want, (e, [o["curve"][j] for o in out], want)


def test_marks_property_and_cached_base():
    rec, ctx, pred, rules, engine = _setup("complex_tiny", "necessary")
    marks = _marks_of(rec)
    eng = engine()
    assert eng.marks is None
    eng.compute_relevance_batch(pred, rules[:1])  # caches the base result, without marks
    slots_before = sum(ctx.calls)
    out = eng.compute_curves(pred, rules[1:], marks)
    assert sum(ctx.calls) - slots_before == len(rules) - 1  # the post-trainings only: no base run again
    for o in out:
        assert o["base"]["marks"] is None and o["curve"] is None and o["base"]["rank"] >= 1
        assert [m["epoch"] for m in o["post"]["marks"]] == marks
    # a base cached with other marks does not serve these
    eng.set_cache()
    eng.compute_curves(pred, rules[:1], marks[:2])
    out = eng.compute_curves(pred, rules[1:2], marks)
    assert out[0]["base"]["marks"] is None and out[0]["curve"] is None
    out = eng.compute_curves(pred, rules[1:2], marks[:2])
    assert [m["epoch"] for m in out[0]["base"]["marks"]] == marks[:2] and len(out[0]["curve"]) == 2
    # the property: validated on set, reported on every result
    eng.set_cache()
    eng.marks = marks
    assert eng.marks == marks
    eng.compute_relevance_batch(pred, rules[:1])
    pt, base = eng.last_results[0]
    assert [m["epoch"] for m in pt["marks"]] == marks and [m["epoch"] for m in base["marks"]] == marks
    E = int(rec["hp"]["epochs"])
    for bad in ([], list(range(17)), [1, 1], [2, 1], [-1, 0], [0, E + 1]):
        with pytest.raises(ValueError):
            eng.marks = bad
    for bad in (3, "01", [0.5], [True], [None]):
        with pytest.raises(TypeError):
            eng.marks = bad
    assert eng.marks == marks
    eng.marks = None
    assert eng.marks is None


def test_bad_epochs_raise_before_any_draw():
    rec, ctx, pred, rules, engine = _setup("complex_tiny", "necessary")
    E = int(rec["hp"]["epochs"])
    eng = engine()
    before = _state()
    for bad, err in (([], ValueError), (list(range(17)), ValueError), ([1, 1], ValueError), ([3, 2], ValueError),
                     ([-1], ValueError), ([E + 1], ValueError), (2, TypeError), ([1.0], TypeError),
                     (["1"], TypeError), (None, TypeError)):
        with pytest.raises(err):
            eng.compute_curves(pred, rules, bad)
    assert _state() == before and ctx.mark_calls == [] and eng.marks is None


def test_no_marks_passes_no_new_keyword():
    rec, ds, model = build_product("complex_tiny", "cpu")
    ctx = model._ctx
    assert "marks" not in inspect.signature(ctx.posttrain_rank).parameters
    block = rec["necessary"][0]
    pred = tuple(block["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in block["calls"]]
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    eng.compute_relevance_batch(pred, rules)
    eng.set_cache()
    with pytest.raises(TypeError, match="marks"):
        eng.compute_curves(pred, rules, [0, 1])


def test_sharding_refused_before_any_draw():
    rec, ctx, pred, rules, engine = _setup("complex_tiny", "necessary")

    class Sharding:
        world, rank = 2, 0

        def __getattr__(self, name):
            raise AssertionError(f"sharding used: {name}")

    eng = engine()
    eng.sharding = Sharding()
    before = _state()
    with pytest.raises(NotImplementedError, match="marks"):
        eng.compute_curves(pred, rules, [0, 1])
    eng.marks = [0, 1]
    with pytest.raises(NotImplementedError, match="marks"):
        eng.compute_relevance_batch(pred, rules)
    assert _state() == before and ctx.mark_calls == []


def test_check_marks():
    assert _lib.check_marks([0, 1, 3], 3).tolist() == [0, 1, 3]
    assert _lib.check_marks(np.array([2, 5]), 5).dtype == np.int32
    assert _lib.check_marks(range(16), 15).tolist() == list(range(16))
    assert _lib.check_marks((4,)).tolist() == [4]


def test_symbol_declared_and_bound():
    """The library on CPU: the symbol is exported and a null context is refused."""
    assert "kp_posttrain_rank_marks" in _lib.EXPORTS
    L = _lib.lib()
    assert L.kp_posttrain_rank_marks(None, None, None, 0, None, None, None, None, None) != 0
    assert inspect.signature(_lib.Context.posttrain_rank).parameters["marks"].default is None
    fields = [f[0] for f in _lib.Marks._fields_]
    assert fields == ["n", "epochs", "out_score", "out_rank", "out_x"]


# ----------------------------------------------------------------------------- the reference fixture
def test_fixture_conditions():
    """The generator's conditions, asserted again on the file."""
    import marks_golden as mg
    rec = mg.golden()
    assert rec["epochs"] == 6 and rec["marks"] == [0, 1, 2, 4, 6]
    names = [c["name"] for c in rec["cases"]]
    assert names == ["complex8_n3", "complex8_adam", "distmult8_n3", "complex200_n3", "transe16_l2", "transe16_l1",
                     "conve60", "conve60_drop"]
    for case in rec["cases"]:
        flat = [m for pt in case["posttrainings"] for m in pt["marks"]]
        for pt in case["posttrainings"]:
            assert [m["epoch"] for m in pt["marks"]] == rec["marks"] and pt["hp"]["epochs"] == 6
        for m in flat:
            # reference agreement, and the rank rule decides
            assert abs(m["score32"] - m["score64"]) <= 1e-4 * max(1.0, abs(m["score64"])), (case["name"], m)
            assert m["hi"] - m["lo"] <= 1 and m["lo"] <= m["rank32"] <= m["hi"] and m["lo"] <= m["rank64"] <= m["hi"]
        assert 4 * sum(int(m["lo"] == m["hi"]) for m in flat) >= 3 * len(flat), case["name"]
        # the marks move: a feature that returned the final result everywhere must fail
        assert any(len({m["rank64"] for m in pt["marks"]}) > 1 and len({m["rank32"] for m in pt["marks"]}) > 1
                   for pt in case["posttrainings"]), case["name"]
    by = {c["name"]: c for c in rec["cases"]}
    steps = [-(-len(pt["rows"]) // pt["hp"]["batch_size"]) for pt in by["complex8_n3"]["posttrainings"]]
    assert [pt["kind"] for pt in by["complex8_n3"]["posttrainings"]] == ["base", "necessary", "sufficient"]
    assert steps == [3, 2, 1]
    assert by["complex8_adam"]["posttrainings"][0]["hp"]["optimizer_name"] == "Adam"
    assert by["transe16_l2"]["weights"]["norm"] == 2 and by["transe16_l1"]["weights"]["norm"] == 1
    assert by["conve60"]["rates"] == [0.0, 0.0, 0.0] and by["conve60_drop"]["rates"] == [0.2, 0.3, 0.1]
    for name in ("conve60", "conve60_drop"):  # a last step of one pair, no logit near the clamp
        pt = by[name]["posttrainings"][0]
        assert pt["pairs"] % pt["hp"]["batch_size"] == 1 and pt["max_logit"] < 16 / 1.25


def _fixture_ids():
    import marks_golden as mg
    return [pid for pid, _, _ in mg.posttrainings()]


@pytest.mark.parametrize("pid", _fixture_ids())
def test_standin_equals_fixture(pid):
    """The stand-in's marks (the oracle on the same batch with hp.epochs = e) against the values
    the reference gave inside one run: scores within 1e-4, ranks by the rank rule."""
    import marks_golden as mg
    import width_cases as wc
    _, case, pt = next(p for p in mg.posttrainings() if p[0] == pid)
    model = mg.make_model(case)
    ctx = MarksContext(wc.oracle_context(model), model.name)
    s, r, x, (ms, mr, mx) = ctx.posttrain_rank(*mg.batch(model, case, pt), want_x=True, marks=mg.golden()["marks"])
    print(pid, "row error", mg.row_error(pt, mx[0]), "of the fp64 row's scale")
    exact = mg.check(pid, pt, ms[0], mr[0], mx[0])  # the rows of every family that the fixture keeps
    print(pid, "ranks", mr[0].tolist(), "exact", exact)
    assert float(ms[0, -1]) == float(s[0]) and int(mr[0, -1]) == int(r[0])


def test_marks_cases_are_decided_by_the_standin():
    """The GPU cases' stand-in side alone: the rank rule decides every case's marks and they move."""
    import marks_cases as mc
    for case in mc.CASES + mc.MIXED:
        ref, spe = mc.reference(case)
        mc.check_marks_vacuity(ref)
        if case.get("mixed"):
            assert sorted(spe[0]) == [1, 2, 3], spe
