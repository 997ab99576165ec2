"""Probes, host layers (CPU tier): ``compute_side_effects``, the engine's ``side_effects``,
the builder / pipeline ``side_effects`` and the ``output.json`` schema, over the
oracle-backed stand-in contexts wrapped to serve probes (probe_backend.py); the rank rule's
decidability on the device's cases (probe_cases.py); the reference fixture.  The device side
is test_probes_gpu.py.
"""
import inspect
import json
import os
import random

import numpy as np
import pytest
import torch

import kelpie_amd as ka
import probe_cases as pc
from engine_cases import build_product
from golden_io import seed_all
from kelpie_amd import _lib
from kelpie_amd.pipeline import build_pipeline, explain_preds, read_preds, run_explain
from probe_backend import triple_results, wrap

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probes_tiny.json")


def _state():
    return (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
            random.getstate())


def _necessary(name="complex_tiny", probe_ctx=True):
    rec, ds, model = build_product(name, "cpu")
    ctx = wrap(model) if probe_ctx else model._ctx
    block = rec["necessary"][0]
    pred = tuple(block["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in block["calls"]]
    return rec, ds, model, ctx, pred, rules


def _own_target_holds(side):
    """Consequence 1 on a side whose first probe is the slot's own prediction."""
    own = side["probes"][0]
    assert own["score"] == side["score"] and own["rank"] == side["rank"], (own, side)


# ----------------------------------------------------------------------------- the definition
def test_triple_results_definition():
    row = np.array([0.5, 2.0, 2.0, -1.0, 3.0, 0.25], np.float32)  # column 5: the kelpie entity
    assert triple_results(row, [], 1, False) == (2.0, 3)          # >=: the tie counts
    assert triple_results(row, [4, 4, 2], 1, False) == (2.0, 1)
    assert triple_results(row, [1, 4], 1, False) == (2.0, 1)      # a filtered o does not count itself: only column 2
    assert triple_results(row, [], 5, False) == (0.25, 5)         # o = the kelpie entity
    assert triple_results(row, [], 3, True) == (-1.0, 1)          # minimizer: <=
    assert triple_results(row, [3, 5], 0, True) == (0.5, 1)       # filtered columns go to 1e6
    assert triple_results(row, [0, 3], 0, True) == (0.5, 2)       # ... and a filtered o is restored


def test_symbol_declared_and_bound():
    assert "kp_posttrain_rank_probes" in _lib.EXPORTS
    L = _lib.lib()
    assert L.kp_posttrain_rank_probes(None, None, None, 0, None, None, None) != 0  # null context: refused, no device
    assert inspect.signature(_lib.Context.posttrain_rank).parameters["probes"].default is None
    for f in (ka.StochasticBuilder.__init__, build_pipeline, run_explain):
        assert inspect.signature(f).parameters["side_effects"].default == 0
    assert inspect.signature(explain_preds).parameters["side_effects"].default is None


def test_default_probes_and_kelpie_form():
    rec, ds, model, ctx, pred, rules = _necessary()
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    s = pred[0]
    held = [tuple(t) for t in ds.entity_to_validation_triples.get(s, [])] + \
           [tuple(t) for t in ds.entity_to_testing_triples.get(s, [])]
    want = [t for t in held if t != pred]
    assert eng.default_probes(pred, 16) == want[:16] and eng.default_probes(pred, 1) == want[:1]
    assert pred not in eng.default_probes(pred, 64)
    # s as tail gives the inverse relation's (p + |R|, head); a self-loop the kelpie entity itself
    view = eng._get_kelpie_dataset(s)
    other = next(e for e in range(ds.num_entities) if e != s)
    eng._cur_probes = (s, [(other, 1, s), (s, 0, s), (s, 1, other)])
    got = [po for _, po, _ in eng._slot_probes(view, None)]
    assert got == [(1 + ds.num_relations, other), (0, ds.num_entities), (1, other)]


# ----------------------------------------------------------------------------- without probes: today's call
def test_no_probes_pass_no_new_keyword():
    rec, ds, model, ctx, pred, rules = _necessary(probe_ctx=False)
    assert "probes" not in inspect.signature(ctx.posttrain_rank).parameters
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    eng.compute_relevance_batch(pred, rules)
    assert all("probes" not in pt and "probes" not in base for pt, base in eng.last_results)
    eng.set_cache()
    with pytest.raises(TypeError, match="probes"):
        eng.compute_side_effects(pred, rules)


# ----------------------------------------------------------------------------- compute_side_effects
@pytest.mark.parametrize("name", ["complex_tiny", "transe_tiny", "conve60_tiny"])
def test_side_effects_equal_relevance_batch(name):
    """Same relevances, same generator state afterwards, same batches; consequence 1."""
    rec, ds, model, ctx, pred, rules = _necessary(name)
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    plain = eng.compute_relevance_batch(pred, rules)
    after_plain = _state()
    calls = list(ctx.calls)
    assert set(ctx.probe_calls) == {0}

    probes = [pred] + eng.default_probes(pred, 16) + [tuple(t) for t in ds.entity_to_training_triples[pred[0]][:2]]
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    out = eng.compute_side_effects(pred, rules, probes=probes)
    assert _state() == after_plain
    assert [o["relevance"] for o in out] == plain
    assert ctx.calls[len(calls):] == calls  # the same batches of the same slots
    assert ctx.probe_calls[len(calls):] == [len(probes) * n for n in calls]
    assert eng.side_effects == 0 and eng._probe_req is None
    for o in out:
        assert set(o) == {"relevance", "base", "post"}
        for side in (o["base"], o["post"]):
            assert set(side) == {"score", "rank", "probes"}
            assert [p["triple"] for p in side["probes"]] == probes
            assert all(set(p) == {"triple", "score", "rank"} and p["rank"] >= 0 for p in side["probes"])
            _own_target_holds(side)
    # the default: the subject's held-out triples
    eng.set_cache()
    out = eng.compute_side_effects(pred, rules[:1], cap=3)
    assert [p["triple"] for p in out[0]["post"]["probes"]] == eng.default_probes(pred, 3)


def test_distmult_side_effects():
    from distmult_backend import DistMultOracleContext, load_fixture
    rec, ds, model = load_fixture()
    model._ctx = DistMultOracleContext(model)
    assert "probes" not in inspect.signature(model._ctx.posttrain_rank).parameters
    pred = tuple(int(v) for v in ds.testing_triples[0])
    rules = [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]
    hp = rec["slots"][0]["hp"]
    seed_all(42)
    plain = ka.NecessaryPostTrainingEngine(model, ds, hp).compute_relevance_batch(pred, rules)
    ctx = wrap(model)
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    probes = [pred] + [tuple(t) for t in ds.entity_to_training_triples[pred[0]][:3]]
    out = eng.compute_side_effects(pred, rules, probes=probes)
    assert [o["relevance"] for o in out] == plain and ctx.probe_calls == [3 * len(probes)]
    for o in out:
        _own_target_holds(o["base"])
        _own_target_holds(o["post"])
    # builder record
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    res = ka.StochasticBuilder(1e9, eng, max_explanation_length=1, side_effects=4).build_explanations(
        pred, [r[0] for r in rules])
    _check_side_effect_records(res["side_effects"], res["rule_to_relevance"], eng.default_probes(pred, 4), ds)


def test_sufficient_side_effects():
    rec, ds, model = build_product("complex_tiny", "cpu")
    ctx = wrap(model)
    block = rec["sufficient"][0]
    pred = tuple(block["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in block["calls"]]

    def engine():
        seed_all(rec["seed"])
        eng = ka.SufficientPostTrainingEngine(model, ds, rec["hp"])
        eng.select_entities_to_convert(pred, block["k"], block["degree_cap"])
        return eng

    eng = engine()
    plain = eng.compute_relevance_batch(pred, rules)
    after = _state()
    eng = engine()
    probes = [pred] + eng.default_probes(pred, 16)
    out = eng.compute_side_effects(pred, rules, probes=probes)
    assert _state() == after and [o["relevance"] for o in out] == plain
    s = pred[0]
    for o in out:
        assert set(o) == {"relevance", "conversions"}
        assert [c["entity"] for c in o["conversions"]] == list(eng.entities_to_convert)
        for c in o["conversions"]:
            assert set(c) == {"entity", "base", "post"}
            moved = [ka.Dataset.replace_entity_in_triple(t, s, c["entity"]) for t in probes]
            for side in (c["base"], c["post"]):
                assert [p["triple"] for p in side["probes"]] == moved  # does c inherit them?
                _own_target_holds(side)
    assert set(ctx.probe_calls) - {0}


def test_cached_base_reports_none_and_is_not_rerun():
    rec, ds, model, ctx, pred, rules = _necessary()
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    eng.compute_relevance_batch(pred, rules[:1])  # caches the base result, without probes
    slots_before = sum(ctx.calls)
    out = eng.compute_side_effects(pred, rules[1:])
    assert sum(ctx.calls) - slots_before == len(rules) - 1  # the post-trainings only: no base run again
    for o in out:
        assert o["base"]["probes"] is None and o["base"]["rank"] >= 1
        assert len(o["post"]["probes"]) == len(eng.default_probes(pred, 16))
    eng.set_cache()
    out = eng.compute_side_effects(pred, rules[:1])
    assert out[0]["base"]["probes"] is not None


def test_errors_before_any_draw():
    rec, ds, model, ctx, pred, rules = _necessary()
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    before = _state()
    s = pred[0]
    a, b = [e for e in range(ds.num_entities) if e != s][:2]
    with pytest.raises(Exception, match="Could not find the original entity"):
        eng.compute_side_effects(pred, rules, probes=[pred, (a, 0, b)])
    with pytest.raises(ValueError, match="64"):
        eng.compute_side_effects(pred, rules, probes=[pred] * 65)
    with pytest.raises(ValueError):
        eng.compute_side_effects(pred, rules, cap=-1)
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            eng.side_effects = bad
        with pytest.raises(ValueError):
            ka.StochasticBuilder(5, eng, side_effects=bad)
    for bad in (1.5, "3", True):
        with pytest.raises((TypeError, ValueError)):
            eng.side_effects = bad
    assert _state() == before and ctx.probe_calls == [] and eng.side_effects == 0 and eng._probe_req is None
    eng.compute_side_effects(pred, rules[:1], probes=[pred] * 64)  # the most a slot takes


def test_sharding_refused_before_any_draw():
    rec, ds, model, ctx, pred, rules = _necessary()

    class Sharding:
        world, rank = 2, 0

        def __getattr__(self, name):
            raise AssertionError(f"sharding used: {name}")

    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    eng.sharding = Sharding()
    before = _state()
    with pytest.raises(NotImplementedError):
        eng.compute_side_effects(pred, rules)
    eng.side_effects = 2
    with pytest.raises(NotImplementedError):
        eng.compute_relevance_batch(pred, rules)
    assert _state() == before and ctx.probe_calls == []


def test_context_checks_lengths_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("library reached"))
    ctx = object.__new__(_lib.Context)
    ctx.dim = 2
    z = np.zeros
    with pytest.raises(ValueError, match="probe_off"):
        ctx.posttrain_rank(None, z((1, 2)), [0, 1], z((1, 3)), [0, 0], [0], z((1, 3)), [0, 0], [0],
                           probes=([0, 1, 1], [[0, 0]], [0, 0], []))


# ----------------------------------------------------------------------------- builder, pipeline, output.json
def _check_side_effect_records(records, rule_to_relevance, probes, ds, entities=None):
    assert len(records) == len(rule_to_relevance) >= 1
    labelled = [list(ds.labels_triple(t)) for t in probes]
    some_base = False
    for rec in records:
        for r in ([rec] if entities is None else rec):
            assert set(r) == {"probes", "base", "post", "ranks"} | ({"entity"} if entities is not None else set())
            assert r["probes"] == len(probes) == len(r["ranks"])
            assert all(isinstance(k[2], int) and k[2] >= 0 for k in r["ranks"])
            post = [max(1, k[2]) for k in r["ranks"]]  # rank 0: a filtered object the model answers first
            # compute_metrics' formulas and rounding (verification.py)
            mrr = round(sum(1.0 / float(v) for v in post) / float(len(post)), 3)
            h1 = round(sum(1.0 for v in post if v <= 1) / float(len(post)), 3)
            assert r["post"] == {"mrr": mrr, "h1": h1}
            if r["base"] is not None:
                some_base = True
                base = [max(1, k[1]) for k in r["ranks"]]
                assert r["base"]["mrr"] == round(sum(1.0 / float(v) for v in base) / float(len(base)), 3)
            else:
                assert all(k[1] is None for k in r["ranks"])
            if entities is None:
                assert [k[0] for k in r["ranks"]] == labelled
        if entities is not None:
            assert [r["entity"] for r in rec] == entities
    assert some_base


def _explain(tmpdir, name, mode, cap):
    rec, ds, model = build_product(name, "cpu")
    wrap(model)
    seed_all(rec["seed"])
    # a test prediction whose subject has other held-out facts to probe
    pred = next(t for t in (tuple(int(v) for v in t) for t in ds.testing_triples)
                if len(ds.entity_to_validation_triples.get(t[0], [])) + len(ds.entity_to_testing_triples.get(t[0], [])) >= 3
                and 3 <= len(ds.entity_to_training_triples.get(t[0], [])) <= 40)
    n_cand, xsi = 3, (rec["builder"]["xsi"] if mode == "necessary" else None)
    preds_path = os.path.join(tmpdir, f"preds_{mode}_{cap}.csv")
    with open(preds_path, "w") as f:
        f.write("\t".join(ds.labels_triple(pred)) + "\n")
    kw = {"side_effects": cap} if cap else {}
    pipe = build_pipeline(model, ds, rec["hp"], mode, xsi=xsi, **kw)
    out_path = os.path.join(tmpdir, f"output_{mode}_{cap}.json")
    explain_preds(pipe, ds, read_preds(preds_path), prefilter_k=n_cand, output_path=out_path)
    with open(out_path) as f:
        return ds, pred, json.load(f)[0], pipe


@pytest.mark.parametrize("name", ["complex_tiny", "transe_tiny", "conve60_tiny"])
def test_output_json_necessary(name, tmp_path):
    ds, pred, plain, _ = _explain(str(tmp_path), name, "necessary", 0)
    assert "side_effects" not in plain
    ds, pred, rec3, pipe = _explain(str(tmp_path), name, "necessary", 3)
    assert set(rec3) == set(plain) | {"side_effects"}
    # the search itself is unchanged
    assert rec3["rule_to_relevance"] == plain["rule_to_relevance"] and rec3["#relevances"] == plain["#relevances"]
    _check_side_effect_records(rec3["side_effects"], rec3["rule_to_relevance"], pipe.engine.default_probes(pred, 3), ds)
    assert pipe.engine.side_effects == 3 and pipe.builder.side_effects == 3


def test_output_json_sufficient(tmp_path):
    ds, pred, plain, _ = _explain(str(tmp_path), "complex_tiny", "sufficient", 0)
    ds, pred, rec2, pipe = _explain(str(tmp_path), "complex_tiny", "sufficient", 2)
    assert set(rec2) == set(plain) | {"side_effects"}
    assert rec2["rule_to_relevance"] == plain["rule_to_relevance"]
    _check_side_effect_records(rec2["side_effects"], rec2["rule_to_relevance"], pipe.engine.default_probes(pred, 2), ds,
                               entities=rec2["entities_to_convert"])


# ----------------------------------------------------------------------------- the device's cases decide
@pytest.mark.parametrize("case", pc.CASES, ids=pc.ids())
def test_rank_rule_decides(case):
    """On the oracle alone: every probe's rank bounds at most one apart, at least three
    quarters of a case's probes with a single admissible rank (the condition
    test_width_cases_cpu.py uses), the stand-in's own rank inside, consequence 1."""
    import width_cases as wc
    call, model = pc.run(case, pc.oracle_ctx)
    n, exact, sharp, widest = pc.check_probes(call, model, wc.oracle_context(model))
    assert n == sum(pc.COUNTS) == 65 and widest <= 1 and 4 * sharp >= 3 * n, (n, sharp, widest)
    assert pc.check_own_target(call) == 5
    p_off, tr, f_off, fl = call["probes"]
    assert tr[1, 1] == case["n_ent"] and tr[2, 1] in fl[f_off[2]:f_off[3]]
    assert p_off.tolist() == [0, 16, 16, 33, 34, 49, 65]


# ----------------------------------------------------------------------------- the reference fixture
def test_reference_fixture():
    import probe_golden as pg
    with open(GOLDEN) as f:
        golden = json.load(f)
    kinds = set()
    for rec in golden["cases"]:
        pg.compare(rec, pg.replay(rec, pg.oracle_ctx))
        kinds |= set(rec["kinds"])
    assert {"self-loop", "filtered-object", "compound"} <= kinds
    assert {(r["model"], r["mode"]) for r in golden["cases"]} == {(m, k) for m in ("TransE", "ComplEx", "ConvE")
                                                                    for k in ("necessary", "sufficient")}
