"""Top-k tails, host layers (CPU tier): the engine's ``top_k``, ``compute_counterfactuals``,
the builder / pipeline ``top_k`` and the ``output.json`` schema, over the oracle-backed
stand-in contexts wrapped to serve lists (topk_backend.py).  The device side is
test_topk_gpu.py.
"""
import inspect
import json
import os
import random

import numpy as np
import pytest
import torch

import kelpie_amd as ka
from engine_cases import TOL, build_product
from golden_io import seed_all
from kelpie_amd import _lib
from kelpie_amd.pipeline import build_pipeline, explain_preds, read_preds, run_explain
from topk_backend import TopkContext, reference_topk, wrap


def _state():
    return (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
            random.getstate())


def _necessary(name="complex_tiny", topk_ctx=True):
    rec, ds, model = build_product(name, "cpu")
    ctx = wrap(model) if topk_ctx else model._ctx
    block = rec["necessary"][0]
    pred = tuple(block["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in block["calls"]]
    return rec, ds, model, ctx, pred, rules


# ----------------------------------------------------------------------------- validation of k
@pytest.mark.parametrize("bad", [-1, 33, 100])
def test_top_k_out_of_range(bad):
    rec, ds, model, ctx, pred, rules = _necessary()
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    assert eng.top_k == 0
    with pytest.raises(ValueError):
        eng.top_k = bad
    assert eng.top_k == 0
    with pytest.raises(ValueError):
        eng.compute_counterfactuals(pred, rules, bad)
    with pytest.raises(ValueError):
        ka.StochasticBuilder(5, eng, top_k=bad)
    assert ctx.topk_calls == []  # refused before any library call


def test_top_k_type_and_zero():
    rec, ds, model, ctx, pred, rules = _necessary()
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    for bad in (1.5, "3", True):
        with pytest.raises((TypeError, ValueError)):
            eng.top_k = bad
    with pytest.raises(ValueError):
        eng.compute_counterfactuals(pred, rules, 0)  # a counterfactual needs a list
    for ok in (0, 1, 32):
        eng.top_k = ok
        assert eng.top_k == ok


@pytest.mark.parametrize("bad", [-1, 33])
def test_context_refuses_k_before_the_library(bad, monkeypatch):
    """_lib.Context.posttrain_rank checks topk before it touches the library."""
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("library reached"))
    ctx = object.__new__(_lib.Context)
    with pytest.raises(ValueError):
        ctx.posttrain_rank(None, None, [0, 1], None, None, None, None, None, None, topk=bad)


def test_symbol_declared_and_bound():
    assert "kp_posttrain_rank_topk" in _lib.EXPORTS
    L = _lib.lib()
    assert L.kp_posttrain_rank_topk(None, None, None, 5, None, None) != 0  # null context: refused, no device
    assert "topk" in inspect.signature(_lib.Context.posttrain_rank).parameters


# ----------------------------------------------------------------------------- top_k == 0 is today's call
def test_top_k_zero_passes_no_new_keyword():
    """The existing stand-ins take no ``topk`` keyword: the engine at top_k = 0 must call them
    as before, and at top_k > 0 the call carries the keyword (which they reject)."""
    rec, ds, model, ctx, pred, rules = _necessary(topk_ctx=False)
    assert "topk" not in inspect.signature(ctx.posttrain_rank).parameters
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    rels = eng.compute_relevance_batch(pred, rules)
    for call, rel in zip(rec["necessary"][0]["calls"], rels):
        assert abs(rel - call["relevance"]) <= TOL
    assert all("top_ids" not in pt and "top_ids" not in base for pt, base in eng.last_results)
    eng.set_cache()
    eng.top_k = 3
    with pytest.raises(TypeError, match="topk"):
        eng.compute_relevance_batch(pred, rules)


def test_distmult_stand_in_untouched():
    from distmult_backend import DistMultOracleContext, load_fixture
    rec, ds, model = load_fixture()
    model._ctx = DistMultOracleContext(model)
    assert "topk" not in inspect.signature(model._ctx.posttrain_rank).parameters
    pred = tuple(int(v) for v in ds.testing_triples[0])
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:2]
    hp = rec["slots"][0]["hp"]
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    plain = eng.compute_relevance_batch(pred, [[c] for c in cands])
    ctx = wrap(model)
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    out = eng.compute_counterfactuals(pred, [[c] for c in cands], 4)
    assert [o["relevance"] for o in out] == plain
    assert ctx.topk_calls == [4]
    for o in out:
        ids = [e for e, _ in o["post"]["top"]]
        assert len(ids) == 4 and len(set(ids)) == 4
        sc = [v for _, v in o["post"]["top"]]
        assert sc == sorted(sc, reverse=True)


# ----------------------------------------------------------------------------- compute_counterfactuals
@pytest.mark.parametrize("name", ["complex_tiny", "transe_tiny", "conve60_tiny"])
def test_counterfactuals_equal_relevance_batch(name):
    """Same relevances, same generator state afterwards, same batches."""
    rec, ds, model, ctx, pred, rules = _necessary(name)
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    plain = eng.compute_relevance_batch(pred, rules)
    after_plain = _state()
    n_calls = len(ctx.topk_calls)
    assert set(ctx.topk_calls) == {0}

    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    out = eng.compute_counterfactuals(pred, rules, 3)
    assert _state() == after_plain
    assert [o["relevance"] for o in out] == plain
    assert ctx.topk_calls[n_calls:] == [3] * n_calls
    assert eng.top_k == 0  # the call's k does not stick
    minimizer = model.is_minimizer()
    K = ds.num_entities
    for o in out:
        assert set(o) == {"relevance", "base", "post"}
        for side in (o["base"], o["post"]):
            assert set(side) == {"score", "rank", "top"}
            top = side["top"]
            assert 1 <= len(top) <= 3
            ids, sc = [e for e, _ in top], [v for _, v in top]
            assert all(0 <= e <= K for e in ids) and len(set(ids)) == len(ids)
            assert sc == sorted(sc, reverse=not minimizer)
            # the rank invariant: an unmasked target of rank <= k is among the first `rank` ids
            if side["rank"] <= 3 and (minimizer or pred[2] not in _filter_of(ds, pred)):
                assert pred[2] in ids[:side["rank"]], (side, pred)


def _filter_of(ds, pred):
    return set(ds.to_filter.get((pred[0], pred[1]), []))


def test_sufficient_counterfactuals():
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
    out = eng.compute_counterfactuals(pred, rules, 2)
    assert _state() == after and [o["relevance"] for o in out] == plain
    for o in out:
        assert set(o) == {"relevance", "conversions"}
        assert [c["entity"] for c in o["conversions"]] == list(eng.entities_to_convert)
        for c in o["conversions"]:
            assert set(c) == {"entity", "base", "post"}
            assert len(c["post"]["top"]) == 2 and len(c["base"]["top"]) == 2
    assert set(ctx.topk_calls) == {0, 2}


def test_cached_base_reports_none_and_is_not_rerun():
    rec, ds, model, ctx, pred, rules = _necessary()
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    eng.compute_relevance_batch(pred, rules[:1])  # caches the base result, without a list
    slots_before = sum(ctx.calls)
    out = eng.compute_counterfactuals(pred, rules[1:], 3)
    assert sum(ctx.calls) - slots_before == len(rules) - 1  # the post-trainings only: no base run again
    for o in out:
        assert o["base"]["top"] is None
        assert o["base"]["rank"] >= 1 and len(o["post"]["top"]) == 3
    # a fresh cache gives the base its list
    eng.set_cache()
    out = eng.compute_counterfactuals(pred, rules[:1], 3)
    assert out[0]["base"]["top"] is not None


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
        eng.compute_counterfactuals(pred, rules, 3)
    eng.top_k = 2
    with pytest.raises(NotImplementedError):
        eng.compute_relevance_batch(pred, rules)
    assert _state() == before and ctx.topk_calls == []


# ----------------------------------------------------------------------------- the -1 cut and the kelpie label
class _FixedLists(TopkContext):
    """Serves a fixed list per slot: the kelpie column first, one entity, then the -1 tail."""

    def posttrain_rank(self, *a, want_x=False, topk=0):
        out = super().posttrain_rank(*a, want_x=want_x, topk=topk)
        if topk:
            ids, top = out[3]
            ids[:, 0] = self.n_ent
            ids[:, 2:] = -1
            top[:, 2:] = 0.0
        return out


def test_cut_at_first_minus_one_and_kelpie_label():
    rec, ds, model = build_product("complex_tiny", "cpu")
    model._ctx = _FixedLists(model._ctx, False)
    b = rec["builder"]
    pred = tuple(b["pred"])
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    out = eng.compute_counterfactuals(pred, [[tuple(b["candidates"][0])]], 5)
    top = out[0]["post"]["top"]
    assert len(top) == 2 and top[0][0] == ds.num_entities and top[1][0] >= 0

    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    res = ka.StochasticBuilder(b["xsi"], eng, top_k=5).build_explanations(pred, [tuple(t) for t in b["candidates"]])
    for cf in res["counterfactuals"]:
        for side in (cf["base"], cf["post"]):
            assert len(side) == 2
            assert side[0][0] == "kelpie:" + ds.id_to_entity[pred[0]]
            assert side[1][0] in ds.entity_to_id


def test_reference_topk_definition():
    row = np.array([0.5, 2.0, 2.0, -1.0, 3.0, 0.25], np.float32)  # column 5: the kelpie entity
    ids, vals = reference_topk(row, [4, 4, 1], obj=1, k=8, minimizer=False)
    assert ids.tolist() == [2, 0, 5, 3, -1, -1, -1, -1] and vals[4:].tolist() == [0, 0, 0, 0]
    ids, _ = reference_topk(row, [4, 3], obj=3, k=3, minimizer=True)  # the filtered target restored
    assert ids.tolist() == [3, 5, 0]
    ids, _ = reference_topk(row, [], obj=0, k=2, minimizer=False)  # the tie: lower id first
    assert ids.tolist() == [4, 1]


# ----------------------------------------------------------------------------- builder, pipeline, output.json
def _explain(tmpdir, mode, top_k):
    rec, ds, model = build_product("complex_tiny", "cpu")
    wrap(model)
    seed_all(rec["seed"])
    if mode == "necessary":
        b = rec["builder"]
        pred, n_cand, xsi = tuple(b["pred"]), len(b["candidates"]), b["xsi"]
    else:
        pred, n_cand, xsi = tuple(rec["sufficient"][0]["pred"]), 4, None
    preds_path = os.path.join(tmpdir, f"preds_{mode}_{top_k}.csv")
    with open(preds_path, "w") as f:
        f.write("\t".join(ds.labels_triple(pred)) + "\n")
    kw = {"top_k": top_k} if top_k else {}
    pipe = build_pipeline(model, ds, rec["hp"], mode, xsi=xsi, **kw)
    out_path = os.path.join(tmpdir, f"output_{mode}_{top_k}.json")
    explain_preds(pipe, ds, read_preds(preds_path), prefilter_k=n_cand, output_path=out_path)
    with open(out_path) as f:
        text = f.read()
    return ds, pred, json.loads(text)[0], pipe


def test_output_json_necessary(tmp_path):
    ds, pred, plain, _ = _explain(str(tmp_path), "necessary", 0)
    assert set(plain) == {"triple", "rule_to_relevance", "#relevances", "execution_time"}
    ds, pred, rec3, pipe = _explain(str(tmp_path), "necessary", 3)
    assert set(rec3) == set(plain) | {"counterfactuals"}
    # the search itself is unchanged
    assert rec3["rule_to_relevance"] == plain["rule_to_relevance"] and rec3["#relevances"] == plain["#relevances"]
    assert len(rec3["counterfactuals"]) == len(rec3["rule_to_relevance"])
    labels = set(ds.entity_to_id) | {"kelpie:" + ds.id_to_entity[pred[0]]}
    some_base = False
    for cf in rec3["counterfactuals"]:
        assert set(cf) == {"base", "post"}
        assert 1 <= len(cf["post"]) <= 3
        for lab, score in cf["post"] + (cf["base"] or []):
            assert lab in labels and isinstance(score, float)
        some_base |= cf["base"] is not None
    assert some_base
    assert pipe.engine.top_k == 3 and pipe.builder.top_k == 3


def test_output_json_sufficient(tmp_path):
    ds, pred, plain, _ = _explain(str(tmp_path), "sufficient", 0)
    assert "counterfactuals" not in plain
    ds, pred, rec2, pipe = _explain(str(tmp_path), "sufficient", 2)
    assert set(rec2) == set(plain) | {"counterfactuals"}
    assert rec2["rule_to_relevance"] == plain["rule_to_relevance"]
    assert len(rec2["counterfactuals"]) == len(rec2["rule_to_relevance"])
    for cf in rec2["counterfactuals"]:
        assert [c["entity"] for c in cf] == rec2["entities_to_convert"]
        for c in cf:
            assert set(c) == {"entity", "base", "post"} and len(c["post"]) == 2
            for lab, _ in c["post"]:
                assert lab in ds.entity_to_id or lab == "kelpie:" + c["entity"]


def test_signatures_default_to_zero():
    for f in (ka.StochasticBuilder.__init__, build_pipeline, run_explain):
        assert inspect.signature(f).parameters["top_k"].default == 0
    assert inspect.signature(_lib.Context.posttrain_rank).parameters["topk"].default == 0
