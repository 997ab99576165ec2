"""Replay of tests/golden/probes_tiny.json (TEST INFRASTRUCTURE): the reference's
get_triple_results on every probe of every post-trained Kelpie model of the tiny TransE,
ComplEx and ConvE cases (tools/make_probe_golden.py), against ``compute_side_effects``
through a stand-in or the device context.  The small goldens' own rule: ranks exact,
scores to 1e-4 (engine_cases.TOL)."""
from __future__ import annotations

import kelpie_amd as ka
from engine_cases import TOL, build_product
from golden_io import seed_all


def oracle_ctx(model):
    """The oracle-backed stand-in ``build_product(name, "cpu")`` installed, serving probes."""
    from probe_backend import ProbeContext
    return ProbeContext(model._ctx, model.is_minimizer())


def replay(rec, ctx_of):
    """The record's rules through ``compute_side_effects``; per rule its relevance and its
    results in the reference's call order: per post-training the base (when it was not yet
    cached), then the post-trained model."""
    backend = "cpu" if ctx_of is oracle_ctx else "gpu"
    fixture, ds, model = build_product(rec["name"], backend)
    model._ctx = ctx_of(model)
    pred = tuple(rec["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in rec["calls"]]
    seed_all(rec["seed"])
    if rec["mode"] == "necessary":
        eng = ka.NecessaryPostTrainingEngine(model, ds, fixture["hp"])
    else:
        eng = ka.SufficientPostTrainingEngine(model, ds, fixture["hp"])
        eng.select_entities_to_convert(pred, rec["k"], rec["degree_cap"])
        assert [int(e) for e in eng.entities_to_convert] == rec["entities_to_convert"]
    out = eng.compute_side_effects(pred, rules, probes=[tuple(t) for t in rec["probes"]])
    calls, seen = [], set()
    for o in out:
        results = []
        for side in ([dict(o, entity=pred[0])] if rec["mode"] == "necessary" else o["conversions"]):
            if side["entity"] not in seen:
                seen.add(side["entity"])
                results.append(side["base"])
            results.append(side["post"])
        calls.append({"relevance": o["relevance"], "results": results})
    return calls


def compare(rec, got):
    assert len(got) == len(rec["calls"])
    n = 0
    for want, have in zip(rec["calls"], got):
        assert abs(have["relevance"] - want["relevance"]) <= TOL * max(1.0, abs(want["relevance"])), (want, have)
        assert len(have["results"]) == len(want["results"])
        for w, h in zip(want["results"], have["results"]):
            assert h["rank"] == w["rank"] and abs(h["score"] - w["score"]) <= TOL * max(1.0, abs(w["score"])), (w, h)
            assert len(h["probes"]) == len(w["probes"]) == len(rec["probes"])
            for wp, hp in zip(w["probes"], h["probes"]):
                assert list(hp["triple"]) == wp["triple"], (wp, hp)
                assert hp["rank"] == wp["rank"], (rec["name"], rec["mode"], wp, hp)
                assert abs(hp["score"] - wp["score"]) <= TOL * max(1.0, abs(wp["score"])), (wp, hp)
                n += 1
            # the own-target probe is the slot's own result, on both sides
            assert w["probes"][0]["rank"] == w["rank"] and w["probes"][0]["score"] == w["score"]
            assert h["probes"][0]["rank"] == h["rank"] and h["probes"][0]["score"] == h["score"]
    return n
