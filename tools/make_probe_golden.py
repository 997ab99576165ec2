"""Generate tests/golden/probes_tiny.json from the reference.

Run in the development container only (needs the reference checkout that
tests/golden/ref_harness.py loads):

    python tools/make_probe_golden.py

For the tiny TransE, ComplEx and ConvE cases of tests/golden/make_golden.py (same graphs,
same weights: the fixture names their .npz files) it runs the reference's necessary and
sufficient engines on two singleton rules and one compound rule, with
``engine.get_triple_results`` wrapped as make_golden.py's ``record_engine_calls`` wraps it:
after every call the original is called again on the same post-trained Kelpie model, still
holding its edited KelpieDataset, for every kelpie-form probe (post_training_engine.py:
101-125).  That consumes no draw, so the relevances are those of the committed goldens.

Probes, about the prediction's subject s and moved to the conversion entity as the
prediction is: the prediction itself, s's other held-out facts (their objects are in
to_filter: filtered objects) and one of its training facts (filtered too), a fact nobody knows (unfiltered), a fact with s as tail (the
inverse relation) and the self-loop (s, p, s) (the kelpie entity as its own object).

The output is data: triples, scores and ranks.  No reference source is stored.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

import make_golden as mg  # noqa: E402
import ref_harness  # noqa: E402

NAMES = ("transe_tiny", "complex_tiny", "conve60_tiny")
CAP = 4


def pick_probes(dataset, pred):
    """The probes of a prediction, in original ids, with what each is there for."""
    s, p, o = pred
    held = [tuple(int(v) for v in t) for t in list(dataset.entity_to_validation_triples.get(s, []))
            + list(dataset.entity_to_testing_triples.get(s, []))]
    held = [t for t in held if t != tuple(pred)][:CAP]
    known = set(map(tuple, dataset.all_triples.tolist())) if hasattr(dataset, "all_triples") else set()
    free = next((s, p, e) for e in range(dataset.num_entities) if e not in (s, o) and (s, p, e) not in known
                and e not in dataset.to_filter.get((s, p), []))
    tail = next((e, p, s) for e in range(dataset.num_entities) if e != s and (e, p, s) not in known)
    # a training fact of s (as head): its object is filtered whether or not s has held-out facts
    held.append(next(tuple(int(v) for v in t) for t in dataset.entity_to_training_triples[s] if int(t[0]) == s))
    probes = [tuple(pred)] + held + [free, tail, (s, p, s)]
    kinds = ["own-target"] + ["filtered-object"] * len(held) + ["unfiltered", "inverse", "self-loop"]
    return probes, kinds


def record(engine, pred, rules, probes, subject):
    """make_golden.record_engine_calls, with every probe ranked on the same model after
    each get_triple_results call."""
    from src.data import Dataset
    log = []
    orig = engine.get_triple_results

    def wrapped(model, triple):
        r = orig(model, triple)
        kd = model.dataset
        k, nrel = kd.kelpie_entity, kd.num_relations
        rows = []
        for t in probes:
            moved = Dataset.replace_entity_in_triple(t, subject, kd.original_entity)
            a, p, b = kd.as_kelpie_triple(moved)
            if a != k:  # the entity is the tail: head prediction through the inverse relation
                p, b = p + nrel, a
            pr = orig(model, (k, int(p), int(b)))
            rows.append({"triple": [int(v) for v in moved], "kelpie": [int(p), int(b)],
                         "score": float(pr["target_score"]), "rank": int(pr["target_rank"])})
        log.append({"triple": [int(v) for v in triple], "score": float(r["target_score"]),
                    "rank": int(r["target_rank"]), "probes": rows})
        return r

    engine.get_triple_results = wrapped
    out = []
    for rule in rules:
        log.clear()
        rel = engine.compute_relevance(pred, list(rule))
        out.append({"rule": [[int(v) for v in t] for t in rule], "relevance": float(rel), "results": list(log)})
    engine.get_triple_results = orig
    return out


def main():
    src = ref_harness.load_reference()
    from src.prefilters import TopologyPreFilter
    from src.relevance_engines import NecessaryPostTrainingEngine, SufficientPostTrainingEngine
    cases = []
    for name in NAMES:
        cfg = mg.CASES[name]
        g, w, dataset, model = mg.build_case(src, name, cfg)
        pred = mg.pick_preds(dataset, g)[0]
        prefilter = TopologyPreFilter(dataset)
        probes, kinds = pick_probes(dataset, pred)
        for mode in ("necessary", "sufficient"):
            ref_harness.seed_all(42)
            cls = NecessaryPostTrainingEngine if mode == "necessary" else SufficientPostTrainingEngine
            engine = cls(model, dataset, cfg["hp"])
            engine.set_cache()
            conv = None
            if mode == "sufficient":
                engine.select_entities_to_convert(pred, 2, 200)
                conv = [int(e) for e in engine.entities_to_convert]
            cands = prefilter.select_triples(pred=pred, k=4)
            rules = [(cands[0],), (cands[1],), (cands[0], cands[1])]
            calls = record(engine, pred, rules, probes, pred[0])
            cases.append({"name": name, "model": cfg["model"], "mode": mode, "seed": 42, "pred": list(pred),
                          "k": 2, "degree_cap": 200, "entities_to_convert": conv,
                          "probes": [list(t) for t in probes], "kinds": kinds + ["compound"], "calls": calls})
            print(name, mode, pred, conv, [round(c["relevance"], 4) for c in calls],
                  [[p["rank"] for p in r["probes"]] for r in calls[-1]["results"]], flush=True)
    with open(os.path.join(GOLDEN, "probes_tiny.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1, default=mg._to_py)


if __name__ == "__main__":
    main()
