"""DistMult natively against its ComplEx embedding, on the device (recorded, not gated).

FB15k-237 shape, d = 200, sufficient mode, K = 10 conversion entities, 43 Adagrad epochs
(the shape of bench.py's complex-fb15k237-sufficient).  Two legs post-train the same slots:

* ``native``:   ka.DistMult (rows of 200 floats, attention at D = 208);
* ``embedded``: ka.ComplEx on the zero-imaginary tables [E | 0], [R | 0] with
  ``init_scale`` unchanged (D = 400) -- what a user could do before DistMult was a model
  family.  Its kelpie init draws 2d values, so its rows differ from the native leg's;
  the work (slots, rows, steps) is the same.

Same process, alternating legs, ``--rounds`` rounds after a warm-up of each leg.  Per leg:
candidates per second (wall clock around compute_relevance_batch, which ends in a device
synchronise), and from the last batch kp_last_timing's device seconds, hot-kernel
(attention) seconds and launches, and kp_last_attn_plan.

    python tools/distmult_probe.py [--out profiles/distmult/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kelpie_amd as ka  # noqa: E402
from kelpie_amd import synth  # noqa: E402

HP = {"optimizer_name": "Adagrad", "batch_size": 512, "epochs": 43, "lr": 0.043, "decay1": 0.9, "decay2": 0.999,
      "regularizer_name": "N3", "regularizer_weight": 0}


def seed_all(seed):
    import random

    import torch
    np.random.seed(seed)
    torch.manual_seed(seed)
    random.seed(seed)


def pick_pred(ds, seed=1234, lo=5, hi=200):
    rng = np.random.default_rng(seed)
    test = ds.testing_triples
    for i in rng.permutation(len(test)):
        s, p, o = (int(v) for v in test[i])
        if lo <= ds.entity_to_degree.get(s, 0) <= hi:
            return s, p, o
    raise RuntimeError("no prediction with a subject of the wanted degree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="FB15k-237")
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--convert", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distmult", "probe.json"))
    args = ap.parse_args()

    g = synth.make_graph(args.shape, seed=0)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    w = synth.make_weights("DistMult", g.num_entities, g.num_relations, args.dim, seed=0)
    E, R = w["entity_embeddings"], w["relation_embeddings"]
    legs = {"native": ka.DistMult(ds, E, R),
            "embedded": ka.ComplEx(ds, np.hstack([E, np.zeros_like(E)]), np.hstack([R, np.zeros_like(R)]))}
    pred = pick_pred(ds)
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:args.candidates]
    rules = [[c] for c in cands]

    def run(name):
        model = legs[name]
        seed_all(42)
        eng = ka.SufficientPostTrainingEngine(model, ds, HP)
        ents = eng.select_entities_to_convert(pred, args.convert, 200)
        t0 = time.perf_counter()
        rels = eng.compute_relevance_batch(pred, rules)
        dt = time.perf_counter() - t0
        out = {"seconds": dt, "cand_per_s": len(rules) / dt, "entities": len(ents)}
        out.update(model.ctx.last_timing())
        out.update(model.ctx.last_attn_plan())
        out["relevance_sum"] = float(np.sum(rels))
        return out

    for name in legs:  # warm-up: code objects, workspaces, pinned arenas
        run(name)
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: run(name) for name in legs})
    rec = {"shape": args.shape, "dim": args.dim, "mode": "sufficient", "convert": args.convert,
           "candidates": len(rules), "hp": HP, "pred": list(pred), "attention": ka._lib.attention_contraction(),
           "rounds": rounds}
    for name in legs:
        rec[name] = {k: float(np.median([r[name][k] for r in rounds]))
                     for k in ("cand_per_s", "seconds", "device_s", "hot_s", "hot_launches")}
    rec["native_over_embedded"] = rec["native"]["cand_per_s"] / rec["embedded"]["cand_per_s"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("native", "embedded", "native_over_embedded")}), flush=True)


if __name__ == "__main__":
    main()
