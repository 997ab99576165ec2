"""Reference fixture for DistMult: tests/golden/distmult_tiny.json (data only).

Runs the imported reference (``tests/golden/ref_harness.load_reference()``; the tool
skips itself when the reference is absent) on a seeded tiny model and records

* ``DistMult.all_scores`` and ``DistMult.forward`` (scores and the three regulariser
  factors, distmult.py:51-68) for a few (h, r);
* the reference's ``KelpieComplEx`` + ``KelpieMultiClassNLLOptimizer`` post-training of
  the zero-imaginary tables [E | 0], [R | 0] with a zero-imaginary ``init_tensor``
  (DistMult of width d is ComplEx of width 2d with zero imaginary halves; the
  reference's own KelpieDistMult cannot be constructed, distmult.py:77,86): the final
  row, the largest magnitude of its imaginary half, the target score and rank and the
  score row, in the reference's fp32 run and in an fp64 run (tables, init and default
  dtype float64; the permutations are the fp32 run's).

    python tools/make_distmult_golden.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import ref_harness  # noqa: E402
from kelpie_amd import synth  # noqa: E402

GRAPH = {"shape": "tiny", "seed": 11}
WEIGHTS = {"dim": 16, "seed": 11, "trained_scale": 0.3}
INIT_SCALE = 0.5
HP = {"optimizer_name": "Adagrad", "batch_size": 256, "epochs": 10, "lr": 0.043, "decay1": 0.9, "decay2": 0.999,
      "regularizer_name": "N3", "regularizer_weight": 0.0}
# (name, hp overrides): one minibatch per epoch; several (the permutations are recorded); N3; N2 with Adam
SLOTS = [("one_step", {}), ("multi_step", {"batch_size": 16}),
         ("n3", {"regularizer_weight": 0.05, "batch_size": 16}),
         ("n2_adam", {"regularizer_name": "N2", "regularizer_weight": 0.05, "optimizer_name": "Adam", "lr": 0.01})]
OUT = os.path.join(ROOT, "tests", "golden", "distmult_tiny.json")


def tables():
    g = synth.make_graph(GRAPH["shape"], seed=GRAPH["seed"])
    w = synth.make_weights("DistMult", g.num_entities, g.num_relations, WEIGHTS["dim"], seed=WEIGHTS["seed"],
                           trained_scale=WEIGHTS["trained_scale"])
    return g, w


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def f9(a):
    """Nine significant digits: exact for float32 data, 1e-9 relative on the fp64 score rows."""
    a = np.asarray(a, np.float64)
    return [f9(r) for r in a] if a.ndim > 1 else [float(f"{v:.9g}") for v in a]


def pad(a):
    return np.hstack([a, np.zeros_like(a)])


def posttrain(engine, kd, model, init, hp, kelpie_triple, perms=None):
    """One reference post-training of the kelpie row from ``init`` over the kelpie dataset's
    training triples; ``perms``: replayed permutations, else they are drawn and returned."""
    from src.link_prediction import MODEL_REGISTRY
    drawn, orig = [], torch.randperm

    def randperm(n, *a, **k):
        p = orig(n, *a, **k) if perms is None else torch.as_tensor(perms[len(drawn)], dtype=torch.int64)
        drawn.append(p.tolist())
        return p

    km = model.kelpie_model_class()(kd, model, init.clone())
    cls = MODEL_REGISTRY["ComplEx"]["optimizer"]
    opt = cls.get_kelpie_class()(model=km, hp=cls.get_hyperparams_class()(**hp), verbose=False)
    torch.randperm = randperm
    try:
        opt.train(training_triples=np.array(kd.kelpie_training_triples))
    finally:
        torch.randperm = orig
    km.eval()
    with torch.no_grad():
        scores = km.all_scores(np.array([kelpie_triple]))[0].detach().double().numpy().copy()
    res = engine.get_triple_results(km, kelpie_triple)
    row = km.kelpie_entity_emb.detach().double().numpy()[0]
    d = row.shape[0] // 2
    return {"row": row[:d].tolist(), "imag_max": float(np.abs(row[d:]).max()), "score": float(res["target_score"]),
            "rank": int(res["target_rank"]), "scores": f9(scores)}, drawn


def main():
    if not os.path.isdir(os.path.join(ref_harness.REF_ROOT, "src")):
        print("reference absent: nothing written")
        return
    ref_harness.load_reference()
    torch.set_num_threads(2)
    from src.data import Dataset, KelpieDataset
    from src.link_prediction.models.complex import ComplEx, ComplExHyperParams
    from src.link_prediction.models.distmult import DistMult, DistMultHyperParams
    from src.relevance_engines import NecessaryPostTrainingEngine

    g, w = tables()
    d = WEIGHTS["dim"]
    ref_harness.register_dataset("distmult_tiny", g.num_entities, g.num_relations, g.train, g.valid, g.test)
    dataset = Dataset("distmult_tiny")
    rec = {"graph": GRAPH, "weights": WEIGHTS, "init_scale": INIT_SCALE,
           "sha256": {k: sha(w[k]) for k in ("entity_embeddings", "relation_embeddings")}}

    # ---- DistMult.all_scores / forward
    ref_harness.seed_all(42)
    dm = DistMult(dataset=dataset, hp=DistMultHyperParams(dimension=d, init_scale=INIT_SCALE))
    with torch.no_grad():
        dm.entity_embeddings.data = torch.from_numpy(w["entity_embeddings"].copy())
        dm.relation_embeddings.data = torch.from_numpy(w["relation_embeddings"].copy())
    trip = np.asarray(g.test[:3], dtype=np.int64)
    with torch.no_grad():
        sc = dm.all_scores(trip)
        fsc, (f0, f1, f2) = dm.forward(trip)
    rec["model"] = {"triples": trip.tolist(), "all_scores": f9(sc.numpy()), "forward_scores": f9(fsc.numpy()),
                    "factors": [f9(f0.numpy()), f9(f1.numpy()), f9(f2.numpy())]}

    # ---- post-training on the zero-imaginary embedding
    deg = {}
    for h, _, t in g.train.tolist():
        deg[h] = deg.get(h, 0) + 1
        deg[t] = deg.get(t, 0) + 1
    pred = next(tuple(int(v) for v in t) for t in g.test.tolist() if 12 <= deg.get(t[0], 0) <= 30)
    ref_harness.seed_all(42)
    init = torch.rand(1, d)
    rec["pred"], rec["init"] = list(pred), init.numpy()[0].tolist()
    rec["slots"] = []
    for name, over in SLOTS:
        hp = dict(HP, **over)
        out = {"name": name, "hp": hp}
        perms = None
        for variant, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
            torch.set_default_dtype(dtype)
            try:
                cx = ComplEx(dataset=dataset, hp=ComplExHyperParams(dimension=d, init_scale=INIT_SCALE))
                with torch.no_grad():
                    cx.entity_embeddings.data = torch.from_numpy(pad(w["entity_embeddings"])).to(dtype)
                    cx.relation_embeddings.data = torch.from_numpy(pad(w["relation_embeddings"])).to(dtype)
                cx.eval()
                kd = KelpieDataset(dataset=dataset, entity=pred[0])
                eng = NecessaryPostTrainingEngine(cx, dataset, hp)
                ref_harness.seed_all(7)
                init2 = torch.cat([init, torch.zeros_like(init)], 1).to(dtype)
                out[variant], drawn = posttrain(eng, kd, cx, init2, hp, kd.as_kelpie_triple(pred), perms)
                perms = drawn
                if variant == "fp32":
                    del out[variant]["scores"]  # the rank rule reads the fp64 run's row
            finally:
                torch.set_default_dtype(torch.float32)
        rec["kelpie_training_triples"] = np.asarray(kd.kelpie_training_triples).tolist()
        out["n_rows"] = len(perms[0])
        out["perms"] = perms if out["n_rows"] > hp["batch_size"] else None
        out["kelpie_triple"] = [int(v) for v in kd.as_kelpie_triple(pred)]
        out["filter"] = [int(v) for v in kd.to_filter.get((out["kelpie_triple"][0], out["kelpie_triple"][1]), [])]
        rec["slots"].append(out)
        print(name, {v: (out[v]["score"], out[v]["rank"], out[v]["imag_max"]) for v in ("fp32", "fp64")})
    with open(OUT, "w") as f:
        json.dump(rec, f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
