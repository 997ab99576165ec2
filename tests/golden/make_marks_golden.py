"""Reference fixture for the epoch marks: tests/golden/marks_golden.json (data only).

TEST INFRASTRUCTURE, run in the development container only: it imports the reference through
``ref_harness`` (and skips itself when the reference is absent).  For every case it runs the
reference's own Kelpie optimizer on a seeded tiny model for 6 epochs and, before the first
epoch and after epochs 1, 2, 4 and 6, calls the reference's ``get_triple_results``
(post_training_engine.py:101-125) on the model under training.  That call evaluates in eval
mode and draws nothing (asserted here: the generator states before and after it are equal);
the optimizers put the model back into train mode at the next epoch.  Every value is taken
inside ONE reference run: the reference started with ``epochs = e`` from the same seed is
another thing (include/kelpie_hip.h, "Epoch marks").

Recorded per mark: the reference's fp32 run's score and rank, and the score, rank, rank rule's
bounds (width_cases.rank_bounds on the fp64 score row) and kelpie row of an fp64 run on the
same draws (tables, init, optimizer state and arithmetic in float64).  The graph, the tables,
``kelpie_init``, the draw recording and ``ref_harness`` are make_trace_golden.py's.

Cases (the 300-entity synthetic graph): ComplEx d = 8 Adagrad N3 0.05 for the subject's own
rows (base), with one triple removed (necessary) and another entity's rows with the subject's
triple added (sufficient), at batch sizes that give 3, 2 and 1 steps per epoch; ComplEx d = 8
Adam; DistMult d = 8 through the zero-imaginary tables; ComplEx d = 200; TransE d = 16 with the
L2 and the L1 norm; ConvE d = 60 without dropouts and with (0.2, 0.3, 0.1), a last step of one
pair.

The generator asserts what tests/test_marks_cpu.py asserts again on the file: fp32 and fp64
scores agree within 1e-4 * max(1, |s64|); every mark's bounds are at most one apart and at
least three quarters of a case's marks have a single admissible rank; the ConvE training
logits stay below 16 / 1.25; in every case two marks of some post-training differ in rank.
The weight seed of a case is the first of SEEDS that meets them.

    python tests/golden/make_marks_golden.py
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness  # noqa: E402
from make_trace_golden import GRAPH, INIT_SCALE, LOGIT_BOUND, MaskedDropouts, kelpie_init, pack_masks, transe_draws  # noqa: E402
from kelpie_amd import synth  # noqa: E402

EPOCHS = 6
MARKS = [0, 1, 2, 4, 6]
TOL = 1e-4
SEEDS = range(3, 40)
OUT = os.path.join(HERE, "marks_golden.json")
ALL, BASE = ("base", "necessary", "sufficient"), ("base",)
NLL_HP = {"optimizer_name": "Adagrad", "batch_size": 0, "epochs": EPOCHS, "lr": 0.043, "decay1": 0.9,
          "decay2": 0.999, "regularizer_name": "N3", "regularizer_weight": 0.05}
TRANSE_HP = {"batch_size": 0, "epochs": EPOCHS, "lr": 0.01, "margin": 5, "negative_triples_ratio": 5,
             "regularizer_weight": 1.0}
CONVE_HP = {"batch_size": 0, "epochs": EPOCHS, "label_smoothing": 0.1, "lr": 0.0432, "decay": 0.995}
# (case, family, dim, weight options, hp overrides, post-trainings, keep the rows)
CASES = [
    ("complex8_n3", "ComplEx", 8, {"trained_scale": 0.3}, {}, ALL, True),
    ("complex8_adam", "ComplEx", 8, {"trained_scale": 0.3}, {"optimizer_name": "Adam", "lr": 0.01}, BASE, True),
    ("distmult8_n3", "DistMult", 8, {"trained_scale": 0.3}, {}, BASE, True),
    ("complex200_n3", "ComplEx", 200, {"trained_scale": 0.3}, {}, BASE, False),
    ("transe16_l2", "TransE", 16, {"norm": 2}, {}, BASE, True),
    ("transe16_l1", "TransE", 16, {"norm": 1}, {}, BASE, True),
    ("conve60", "ConvE", 60, {"rates": (0.0, 0.0, 0.0)}, {}, BASE, True),
    ("conve60_drop", "ConvE", 60, {"rates": (0.2, 0.3, 0.1)}, {}, BASE, True),
]
STEPS_PER_EPOCH = {"base": 3, "necessary": 2, "sufficient": 1}  # complex8_n3's three post-trainings


def rng_states():
    return (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
            random.getstate())


def rank_bounds(scores, target, filt, obj, minimizer):
    """width_cases.rank_bounds, restated (the generator imports no test module)."""
    s = np.asarray(scores, np.float64).copy()
    target = float(target)
    delta = TOL * max(1.0, abs(target))
    filt = np.asarray(filt, np.int64)
    own = 1 if minimizer or int(obj) not in set(filt.tolist()) else 0
    if minimizer:
        s[filt] = 1e6
        s[obj] = 2e6
        return own + int((s <= target - delta).sum()), own + int((s <= target + delta).sum())
    s[filt] = -1e6
    s[obj] = -2e6
    return own + int((s >= target + delta).sum()), own + int((s >= target - delta).sum())


def mark(km, kelpie_pred):
    """The reference's get_triple_results on the model under training, drawing nothing; with
    the score row it ranked (before the masking) and the kelpie row."""
    from src.relevance_engines.post_training_engine import PostTrainingEngine
    before = rng_states()
    res = PostTrainingEngine.get_triple_results(None, km, kelpie_pred)
    with torch.no_grad():
        row = km.all_scores(np.array([kelpie_pred]))[0].detach().double().numpy().copy()
    assert rng_states() == before, "get_triple_results drew from a generator"
    assert float(row[kelpie_pred[2]]) == float(res["target_score"])
    return {"score": float(res["target_score"]), "rank": int(res["target_rank"]), "scores": row,
            "row": km.kelpie_entity_emb.detach().double().numpy()[0].tolist()}


def run_with_marks(opt, km, kelpie_pred, train):
    """``train()`` with a mark before the first epoch and after every epoch of MARKS."""
    marks, done, inner = [mark(km, kelpie_pred)], [0], opt.epoch

    def epoch(*a, **k):
        out = inner(*a, **k)
        done[0] += 1
        if done[0] in MARKS:
            marks.append(mark(km, kelpie_pred))
        return out

    opt.epoch = epoch
    train()
    assert done[0] == EPOCHS and len(marks) == len(MARKS)
    return marks


def kelpie_triple(pred, original, kelpie):
    return tuple(kelpie if v == original and i != 1 else int(v) for i, v in enumerate(pred))


def rows_of(kd, n_rel):
    tr = np.array(kd.kelpie_training_triples)
    inv = tr[:, [2, 1, 0]].copy()
    inv[:, 1] += n_rel
    return np.vstack([tr, inv])


def batch_size_for(R, steps):
    """The largest batch size that gives ``steps`` steps per epoch with a shorter last one
    (steps == 1: the rows in one batch)."""
    if steps == 1:
        return R
    for bs in range(R, 0, -1):
        if (R + bs - 1) // bs == steps and R % bs != 0:
            return bs
    raise ValueError(f"no batch size for {R} rows in {steps} steps")


def nll_or_transe(family, model, kd, init, hp, perms, kelpie_pred):
    """One reference post-training with marks; the permutations (ComplEx: replayed from
    ``perms`` when given) and the (positive, negative) batches of every step (TransE)."""
    from src.link_prediction import MODEL_REGISTRY
    drawn, steps, orig = [], [], torch.randperm
    transe = family == "TransE"

    def randperm(n, *a, **k):
        p = orig(n, *a, **k) if perms is None else torch.as_tensor(perms[len(drawn)], dtype=torch.int64)
        drawn.append(p.tolist())
        return p

    km = model.kelpie_model_class()(kd, model, torch.zeros_like(init) if transe else init.clone())
    if transe:
        with torch.no_grad():
            km.kelpie_entity_emb.copy_(init.to(km.kelpie_entity_emb.dtype))
        km.update_embeddings()
    cls = MODEL_REGISTRY["TransE" if transe else "ComplEx"]["optimizer"]
    opt = cls.get_kelpie_class()(model=km, hp=cls.get_hyperparams_class()(**hp), verbose=False)
    inner = opt.step_on_batch

    def step_on_batch(a, b):
        if transe:
            steps.append((np.asarray(a).copy(), np.asarray(b).copy()))
        return inner(a, b)

    opt.step_on_batch = step_on_batch
    torch.randperm = randperm
    ref_harness.seed_all(7)
    try:
        marks = run_with_marks(opt, km, kelpie_pred,
                               lambda: opt.train(training_triples=np.array(kd.kelpie_training_triples)))
    finally:
        torch.randperm = orig
    return marks, drawn, steps


def conve_model(dataset, w, d, rates, dtype):
    from src.link_prediction.models.conve import ConvE, ConvEHyperParams
    model = ConvE(dataset=dataset, hp=ConvEHyperParams(
        dimension=d, input_dropout_rate=rates[0], feature_map_dropout_rate=rates[1], hidden_dropout_rate=rates[2],
        hidden_layer_size=32 * 38 * (d // 20 - 2)))
    with torch.no_grad():
        model.entity_embeddings.data = torch.from_numpy(w["entity_embeddings"].copy()).to(dtype)
        model.relation_embeddings.data = torch.from_numpy(w["relation_embeddings"].copy()).to(dtype)
        model.convolutional_layer.weight.data = torch.from_numpy(w["conv_weight"].copy()).to(dtype)
        model.convolutional_layer.bias.data = torch.from_numpy(w["conv_bias"].copy()).to(dtype)
        model.hidden_layer.weight.data = torch.from_numpy(w["fc_weight"].copy()).to(dtype)
        model.hidden_layer.bias.data = torch.from_numpy(w["fc_bias"].copy()).to(dtype)
        for i, bn in ((1, model.batch_norm_1), (2, model.batch_norm_2), (3, model.batch_norm_3)):
            bn.weight.data = torch.from_numpy(w[f"bn{i}_weight"].copy()).to(dtype)
            bn.bias.data = torch.from_numpy(w[f"bn{i}_bias"].copy()).to(dtype)
            bn.running_mean.data = torch.from_numpy(w[f"bn{i}_mean"].copy()).to(dtype)
            bn.running_var.data = torch.from_numpy(w[f"bn{i}_var"].copy()).to(dtype)
    model.eval()
    return model


class Unfit(Exception):
    """A seed that does not meet the fixture's conditions."""


def summarise(name, kind, runs, filt, kelpie_pred, minimizer, keep_rows):
    """The marks of one post-training from its fp32 and fp64 runs, with the conditions."""
    out = []
    for e, a, b in zip(MARKS, runs["fp32"], runs["fp64"]):
        if abs(a["score"] - b["score"]) > TOL * max(1.0, abs(b["score"])):
            raise Unfit(f"{name} {kind} epoch {e}: fp32 {a['score']} fp64 {b['score']}")
        lo, hi = rank_bounds(b["scores"], b["score"], filt, kelpie_pred[2], minimizer)
        if hi - lo > 1 or not (lo <= a["rank"] <= hi and lo <= b["rank"] <= hi):
            raise Unfit(f"{name} {kind} epoch {e}: ranks {a['rank']} {b['rank']} bounds {lo} {hi}")
        out.append({"epoch": e, "score32": a["score"], "rank32": a["rank"], "score64": b["score"], "rank64": b["rank"],
                    "lo": lo, "hi": hi, "row": b["row"] if keep_rows else None})
    return out


def build_case(dataset, g, spec, seed, pred, other, removed, added):
    from src.data import KelpieDataset
    from src.link_prediction.models.complex import ComplEx, ComplExHyperParams
    from src.link_prediction.models.transe import TransE, TransEHyperParams
    name, family, d, wopt, over, kinds, keep_rows = spec
    transe, conve = family == "TransE", family == "ConvE"
    weights = {"dim": d, "seed": seed, **{k: v for k, v in wopt.items() if k != "rates"}}
    w = synth.make_weights(family, g.num_entities, g.num_relations, d, seed=seed, trained_scale=wopt.get("trained_scale"))
    E, R = w["entity_embeddings"], w["relation_embeddings"]
    init = torch.from_numpy(kelpie_init(family, 2 * d if family == "ComplEx" else d, seed))
    if family == "DistMult":  # the zero-imaginary embedding of the padded tables
        E, R = np.hstack([E, np.zeros_like(E)]), np.hstack([R, np.zeros_like(R)])
        init = torch.cat([init, torch.zeros_like(init)], 1)
    out = {"name": name, "model": family, "weights": weights, "posttrainings": []}
    if conve:
        out["rates"] = list(wopt["rates"])
    mine = [tuple(int(v) for v in t) for t in g.train.tolist() if pred[0] in (t[0], t[2])]
    for kind in kinds:
        entity = other if kind == "sufficient" else pred[0]
        hp = dict(CONVE_HP if conve else TRANSE_HP if transe else dict(NLL_HP, **over))
        runs, perms, masks, steps32, n_removed, max_logit = {}, None, None, None, 0, 0.0
        for variant, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
            torch.set_default_dtype(dtype)
            try:
                kd = KelpieDataset(dataset=dataset, entity=entity)
                if kind == "necessary":
                    kd.remove_training_triples(np.array([removed]))
                elif kind == "sufficient":
                    kd.add_training_triples(np.array([added]))
                if conve:  # as many of the subject's triples removed as gives a last step of one pair
                    for n_removed in range(len(mine)):
                        kd = KelpieDataset(dataset=dataset, entity=entity)
                        if n_removed:
                            kd.remove_training_triples(np.array(mine[:n_removed]))
                        P = len({(int(h), int(r)) for h, r, _ in rows_of(kd, g.num_relations)})
                        bs = next((b for b in range(P // 3, 1, -1) if P % b == 1), None)
                        if bs:
                            break
                    hp["batch_size"] = bs
                rows = rows_of(kd, g.num_relations)
                kelpie = int(kd.kelpie_entity)
                cpred = tuple(other if v == pred[0] and i != 1 else v for i, v in enumerate(pred)) \
                    if kind == "sufficient" else pred
                kp = kelpie_triple(cpred, entity, kelpie)
                filt = [int(v) for v in kd.to_filter.get((kp[0], kp[1]), [])]
                if conve:
                    model = conve_model(dataset, w, d, wopt["rates"], dtype)
                    from src.link_prediction import MODEL_REGISTRY
                    km = model.kelpie_model_class()(kd, model, init.to(dtype).clone())
                    cls = MODEL_REGISTRY["ConvE"]["optimizer"]
                    opt = cls.get_kelpie_class()(model=km, hp=cls.get_hyperparams_class()(**hp), verbose=False)
                    with MaskedDropouts(7, masks) as md:
                        runs[variant] = run_with_marks(
                            opt, km, kp, lambda: opt.train(training_triples=np.array(kd.kelpie_training_triples)))
                        masks = md.masks
                        if variant == "fp64":  # the logits at the last row, every pair, no dropout
                            km.eval()
                            with torch.no_grad():
                                pairs = sorted({(int(h), int(r)) for h, r, _ in rows})
                                p = km.model.all_scores(np.array([[h, r, 0] for h, r in pairs]))
                                max_logit = float(torch.logit(p).abs().max())
                    continue
                if transe:
                    model = TransE(dataset=dataset, hp=TransEHyperParams(dimension=d, norm=wopt["norm"]))
                else:
                    model = ComplEx(dataset=dataset, hp=ComplExHyperParams(dimension=d, init_scale=INIT_SCALE))
                with torch.no_grad():
                    model.entity_embeddings.data = torch.from_numpy(E.copy()).to(dtype)
                    model.relation_embeddings.data = torch.from_numpy(R.copy()).to(dtype)
                model.eval()
                want = STEPS_PER_EPOCH[kind] if len(kinds) > 1 else 3
                hp["batch_size"] = batch_size_for(len(rows), want)
                runs[variant], perms, steps = nll_or_transe(family, model, kd, init.to(dtype), hp, perms, kp)
                if variant == "fp32":
                    steps32 = steps
                elif transe:  # both runs stepped on the same batches
                    assert all(np.array_equal(p, q) and np.array_equal(m, n) for (p, m), (q, n) in zip(steps32, steps))
            finally:
                torch.set_default_dtype(torch.float32)
        pt = {"kind": kind, "rows": rows.tolist(), "kelpie": kelpie, "hp": hp, "pred": list(kp), "filter": filt}
        if conve:
            if max_logit >= LOGIT_BOUND:
                raise Unfit(f"{name}: logit {max_logit}")
            P, bs = len({(int(h), int(r)) for h, r, _ in rows}), hp["batch_size"]
            assert P % bs == 1 and (P + bs - 1) // bs >= 3
            pt.update(removed=[list(t) for t in mine[:n_removed]], pairs=P, max_logit=max_logit, rng=pack_masks(masks))
        elif transe:
            per_epoch = (len(rows) + hp["batch_size"] - 1) // hp["batch_size"]
            assert len(steps32) == EPOCHS * per_epoch
            pt["rng"] = [transe_draws(rows, hp["negative_triples_ratio"], steps32[e * per_epoch:(e + 1) * per_epoch])
                         for e in range(EPOCHS)]
        else:
            assert len(perms) == EPOCHS
            pt["perms"] = perms
        pt["marks"] = summarise(name, kind, runs, filt, kp, transe, keep_rows)
        out["posttrainings"].append(pt)
    flat = [m for pt in out["posttrainings"] for m in pt["marks"]]
    if 4 * sum(int(m["lo"] == m["hi"]) for m in flat) < 3 * len(flat):
        raise Unfit(f"{name}: {sum(int(m['lo'] == m['hi']) for m in flat)} of {len(flat)} marks are sharp")
    if not any(len({m["rank64"] for m in pt["marks"]}) > 1 and len({m["rank32"] for m in pt["marks"]}) > 1
               for pt in out["posttrainings"]):
        raise Unfit(f"{name}: the marks do not move")
    return out


def main():
    if not os.path.isdir(os.path.join(ref_harness.REF_ROOT, "src")):
        print("reference absent: nothing written")
        return
    ref_harness.load_reference()
    torch.set_num_threads(2)
    from src.data import Dataset

    g = synth.make_graph(GRAPH["shape"], seed=GRAPH["seed"])
    ref_harness.register_dataset("marks_tiny", g.num_entities, g.num_relations, g.train, g.valid, g.test)
    dataset = Dataset("marks_tiny")
    deg = {}
    for h, _, t in g.train.tolist():
        deg[h] = deg.get(h, 0) + 1
        deg[t] = deg.get(t, 0) + 1
    pred = next(tuple(int(v) for v in t) for t in g.test.tolist() if 12 <= deg.get(t[0], 0) <= 30)
    other = next(e for e in range(g.num_entities) if e != pred[0] and 8 <= deg.get(e, 0) <= 20)
    removed = tuple(int(v) for v in next(t for t in g.train.tolist() if pred[0] in (t[0], t[2])))
    added = tuple(other if v == pred[0] else int(v) for v in removed)
    added = (added[0], removed[1], added[2])
    rec = {"graph": GRAPH, "init_scale": INIT_SCALE, "epochs": EPOCHS, "marks": MARKS, "pred": list(pred),
           "other": int(other), "removed": list(removed), "added": list(added), "tol": TOL, "cases": []}
    for spec in CASES:
        for seed in SEEDS:
            try:
                out = build_case(dataset, g, spec, seed, pred, other, removed, added)
            except Unfit as why:
                print("  seed", seed, "unfit:", why)
                continue
            break
        else:
            raise SystemExit(f"{spec[0]}: no seed of {SEEDS} meets the conditions")
        rec["cases"].append(out)
        for pt in out["posttrainings"]:
            print(spec[0], pt["kind"], "seed", seed, "rows", len(pt["rows"]), "batch", pt["hp"]["batch_size"], "ranks",
                  [m["rank64"] for m in pt["marks"]], "sharp", sum(m["lo"] == m["hi"] for m in pt["marks"]))
    with open(OUT, "w") as f:  # one line per post-training
        text = json.dumps(rec, separators=(",", ":"))
        f.write(text.replace('{"kind"', '\n{"kind"').replace('"cases"', '\n"cases"') + "\n")


if __name__ == "__main__":
    main()
