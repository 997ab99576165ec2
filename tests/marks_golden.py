"""The marks fixture's post-trainings as models and batches (TEST INFRASTRUCTURE):
tests/golden/marks_golden.json (made by tests/golden/make_marks_golden.py inside one reference
run per post-training) on the seeded tables it was recorded on, shared by test_marks_cpu.py
and test_marks_gpu.py."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import kelpie_amd as ka
from kelpie_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marks_golden.json")
TOL = 1e-4


@functools.lru_cache(maxsize=1)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=1)
def dataset():
    g = golden()["graph"]
    g = synth.make_graph(g["shape"], seed=g["seed"])
    return g, ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)


def posttrainings():
    """Every recorded post-training: (id, case, post-training)."""
    return [(f'{c["name"]}-{p["kind"]}', c, p) for c in golden()["cases"] for p in c["posttrainings"]]


def make_model(case):
    """A fresh ka model on the case's seeded tables."""
    g, ds = dataset()
    w, fam = case["weights"], case["model"]
    t = synth.make_weights(fam, g.num_entities, g.num_relations, w["dim"], seed=w["seed"],
                           trained_scale=w.get("trained_scale"))
    E, R = t["entity_embeddings"], t["relation_embeddings"]
    if fam == "ComplEx":
        return ka.ComplEx(ds, E, R, init_scale=golden()["init_scale"])
    if fam == "DistMult":
        return ka.DistMult(ds, E, R, init_scale=golden()["init_scale"])
    if fam == "TransE":
        return ka.TransE(ds, E, R, norm=w["norm"])
    bn = {i: {"weight": t[f"bn{i}_weight"], "bias": t[f"bn{i}_bias"], "running_mean": t[f"bn{i}_mean"],
              "running_var": t[f"bn{i}_var"]} for i in (1, 2, 3)}
    rates = case["rates"]
    return ka.ConvE(ds, E, R, t["conv_weight"].reshape(32, 3, 3), t["conv_bias"], t["fc_weight"], t["fc_bias"], bn=bn,
                    input_dropout_rate=rates[0], feature_map_dropout_rate=rates[1], hidden_dropout_rate=rates[2])


def x0(case):
    """The kelpie row the case's post-trainings start from, float32 [width]: the generator's seeded
    init (make_trace_golden.kelpie_init), ComplEx / DistMult scaled by init_scale as the model does."""
    fam, d, seed = case["model"], case["weights"]["dim"], case["weights"]["seed"]
    rng = np.random.default_rng(1000 + seed)
    if fam == "TransE":
        return (rng.standard_normal((1, d)) * np.sqrt(2.0 / (1 + d))).astype(np.float32)[0]
    raw = rng.random((1, 2 * d if fam == "ComplEx" else d), dtype=np.float32)[0]
    if fam == "ConvE":
        return raw
    return (raw * np.float32(golden()["init_scale"])).astype(np.float32)


def batch(model, case, pt):
    """posttrain_rank's arguments for one recorded post-training: one slot."""
    rows = np.asarray(pt["rows"], np.int32)
    if case["model"] == "ConvE":
        draws = np.asarray(pt["rng"] or [0], np.int32)
    elif case["model"] == "TransE":
        draws = np.concatenate(pt["rng"]).astype(np.int32)
    else:
        draws = np.concatenate(pt["perms"]).astype(np.int32)
    filt = np.asarray(pt["filter"] or [0], np.int32)
    return (model.kp_hp(pt["hp"]), x0(case)[None], np.array([0, len(rows)], np.int32), rows,
            np.array([0, len(draws)], np.int64), draws, np.array([pt["pred"]], np.int32),
            np.array([0, len(pt["filter"])], np.int32), filt)


def row_error(pt, rows):
    """The largest error of the mark rows against the recorded fp64 rows, relative to the fp64
    row's largest magnitude (0.0 for a post-training recorded without rows)."""
    worst = 0.0
    for j, m in enumerate(pt["marks"]):
        if m["row"] is not None:
            ref = np.asarray(m["row"])[:rows.shape[1]]
            worst = max(worst, float(np.abs(rows[j] - ref).max() / np.abs(ref).max()))
    return worst


def check(pid, pt, scores, ranks, rows=None):
    """One post-training's marks against the fixture: every score within 1e-4 * max(1, |s64|)
    of the reference's fp64 run, every rank inside the rank rule's bounds; ``rows``: each within
    1e-4 of the recorded fp64 row's largest magnitude.  Returns the ranks equal to the fp64 run's."""
    marks = pt["marks"]
    assert len(scores) == len(ranks) == len(marks)
    exact = 0
    for j, m in enumerate(marks):
        assert abs(float(scores[j]) - m["score64"]) <= TOL * max(1.0, abs(m["score64"])), (pid, m["epoch"], scores[j], m)
        assert m["lo"] <= int(ranks[j]) <= m["hi"], (pid, m["epoch"], int(ranks[j]), m["lo"], m["hi"])
        if rows is not None and m["row"] is not None:
            ref = np.asarray(m["row"])[:rows.shape[1]]
            assert np.abs(rows[j] - ref).max() <= TOL * np.abs(ref).max(), (pid, m["epoch"])
        exact += int(int(ranks[j]) == m["rank64"])
    return exact
