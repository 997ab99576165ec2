"""Top-k tails on the device (kp_posttrain_rank_topk) against the CPU.

1. planted: epochs = 0, so the row stays x0 and the CPU knows the query; integer-valued
   tables make every fp64 score exact on both sides (equal scores are exact ties), and the
   ids must equal the CPU's in order;
2. after real post-training (topk_cases.py): the oracle's score row on the slot's
   downloaded final row, within width_cases.TOL position by position;
3. the lists change nothing else, and repeat bit for bit;
4. error paths leave the context usable;
5. the pipelines end to end.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kelpie_amd as ka
import topk_cases as tc
import width_cases as wc
from golden_io import seed_all
from kelpie_amd import _lib, synth
from kelpie_amd.pipeline import build_pipeline, explain_preds, read_preds
from topk_backend import reference_topk

pytestmark = pytest.mark.gpu

N_REL = 3
FAMILIES = ["ComplEx", "DistMult", "TransE-L2", "TransE-L1"]


# ----------------------------------------------------------------------------- 1. planted
def _dataset(n_ent):
    rng = np.random.default_rng(n_ent)
    t = np.stack([rng.integers(0, n_ent, 60), rng.integers(0, N_REL, 60), rng.integers(0, n_ent, 60)], 1)
    return ka.Dataset(n_ent, N_REL, t[:40], t[40:50], t[50:])


def _rows64(family, E, R, x0, rels):
    """fp64 values of (kelpie, p_s, .) over [E; x0_s] per slot, as the rank path orders them:
    dot products, squared L2 or L1 distances."""
    E, R, x0 = E.astype(np.float64), R.astype(np.float64), x0.astype(np.float64)
    out = []
    for s, p in enumerate(rels):
        cols = np.vstack([E, x0[s][None]])
        x, r = x0[s], R[p]
        if family == "ComplEx":
            h = len(x) // 2
            q = np.concatenate([x[:h] * r[:h] - x[h:] * r[h:], x[:h] * r[h:] + x[h:] * r[:h]])
            out.append(cols @ q)
        elif family == "DistMult":
            out.append(cols @ (x * r))
        elif family == "TransE-L2":
            out.append((((x + r)[None] - cols) ** 2).sum(1))
        else:
            out.append(np.abs((x + r)[None] - cols).sum(1))
    return out


def planted(family, n_ent, n_slots):
    """Integer tables, x0 and ranked triples of ``n_slots`` slots with the edge cases planted
    (module docstring); returns the model, the batch arguments and, per slot, its fp64 row,
    filter and object."""
    rng = np.random.default_rng(7 * n_ent + len(family))
    minimizer = family.startswith("TransE")
    width = 16 if minimizer else 12
    E = rng.integers(-3, 4, (n_ent, width)).astype(np.float32)
    R = rng.integers(-2, 3, (2 * N_REL, width)).astype(np.float32)
    x0 = rng.integers(-3, 4, (n_slots, width)).astype(np.float32)
    rels = rng.integers(0, 2 * N_REL, n_slots)
    objs = rng.integers(0, n_ent, n_slots)
    twin = n_ent - 3
    # slot 0: two identical entity rows that are the best columns (a tie: 7 before `twin`)
    if minimizer:
        E[7] = E[twin] = x0[0] + R[rels[0]]
    else:
        x, r = x0[0], R[rels[0]]
        if family == "ComplEx":
            h = width // 2
            q = np.concatenate([x[:h] * r[:h] - x[h:] * r[h:], x[:h] * r[h:] + x[h:] * r[:h]])
        else:
            q = x * r
        E[7] = E[twin] = 3 * np.where(q >= 0, 1, -1)
    rows = _rows64(family, E, R, x0, rels)
    best = [reference_topk(rows[s], [], 0, 3, minimizer)[0] for s in range(n_slots)]
    frozen_best = [[int(e) for e in reference_topk(rows[s][:n_ent], [], 0, 3, minimizer)[0]] for s in range(n_slots)]
    filts = [list(rng.integers(0, n_ent, rng.integers(0, 6))) for _ in range(n_slots)]
    filts[0] = []
    filts[1] = [int(best[1][0])]                                  # the column that would be first
    a, b = frozen_best[2][0], frozen_best[2][1]
    filts[2] = [a, a, b, a]                                       # duplicates
    objs[3] = frozen_best[3][1]
    filts[3] = [int(objs[3]), frozen_best[3][2]]                  # o filtered: absent / restored (TransE)
    objs[4], filts[4] = n_ent, []                                 # o is the kelpie column
    filts[5] = [n_ent, frozen_best[5][0]]                         # the kelpie column filtered
    objs[6], filts[6] = n_ent, [n_ent]                            # both: restored for TransE only
    ds = _dataset(n_ent)
    if family == "ComplEx":
        model = ka.ComplEx(ds, E, R)
        hp = dict(wc.CX_HP, epochs=0)
    elif family == "DistMult":
        model = ka.DistMult(ds, E, R)
        hp = dict(wc.CX_HP, epochs=0)
    else:
        model = ka.TransE(ds, E, R, norm=2 if family == "TransE-L2" else 1)
        hp = dict(wc.TE_HP, epochs=0)
    # two rows per slot (a kelpie triple and its inverse); with no epoch they are never stepped
    one = np.array([[n_ent, 0, 1], [1, N_REL, n_ent]], np.int64)
    row_off = 2 * np.arange(n_slots + 1)
    pred = np.stack([np.full(n_slots, n_ent), rels, objs], 1)
    filt_off = np.concatenate([[0], np.cumsum([len(f) for f in filts])])
    filt = np.array([e for f in filts for e in f] or [0], np.int64)
    args = (model.kp_hp(hp), x0, row_off, np.vstack([one] * n_slots), np.zeros(n_slots + 1, np.int64),
            np.zeros(1, np.int32), pred, filt_off, filt)
    return model, args, rows, filts, [int(o) for o in objs], minimizer


def _expected_score(family, v):
    return np.sqrt(v) if family == "TransE-L2" else v


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n_ent,n_slots,ks", [(517, 17, (1, 32)), (20, 7, (32, 5))],
                         ids=["n517-17slots", "n20-padding"])
def test_planted_exact_ids(family, n_ent, n_slots, ks):
    model, args, rows, filts, objs, minimizer = planted(family, n_ent, n_slots)
    s0, r0, x = model.ctx.posttrain_rank(*args, want_x=True)
    assert np.array_equal(x, args[1])  # no epoch: the rows are x0
    for k in ks:
        s, r, _, (ids, top) = model.ctx.posttrain_rank(*args, topk=k)
        assert np.array_equal(s, s0) and np.array_equal(r, r0)
        for i in range(n_slots):
            exp_ids, exp_vals = reference_topk(rows[i], filts[i], objs[i], k, minimizer)
            print(family, n_ent, k, i, ids[i].tolist(), exp_ids.tolist())
            assert ids[i].tolist() == exp_ids.tolist(), (family, k, i, filts[i], objs[i])
            want = _expected_score(family, exp_vals).astype(np.float32)
            assert np.allclose(top[i], want, rtol=1e-6, atol=0), (family, k, i, top[i], want)
            # the rank invariant
            o_masked = objs[i] in filts[i] and not minimizer
            if not o_masked and r[i] <= k:
                assert objs[i] in ids[i, :r[i]].tolist(), (family, k, i, objs[i], int(r[i]), ids[i])
    # what the plants are for (k = 32 is in both parameter sets)
    ids = model.ctx.posttrain_rank(*args, topk=32)[3][0]
    twin = n_ent - 3
    assert ids[0, :2].tolist() == [7, twin]                      # the tie: lower id first
    first = reference_topk(rows[1], [], 0, 1, minimizer)[0][0]
    assert first == filts[1][0] and first not in ids[1]          # the would-be first column is filtered
    assert filts[2][0] not in ids[2] and filts[2][2] not in ids[2]
    assert (objs[3] in ids[3]) == minimizer                      # o filtered: restored for TransE only
    assert (n_ent in ids[6]) == minimizer
    assert n_ent not in ids[5]
    if n_ent == 20:
        n_un = [n_ent + 1 - len(set(f) - ({objs[i]} if minimizer else set())) for i, f in enumerate(filts)]
        for i in range(n_slots):
            assert (ids[i, :n_un[i]] >= 0).all() and (ids[i, n_un[i]:] == -1).all(), (i, ids[i], n_un[i])
        assert n_ent in ids[4]                                   # the kelpie column takes part


# ----------------------------------------------------------------------------- 2. after real post-training
@pytest.mark.parametrize("case", tc.CASES, ids=wc.ids(tc.CASES))
def test_lists_after_posttraining(case):
    slots, model = tc.run(case, lambda m: m.ctx)
    assert len(slots) == 6
    for s in slots:
        print(case["id"], s["pred"], s["rank"], s["ids"].tolist(), s["top"].tolist())
    near, far = tc.check_lists(slots, model, wc.oracle_context(model))
    assert near >= 1 and far >= 1, (near, far, [s["rank"] for s in slots])


# ----------------------------------------------------------------------------- 3. non-interference
def _query_case(family):
    m, d = {"ComplEx": ("ComplEx", 12), "DistMult": ("DistMult", 40), "ConvE": ("ConvE", 60), "TransE": ("TransE", 50)}[family]
    return dict(wc._case(m, d, tag="nq65"), nq=65)


@pytest.mark.parametrize("family", ["ComplEx", "DistMult", "ConvE", "TransE"])
def test_lists_change_nothing_and_repeat(family):
    case = _query_case(family)
    model = wc.make_model(case)
    args = wc.query_batch(case, model)
    s0, r0, x0 = model.ctx.posttrain_rank(*args, want_x=True)
    s5, r5, x5, (ids_a, top_a) = model.ctx.posttrain_rank(*args, want_x=True, topk=5)
    _, _, _, (ids_b, top_b) = model.ctx.posttrain_rank(*args, want_x=True, topk=5)
    assert x0.tobytes() == x5.tobytes() and s0.tobytes() == s5.tobytes() and r0.tobytes() == r5.tobytes()
    assert ids_a.tobytes() == ids_b.tobytes() and top_a.tobytes() == top_b.tobytes()
    assert (ids_a >= 0).all()
    # and back: a call without lists after one with lists
    s1, r1, x1 = model.ctx.posttrain_rank(*args, want_x=True)
    assert x0.tobytes() == x1.tobytes() and s0.tobytes() == s1.tobytes() and r0.tobytes() == r1.tobytes()


# ----------------------------------------------------------------------------- 4. error paths
def _raw_call(ctx, args, k, ids, top):
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = args
    n = len(row_off) - 1
    keep = [np.ascontiguousarray(x0, np.float32), np.ascontiguousarray(row_off, np.int32),
            np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(rng_off, np.int64),
            np.ascontiguousarray(rng, np.int32), np.ascontiguousarray(pred, np.int32),
            np.ascontiguousarray(filt_off, np.int32), np.ascontiguousarray(filt, np.int32),
            np.zeros(n, np.float32), np.zeros(n, np.int64)]
    p = [_lib._ptr(a) for a in keep]
    b = _lib.Batch(n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], None, p[8], p[9])
    return _lib.lib().kp_posttrain_rank_topk(ctx.h, C.byref(hp), C.byref(b), k, _lib._ptr(ids), _lib._ptr(top))


def test_bad_k_and_null_outputs_leave_the_context_usable():
    model, args, rows, filts, objs, minimizer = planted("DistMult", 20, 7)
    ctx = model.ctx
    good = ctx.posttrain_rank(*args, topk=4)
    ids, top = np.zeros((7, 33), np.int32), np.zeros((7, 33), np.float32)
    EINVAL = -22
    assert _raw_call(ctx, args, 33, ids, top) == EINVAL
    assert _raw_call(ctx, args, -1, ids, top) == EINVAL
    assert _raw_call(ctx, args, 4, None, top) == EINVAL
    assert _raw_call(ctx, args, 4, ids, None) == EINVAL
    assert not ids.any() and not top.any()
    assert b"top-k" in _lib.lib().kp_last_error(ctx.h)
    assert _raw_call(ctx, args, 0, None, None) == 0  # k == 0 with null outputs: kp_posttrain_rank
    again = ctx.posttrain_rank(*args, topk=4)
    for a, b in zip(good[:2] + good[3], again[:2] + again[3]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("family,var", [("TransE", "KP_TE_RANK"), ("ConvE", "KP_CV_RANK")])
def test_fp32_rank_switch_refuses_lists(family, var, monkeypatch):
    monkeypatch.setenv(var, "f32")  # read when the context is created
    case = _query_case(family)
    model = wc.make_model(case)
    args = wc.query_batch(case, model)
    ctx = model.ctx
    monkeypatch.delenv(var)
    with pytest.raises(_lib.KelpieHipError, match="-95"):
        ctx.posttrain_rank(*args, topk=3)
    s, r, _ = ctx.posttrain_rank(*args)  # the fp32 rank itself still runs
    assert len(s) == len(r) == len(args[2]) - 1 and (r >= 1).all()


# ----------------------------------------------------------------------------- 5. end to end
def _supported_graph():
    """The tiny synthetic graph with one planted fact: the subject's only fact about ``o``,
    (s, p', o), under a relation p' whose embedding equals that of the predicted relation p."""
    g = synth.make_graph("tiny", seed=11, n_ent=64, n_rel=6, n_train=360, n_valid=40, n_test=40)
    train = [tuple(int(v) for v in t) for t in g.train]
    deg = {}
    for h, _, t in train:
        deg[h] = deg.get(h, 0) + 1
        deg[t] = deg.get(t, 0) + 1
    s = min((e for e in deg if 4 <= deg[e] <= 8), key=lambda e: (deg[e], e))
    p, p2 = 0, 1
    touched = {h for h, _, t in train if t == s} | {t for h, _, t in train if h == s}
    o = next(e for e in range(g.num_entities) if e != s and e not in touched and deg.get(e, 0) >= 1)
    support = (s, p2, o)
    train = [t for t in train if not (t[0] == s and t[1] in (p, p2))] + [support]
    test = [tuple(int(v) for v in t) for t in g.test if not (t[0] == s and t[1] == p)] + [(s, p, o)]
    ds = ka.Dataset(g.num_entities, g.num_relations, np.array(train), g.valid, np.array(test))
    rng = np.random.default_rng(5)
    d = 16
    E = rng.standard_normal((g.num_entities, d)).astype(np.float32)
    R = (0.5 * rng.standard_normal((2 * g.num_relations, d))).astype(np.float32)
    R[p2] = R[p]
    R[p2 + g.num_relations] = R[p + g.num_relations]
    return ds, E, R, (s, p, o), support


E2E_HP = {"batch_size": 2048, "epochs": 40, "lr": 0.1, "margin": 5, "negative_triples_ratio": 5,
          "regularizer_weight": 0.0}


def test_removing_the_only_support(tmp_path):
    ds, E, R, pred, support = _supported_graph()
    model = ka.TransE(ds, E, R)
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, E2E_HP)
    out = eng.compute_counterfactuals(pred, [[support]], 3)[0]
    print("base", out["base"], "post", out["post"])
    assert len(out["post"]["top"]) == 3 and len(out["base"]["top"]) == 3
    K, o = ds.num_entities, pred[2]
    # with the fact the model answers o (after the kelpie entity itself, a translation away
    # from its own row); without it o is gone from the list
    assert [e for e, _ in out["base"]["top"] if e != K][0] == o
    assert out["post"]["top"][0][0] != o and o not in [e for e, _ in out["post"]["top"]]
    assert out["post"]["rank"] > out["base"]["rank"]


@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
def test_pipeline_end_to_end(mode, tmp_path):
    ds, E, R, pred, support = _supported_graph()
    model = ka.TransE(ds, E, R)
    preds_path = os.path.join(tmp_path, "preds.csv")
    with open(preds_path, "w") as f:
        f.write("\t".join(ds.labels_triple(pred)) + "\n")
    seed_all(42)
    pipe = build_pipeline(model, ds, dict(E2E_HP, epochs=10), mode, xsi=1e9 if mode == "necessary" else None, top_k=3)
    pipe.builder.length_cap = 1  # singleton rules only: the record's first rules are the first singletons
    out_path = os.path.join(tmp_path, "output.json")
    explain_preds(pipe, ds, read_preds(preds_path), prefilter_k=4, output_path=out_path)
    with open(out_path) as f:
        rec = json.load(f)[0]
    assert len(rec["counterfactuals"]) == len(rec["rule_to_relevance"]) >= 1
    labels = set(ds.entity_to_id)
    for cf in rec["counterfactuals"]:
        pairs = [cf] if mode == "necessary" else cf
        if mode == "sufficient":
            assert [c["entity"] for c in cf] == rec["entities_to_convert"]
        for c in pairs:
            cloned = ds.id_to_entity[pred[0]] if mode == "necessary" else c["entity"]
            assert len(c["post"]) == 3
            for lab, score in c["post"] + (c["base"] or []):
                assert (lab in labels or lab == "kelpie:" + cloned) and score >= 0.0
            sc = [v for _, v in c["post"]]
            assert sc == sorted(sc)  # distances, best first
    if mode == "necessary":
        # the first singleton: the planted fact is the subject's only fact about o
        rules = [[tuple(ds.ids_triple(t)) for t in rule] for rule, _ in rec["rule_to_relevance"]]
        assert [support] in rules
        cf = rec["counterfactuals"][rules.index([support])]
        assert cf["post"][0][0] != ds.id_to_entity[pred[2]]
