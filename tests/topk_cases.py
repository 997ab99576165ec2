"""The post-trained top-k cases (TEST INFRASTRUCTURE), shared by test_topk_gpu.py and its
CPU companion in test_topk_cases_cpu.py.

One case per model family at its smallest compiled width (width_cases.py; ConvE at d = 60),
8 epochs, on the 517-entity graph: two subjects with two singleton candidates each, six
post-trainings.  The first subject ranks its test triple's object, which sits mid-table
(rank in the hundreds: far past any list).  For the second the ranked object is replaced by
``NEAR_OBJECT[case id]``: an entity near the head of the subject's post-trained row, so
that its rank is within the list.  The post-trained rows do not depend on the ranked object
(no family draws from it), so the oracle alone fixes these picks on the CPU, and
test_topk_cases_cpu.py holds them to it: per family at least one slot with rank <= K and
one with rank > K.
"""
from __future__ import annotations

import numpy as np

import kelpie_amd as ka
import width_cases as wc
from golden_io import seed_all
from topk_backend import masked_columns, oracle_row, reference_topk

K = 10

CASES = [wc._case("ComplEx", 3, seed=8), wc._case("DistMult", 40, seed=4), wc._case("ConvE", 60, seed=4),
         wc._case("TransE", 50, seed=4)]

# the ranked object of the second subject: the third best unfiltered tail of the oracle's
# post-trained base row (tools: print(topk_cases.pick_near_objects()))
NEAR_OBJECT = {"ComplEx-d3-DB1": 514, "DistMult-d40-DB4": 17, "ConvE-d60-DB4": 191, "TransE-d50-VPL1-NT1024": 344}


def predictions(case, near=True):
    """[(pred, candidates)] of the case's two subjects."""
    ds, ordinary = wc.graph(case["n_ent"])[1], wc.graph(case["n_ent"])[2]
    out = []
    for i, pred in enumerate(ordinary[:2]):
        if i == 1 and near:
            pred = (pred[0], pred[1], NEAR_OBJECT[case["id"]])
        out.append((pred, sorted(ds.entity_to_training_triples[pred[0]])[:2]))
    return out


class ListRecorder:
    """Wraps a context that serves ``topk`` and records every post-trained slot in call
    order: ranked triple, filter, score, rank, final row and its list."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.slots = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, topk=0):
        s, r, x, (ids, top) = self._ctx.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt,
                                                       want_x=True, topk=topk)
        for i in range(len(s)):
            self.slots.append({"pred": tuple(int(v) for v in pred[i]), "score": float(s[i]), "rank": int(r[i]),
                               "filt": np.asarray(filt[filt_off[i]:filt_off[i + 1]], np.int64).copy(),
                               "x": np.array(x[i]), "ids": np.array(ids[i]), "top": np.array(top[i])})
        return s, r, (x if want_x else None), (ids, top)


def run(case, ctx_of, k=K, near=True):
    """The case's necessary-mode batches with ``top_k`` = k through ``ctx_of(model)``; the
    recorded slots and the model."""
    ds = wc.graph(case["n_ent"])[1]
    model = wc.make_model(case)
    model._ctx = ListRecorder(ctx_of(model))
    seed_all(42)
    for pred, cands in predictions(case, near):
        eng = ka.NecessaryPostTrainingEngine(model, ds, wc.hp_of(case))
        eng.top_k = k
        eng.compute_relevance_batch(pred, [[c] for c in cands])
    return model.ctx.slots, model


def oracle_ctx(model):
    """The family's oracle-backed stand-in, wrapped to serve lists."""
    from topk_backend import TopkContext
    return TopkContext(wc.oracle_context(model), model.is_minimizer())


def pick_near_objects():
    """How NEAR_OBJECT was chosen: per case, the third best unfiltered frozen tail of the
    second subject's post-trained base row, by the oracle."""
    out = {}
    for case in CASES:
        slots, model = run(case, oracle_ctx, near=False)
        base = slots[3]  # the second subject's batch: base, then its two candidates
        ids, _ = reference_topk(oracle_row(model.ctx, base["pred"], base["x"]), base["filt"], base["pred"][2], 8,
                                model.is_minimizer())
        out[case["id"]] = int([e for e in ids if e != model.dataset.num_entities][2])
    return out


def check_lists(slots, model, ref_ctx, k=K):
    """Every recorded slot's list against the oracle's score row on the slot's own final
    row (``ref_ctx``: the family's stand-in context), masked and stable-sorted:

    * no position skipped: the list is as long as min(k, unmasked columns), -1 / 0 after;
    * at every position the listed id's oracle score is within TOL * max(1, |score|) of the
      oracle's score at that position;
    * ids distinct, none masked, the list's own scores monotone;
    * the rank invariant: an unmasked target of rank <= k is among the first `rank` ids.

    Returns (slots with rank <= k, slots with rank > k)."""
    minimizer = model.is_minimizer()
    n_cols = model.dataset.num_entities + 1
    near = far = 0
    for i, s in enumerate(slots):
        o = s["pred"][2]
        row = np.asarray(oracle_row(ref_ctx, s["pred"], s["x"]), np.float64)
        masked = masked_columns(n_cols, s["filt"], o, minimizer)
        ref_ids, ref_vals = reference_topk(row, s["filt"], o, k, minimizer)
        n = int(min(k, n_cols - masked.sum()))
        ids, top = s["ids"], s["top"]
        assert (ids[:n] >= 0).all() and (ids[n:] == -1).all() and not top[n:].any(), (i, ids, n)
        assert len(set(ids[:n].tolist())) == n, (i, ids)
        assert not masked[ids[:n]].any(), (i, ids)
        d = np.diff(top[:n].astype(np.float64))
        assert (d >= 0).all() if minimizer else (d <= 0).all(), (i, top)
        for j in range(n):
            tol = wc.TOL * max(1.0, abs(ref_vals[j]))
            assert abs(row[ids[j]] - ref_vals[j]) <= tol, (i, j, int(ids[j]), row[ids[j]], int(ref_ids[j]), ref_vals[j])
            assert abs(float(top[j]) - ref_vals[j]) <= tol, (i, j, float(top[j]), ref_vals[j])
        if s["rank"] <= k:
            near += 1
            if not masked[o]:
                assert o in ids[:s["rank"]].tolist(), (i, o, s["rank"], ids)
        else:
            far += 1
    return near, far
