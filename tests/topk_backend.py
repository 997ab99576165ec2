"""Top-k tails on the CPU (TEST INFRASTRUCTURE).

``reference_topk`` is the test-side definition of kp_posttrain_rank_topk's lists: one row
of scores over the columns 0 .. n_ent (the kelpie entity last), masked as
get_triple_results masks it (post_training_engine.py:101-125: every filtered column left
out, a minimizer's ranked object restored) and stable-sorted, better first.

``TopkContext`` wraps one of the existing stand-in contexts (cpu_backend.py,
distmult_backend.py), which know nothing of lists, so that it accepts
``posttrain_rank(..., topk=k)``: the lists come from the oracle's
``all_scores([kelpie_triple], kelpie_row=x)`` on the slot's final row.
"""
from __future__ import annotations

import numpy as np


def masked_columns(n_cols, filt, obj, minimizer):
    """Boolean mask [n_cols] of the columns the lists leave out."""
    m = np.zeros(n_cols, bool)
    f = np.asarray(filt, np.int64)
    m[f[(f >= 0) & (f < n_cols)]] = True
    if minimizer:
        m[int(obj)] = False
    return m


def reference_topk(row, filt, obj, k, minimizer):
    """(ids int32 [k], values [k]) of one row: -1 / 0 past the last unmasked column."""
    row = np.asarray(row)
    masked = masked_columns(len(row), filt, obj, minimizer)
    order = np.argsort(row if minimizer else -row.astype(np.float64), kind="stable")
    keep = [int(e) for e in order if not masked[e]][:k]
    ids = np.full(k, -1, np.int32)
    vals = np.zeros(k, np.float64)
    ids[:len(keep)] = keep
    vals[:len(keep)] = row[keep]
    return ids, vals


def oracle_row(ctx, kelpie_triple, x):
    """The oracle's scores of (kelpie, p, .) over [E; x] through a stand-in context."""
    if hasattr(ctx, "d"):  # DistMultOracleContext: ComplEx on zero-imaginary rows
        from distmult_backend import zero_imaginary
        return ctx.inner.om.all_scores([kelpie_triple], kelpie_row=zero_imaginary(x))[0]
    inner = getattr(ctx, "inner", ctx)
    return inner.om.all_scores([kelpie_triple], kelpie_row=np.asarray(x, np.float32))[0]


class TopkContext:
    """A stand-in context that also serves ``topk``; ``topk_calls`` records every k it was
    asked for (0 included), in call order."""

    def __init__(self, ctx, minimizer):
        self._ctx = ctx
        self._minimizer = bool(minimizer)
        self.topk_calls = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, topk=0):
        self.topk_calls.append(int(topk))
        s, r, x = self._ctx.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=True)
        if not topk:
            return s, r, (x if want_x else None)
        n = len(s)
        ids = np.full((n, topk), -1, np.int32)
        top = np.zeros((n, topk), np.float32)
        for i in range(n):
            kp = tuple(int(v) for v in pred[i])
            row = oracle_row(self._ctx, kp, x[i])
            ids[i], vals = reference_topk(row, filt[filt_off[i]:filt_off[i + 1]], kp[2], topk, self._minimizer)
            top[i] = vals
        return s, r, (x if want_x else None), (ids, top)


def wrap(model):
    """Give ``model`` (with a stand-in context already set) a list-serving context."""
    model._ctx = TopkContext(model._ctx, model.is_minimizer())
    return model._ctx
