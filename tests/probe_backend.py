"""Probes on the CPU (TEST INFRASTRUCTURE).

``triple_results`` is the test-side restatement of get_triple_results
(post_training_engine.py:101-125) on one row of scores over the columns 0 .. n_ent (the
kelpie entity last): the definition of what kp_posttrain_rank_probes returns per probe.

``ProbeContext`` wraps one of the existing stand-in contexts (cpu_backend.py,
distmult_backend.py, topk_backend.TopkContext), which know nothing of probes, so that it
accepts ``posttrain_rank(..., probes=(probe_off, probes, filt_off, filt))``: a probe's row
comes from the oracle's ``all_scores([kelpie_triple], kelpie_row=x)`` on its slot's final row.
"""
from __future__ import annotations

import numpy as np

from topk_backend import oracle_row


def triple_results(row, filt, obj, minimizer):
    """(target score, target rank) of get_triple_results on ``row`` (not modified)."""
    row = np.array(row, copy=True)
    target = row[int(obj)]
    f = np.asarray(filt, np.int64)
    f = f[(f >= 0) & (f < len(row))]
    if minimizer:
        row[f] = 1e6
        row[int(obj)] = target
        return float(target), int((row <= target).sum())
    row[f] = -1e6
    return float(target), int((row >= target).sum())


class ProbeContext:
    """A stand-in context that also serves ``probes``; ``probe_calls`` records the probe
    count of every call (0 without probes), ``slots`` every slot's final row with its
    probes' results, in call order."""

    def __init__(self, ctx, minimizer):
        self._ctx = ctx
        self._minimizer = bool(minimizer)
        self.probe_calls = []
        self.slots = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, topk=0,
                       probes=None):
        kw = {"topk": topk} if topk else {}
        out = self._ctx.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=True, **kw)
        s, r, x = out[:3]
        ret = (s, r, (x if want_x else None)) + tuple(out[3:])
        self.probe_calls.append(0 if probes is None else len(np.asarray(probes[1]).reshape(-1, 2)))
        if probes is None:
            return ret
        p_off, p_tr, pf_off, pf = probes
        p_tr = np.asarray(p_tr, np.int64).reshape(-1, 2)
        n, n_ent = len(s), int(pred[0][0])
        assert len(p_off) == n + 1 and p_off[0] == 0 and p_off[-1] == len(p_tr) and len(pf_off) == len(p_tr) + 1
        ps = np.zeros(len(p_tr), np.float32)
        prk = np.zeros(len(p_tr), np.int64)
        for i in range(n):
            rows_of = {}  # one oracle row per relation of the slot
            for j in range(int(p_off[i]), int(p_off[i + 1])):
                p, o = int(p_tr[j, 0]), int(p_tr[j, 1])
                if p not in rows_of:
                    rows_of[p] = np.asarray(oracle_row(self._ctx, (n_ent, p, 0), x[i]))
                ps[j], prk[j] = triple_results(rows_of[p], pf[pf_off[j]:pf_off[j + 1]], o, self._minimizer)
            self.slots.append({"x": np.array(x[i]), "score": float(s[i]), "rank": int(r[i]),
                               "probes": [(int(p_tr[j, 0]), int(p_tr[j, 1]), float(ps[j]), int(prk[j]))
                                          for j in range(int(p_off[i]), int(p_off[i + 1]))]})
        return ret + ((ps, prk),)


def wrap(model):
    """Give ``model`` (with a stand-in context already set) a probe-serving context."""
    model._ctx = ProbeContext(model._ctx, model.is_minimizer())
    return model._ctx
