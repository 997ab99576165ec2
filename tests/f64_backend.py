"""CPU stand-ins for the fp64 entry point of a context (TEST INFRASTRUCTURE).

``F64Context`` answers ``posttrain_rank_f64`` with the numpy float64 restatement
(f64_reference.py) on exactly the arrays the product ships across the C ABI, and records per
slot what the device tests hold the device to: score, rank, final row, the restatement's own
score row and the derived rank bound from it.  It has no ``posttrain_rank``: an engine in
fp64 that called the fp32 entry point would fail on it.  ``CallLog`` wraps any context and
logs every post-training call with its arguments; ``F64Recording`` wraps the device's context
and records its fp64 slots.
"""
from __future__ import annotations

import numpy as np

import f64_reference as fr


class F64Context:
    def __init__(self, model):
        assert model.name in ("ComplEx", "DistMult")
        self.model = model
        self.name = model.name
        self.E, self.R = model.entity_embeddings, model.relation_embeddings
        self.n_ent, self.dim = self.E.shape
        self.slots = []

    @staticmethod
    def _hp(hp64):
        hp = hp64.hp
        return {"optimizer_name": {0: "Adagrad", 1: "Adam", 2: "SGD"}[hp.optimizer], "batch_size": hp.batch_size,
                "epochs": hp.epochs, "lr": hp64.lr, "decay1": hp64.beta1, "decay2": hp64.beta2,
                "regularizer_weight": hp64.reg_weight, "regularizer_name": {0: "N3", 1: "N2"}[hp.reg_kind]}

    def posttrain_rank_f64(self, hp64, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False):
        x0 = np.asarray(x0)
        assert x0.dtype == np.float64, x0.dtype
        n = len(row_off) - 1
        hp = self._hp(hp64)
        out_s, out_r = np.zeros(n, np.float64), np.zeros(n, np.int64)
        out_x = np.zeros((n, self.dim), np.float64)
        for i in range(n):
            x = fr.posttrain(self.name, self.E, self.R, x0[i], rows[row_off[i]:row_off[i + 1]],
                             rng[rng_off[i]:rng_off[i + 1]], hp)
            kp = tuple(int(v) for v in pred[i])
            f = np.asarray(filt[filt_off[i]:filt_off[i + 1]], np.int64)
            row = fr.score_row(self.name, self.E, self.R, x, kp[1])
            out_s[i], out_r[i] = fr.triple_results(row, kp[2], f)
            out_x[i] = x
            lo, hi = fr.rank_bounds(row, kp[2], f)
            self.slots.append({"score": float(out_s[i]), "rank": int(out_r[i]), "lo": lo, "hi": hi, "x": x,
                               "row": row, "n_rows": int(row_off[i + 1] - row_off[i])})
        return out_s, out_r, (out_x if want_x else None)

    def last_timing(self):
        return {"device_s": 0.0, "hot_s": 0.0, "hot_launches": 0}


class CallLog:
    """Wraps a context and logs (name, positional arguments as bytes / values) of every
    post-training call; everything else passes through."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.log = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    @staticmethod
    def _freeze(a):
        if isinstance(a, np.ndarray):
            return (str(a.dtype), a.shape, a.tobytes())
        if hasattr(a, "_fields_"):  # a ctypes structure
            return bytes(a)
        if hasattr(a, "_fields"):  # HP64
            return tuple(CallLog._freeze(v) for v in a)
        return a

    def _call(self, name, args, kw):
        self.log.append((name, tuple(self._freeze(np.asarray(a) if isinstance(a, (list, tuple)) else a) for a in args),
                         tuple(sorted((k, repr(v)) for k, v in kw.items()))))
        return getattr(self._ctx, name)(*args, **kw)

    def posttrain_rank(self, *args, **kw):
        return self._call("posttrain_rank", args, kw)

    def posttrain_rank_f64(self, *args, **kw):
        return self._call("posttrain_rank_f64", args, kw)


class F64Recording:
    """Wraps a context (the device's) and records every fp64 slot in call order."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.slots = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def posttrain_rank_f64(self, hp64, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False):
        s, r, x = self._ctx.posttrain_rank_f64(hp64, x0, row_off, rows, rng_off, rng, pred, filt_off, filt,
                                               want_x=True)
        for i in range(len(s)):
            self.slots.append({"score": float(s[i]), "rank": int(r[i]), "x": x[i].copy()})
        return s, r, (x if want_x else None)


def check_slots(got, ref):
    """Every slot of ``got`` against the restatement's record: score within TOL_F64 *
    max(1, |ref|), final row within TOL_F64 of its largest magnitude, rank inside the derived
    bound.  Returns (exact ranks, largest score error, largest row error), both relative."""
    assert len(got) == len(ref) and len(ref) > 0, (len(got), len(ref))
    exact, ws, wx = 0, 0.0, 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        es = abs(a["score"] - b["score"]) / max(1.0, abs(b["score"]))
        scale = float(np.abs(b["x"]).max())
        ex = float(np.abs(a["x"] - b["x"]).max()) / scale
        ws, wx = max(ws, es), max(wx, ex)
        print(f"slot {i}: score {a['score']!r} ref {b['score']!r} err {es:.2e}; row err {ex:.2e}; "
              f"rank {a['rank']} ref {b['rank']} [{b['lo']}, {b['hi']}]")
        assert es <= fr.TOL_F64, (i, a["score"], b["score"], es)
        assert ex <= fr.TOL_F64, (i, ex)
        assert b["lo"] <= a["rank"] <= b["hi"], (i, a["rank"], b["lo"], b["hi"])
        exact += int(a["rank"] == b["rank"])
    return exact, ws, wx
