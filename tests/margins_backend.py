"""CPU stand-in of the rank margins (TEST INFRASTRUCTURE): ``margins=`` in front of any
oracle-backed stand-in (cpu_backend.OracleBackedContext, distmult_backend.DistMultOracleContext,
the recorders of width_cases, the probes' and marks' stand-ins), used as they are.

``MarginsStandIn`` passes the call on without ``margins``, asks for the rows, and answers the
margins by the definition itself (margins_reference.py) on the oracle's own scoring of the
returned rows, read as float64: the oracle's float32 scores are the compared values of ComplEx,
DistMult and TransE L1, their exact squares those of TransE L2, and ConvE's are the float32
logits of the oracle's encoder (its scores are their float32 sigmoids).  A float32 value is
exact in float64 and so is its square, hence the stand-in's own rank is the count at ``tol`` =
0 of the very values the margins are taken from.  Never used by the product.

``rows`` keeps, per call with margins, every rank row's inputs to the definition -- (kind, c,
masked, o, saturated, kelpie triple, kelpie row) -- so that a test can restate or vary them.
"""
from __future__ import annotations

import numpy as np

import margins_reference as mr
from kelpie_amd import _lib
from oracle import kelpie_oracle as ko


def find_oracle(ctx):
    """(the oracle model under a chain of stand-ins, whether a DistMult stand-in is on the way)."""
    distmult = False
    while True:
        d = vars(ctx)
        if "om" in d:
            return d["om"], distmult
        distmult = distmult or type(ctx).__name__ == "DistMultOracleContext"
        ctx = d.get("inner", d.get("_ctx"))
        if ctx is None:
            raise AttributeError("no oracle-backed stand-in under this context")


def mode_of(om):
    if om.name == "TransE":
        return mr.DIST1 if om.norm == 1 else mr.DIST
    return mr.SIGMOID if om.name == "ConvE" else mr.DOT


def compared_row(om, distmult, kelpie_triple, x):
    """(compared values float64 over the columns 0 .. n_ent, saturated flags or None) of
    (kelpie, p, .) on the kelpie row ``x``, from the oracle's own scoring."""
    x = np.asarray(x, np.float32)
    if distmult:
        x = np.concatenate([x, np.zeros_like(x)])
    if om.name == "ConvE":
        E = np.vstack([om.E, x[None]])
        enc, _ = om.conve_encode(E[[kelpie_triple[0]]], om.R[[kelpie_triple[1]]])
        logits = (enc @ E.T).astype(np.float32)[0]
        return logits.astype(np.float64), ko.sigmoid_f32(logits) == np.float32(1.0)
    row = om.all_scores([kelpie_triple], kelpie_row=x)[0].astype(np.float64)
    return (row * row if mode_of(om) == mr.DIST else row), None


class MarginsStandIn:
    def __init__(self, inner):
        self.inner = inner
        self.om, self.distmult = find_oracle(inner)
        self.mode = mode_of(self.om)
        self.margin_calls = []  # per call: the tolerance asked for (None: none)
        self.rows = []          # per call with margins: the rank rows' inputs, slots first

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def _row(self, kind, triple, x, filt, tol, log):
        c, sat = compared_row(self.om, self.distmult, triple, x)
        masked = np.zeros(len(c), bool)
        f = np.asarray(filt, np.int64)
        masked[f[(f >= 0) & (f < len(c))]] = True
        log.append((kind, c, masked, int(triple[2]), sat, tuple(int(v) for v in triple), np.array(x, np.float32)))
        return mr.margins(self.mode, c, masked, triple[2], tol, saturated=sat)

    @staticmethod
    def _arrays(recs, shape):
        return {name: np.asarray([r[name] for r in recs], dt).reshape(shape) for name, dt in _lib.MARGIN_FIELDS}

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, margins=None,
                       **kw):
        self.margin_calls.append(margins)
        if margins is None:
            return self.inner.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt,
                                             want_x=want_x, **kw)
        tol = float(margins)
        assert 0.0 <= tol <= 1.0
        out = self.inner.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=True, **kw)
        res = _lib.split_rank_result(out, **kw)
        n = len(res.score)
        pred = np.asarray(pred, np.int64).reshape(n, 3)
        filt_off, filt = np.asarray(filt_off, np.int64), np.asarray(filt, np.int64)
        log = []
        slot_f = [filt[filt_off[i]:filt_off[i + 1]] for i in range(n)]
        slots = [self._row("slot", tuple(pred[i]), res.x[i], slot_f[i], tol, log) for i in range(n)]
        for i, m in enumerate(slots):  # the stand-in's own rank is the count at tol = 0 of the same values
            m0 = mr.margins(self.mode, *log[i][1:4], 0.0, saturated=log[i][4])
            assert m0["rank_lo"] == m0["rank_hi"] == int(res.rank[i]), (i, m0, int(res.rank[i]))
        mg_p = mg_m = None
        if kw.get("probes") is not None and len(np.asarray(kw["probes"][1]).reshape(-1, 2)):
            p_off, p_tr, pf_off, pf = kw["probes"]
            p_tr, pf = np.asarray(p_tr, np.int64).reshape(-1, 2), np.asarray(pf, np.int64)
            recs = []
            for i in range(n):
                for j in range(int(p_off[i]), int(p_off[i + 1])):
                    recs.append(self._row("probe", (int(pred[i][0]), int(p_tr[j, 0]), int(p_tr[j, 1])), res.x[i],
                                          pf[pf_off[j]:pf_off[j + 1]], tol, log))
            mg_p = self._arrays(recs, len(recs))
        if kw.get("marks") is not None:
            m_x = res.marks[2]
            nm = m_x.shape[1]
            recs = [self._row("mark", tuple(pred[i]), m_x[i, j], slot_f[i], tol, log) for i in range(n) for j in range(nm)]
            mg_m = self._arrays(recs, (n, nm))
        self.rows.append(log)
        ret = list(out)
        if not want_x:
            ret[2] = None
            if kw.get("marks") is not None:
                at = 3 + sum((bool(kw.get("topk")), kw.get("probes") is not None, bool(kw.get("trace"))))
                ret[at] = (ret[at][0], ret[at][1], None)
        return tuple(ret) + ((self._arrays(slots, n), mg_p, mg_m),)
