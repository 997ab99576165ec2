"""CPU stand-in of the attributions (TEST INFRASTRUCTURE): ``attrib=`` in front of any
oracle-backed ComplEx or DistMult stand-in (cpu_backend.OracleBackedContext,
distmult_backend.DistMultOracleContext, the margins', probes' and marks' stand-ins), used as they
are.

``AttribStandIn`` subclasses the margins' stand-in: a call without ``attrib`` goes where it went.
With ``attrib`` it passes the call on without it, asks for the rows, and answers the
attributions by the restatement (attrib_reference.py, float32-emulating mode) on the same
inputs.  The restatement walks the oracle's trajectory: its final row must be the oracle's
within the project's row rule (1e-4 of the row's largest magnitude), asserted per slot.  Never
used by the product.
"""
from __future__ import annotations

import numpy as np

import attrib_reference as ar
from margins_backend import MarginsStandIn


class AttribStandIn(MarginsStandIn):
    def __init__(self, inner):
        super().__init__(inner)
        assert self.om.name == "ComplEx", "attributions serve ComplEx and DistMult"
        self.attrib_calls = []  # per call: whether attributions were asked for
        d = self.om.E.shape[1] // 2
        # a DistMult stand-in holds [E | 0]: the restatement reads the real halves
        self.E = self.om.E[:, :d] if self.distmult else self.om.E
        self.R = self.om.R[:, :d] if self.distmult else self.om.R
        self.prod = "DistMult" if self.distmult else "ComplEx"

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, attrib=False,
                       **kw):
        self.attrib_calls.append(bool(attrib))
        if not attrib:
            return super().posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=want_x, **kw)
        assert int(hp.optimizer) != 1, "Adam"
        assert not any(int(p[2]) == len(self.E) for p in pred), "a kelpie tail"
        out = super().posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=True, **kw)
        fit, reg, delta, x = ar.batch(self.prod, self.E, self.R, hp, x0, row_off, rows, rng_off, rng, pred, mode="f32")
        for i in range(len(delta)):
            scale = float(np.abs(out[2][i]).max())
            assert float(np.abs(x[i] - out[2][i]).max()) <= 1e-4 * scale, (i, scale)
        ret = list(out)
        if not want_x:
            ret[2] = None
            if kw.get("marks") is not None:
                at = 3 + sum((bool(kw.get("topk")), kw.get("probes") is not None, bool(kw.get("trace"))))
                ret[at] = (ret[at][0], ret[at][1], None)
        return tuple(ret) + ((fit, reg, delta),)
