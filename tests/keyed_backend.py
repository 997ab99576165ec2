"""CPU stand-in of an armed context (TEST INFRASTRUCTURE): keyed draws in front of any
oracle-backed stand-in (cpu_backend.OracleBackedContext, distmult_backend.DistMultOracleContext,
the recorders of width_cases, the extras' stand-ins), used as they are.

``arm_keyed`` keeps the keys; the next ``posttrain_rank`` whose ``x0``, ``rng_off`` and ``rng``
are all None gets them from the numpy restatement of the definition (keyed_reference.py) and
goes to the wrapped stand-in: the draws are inputs, so every oracle rule applies unchanged.
Never used by the product."""
from __future__ import annotations

import numpy as np

import keyed_reference as kr


class KeyedStandIn:
    def __init__(self, inner, model):
        self.inner = inner
        self.model_name = model.name
        self.dim = model.dimension
        self.armed = None
        self.keyed_calls = 0   # armed calls served
        self.fed = []          # (x0, rng_off, rng) of each, as generated

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def arm_keyed(self, init_keys, slot_keys, x0_scale, neg_bound=0):
        self.armed = None if init_keys is None else (list(init_keys), list(slot_keys), x0_scale, neg_bound)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, **kw):
        if x0 is None and rng_off is None and rng is None:
            if self.armed is None:
                raise RuntimeError("kp_posttrain_rank: missing buffer")
            ik, sk, scale, bound = self.armed
            self.armed = None
            if len(ik) != len(row_off) - 1:
                raise RuntimeError("keyed draws: n_slots differs from the batch's")
            x0, rng_off, rng = kr.batch_draws(self.model_name, self.dim, int(hp.epochs), int(hp.batch_size),
                                              np.asarray(row_off), ik, sk, scale, bound)
            if rng.size == 0:
                rng = np.zeros(1, np.int32)
            self.keyed_calls += 1
            self.fed.append((x0, rng_off, rng))
        return self.inner.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, **kw)
