"""The post-training trace on the CPU (TEST INFRASTRUCTURE).

``TraceContext`` wraps one of the stand-in contexts (cpu_backend.OracleBackedContext and the
wrappers built on it), which know nothing of traces, so that it accepts
``posttrain_rank(..., trace=True)``: every slot gets a trace of the length kp_trace_steps'
rule gives it (trace_reference.slot_steps), whose values encode where it came from --
``code(call, slot, step)`` -- so that a test can tell which slot's trace the engine put on
which rule, base or conversion.  No loss is computed here: the device's values are checked
in test_trace_gpu.py.
"""
from __future__ import annotations

import numpy as np

from trace_reference import slot_steps


def code(call, slot, step):
    """Exact in float32 for call < 160, slot < 100, step < 1000."""
    return float(call * 100000 + slot * 1000 + step)


class TraceContext:
    """``trace_calls``: per library call whether a trace was asked for; ``slots``: every traced
    slot's (call, slot, rows, score, rank, loss), in call order."""

    def __init__(self, ctx, model_name):
        self._ctx = ctx
        self._name = model_name
        self.trace_calls = []
        self.slots = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, trace=False,
                       **kw):
        out = self._ctx.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=want_x, **kw)
        call = len(self.trace_calls)
        self.trace_calls.append(bool(trace))
        if not trace:
            return out
        rows = np.asarray(rows).reshape(-1, 3)
        losses = []
        for i in range(len(row_off) - 1):
            r = rows[row_off[i]:row_off[i + 1]]
            n = slot_steps(self._name, int(hp.epochs), int(hp.batch_size), r)
            loss = np.array([code(call, i, j) for j in range(n)], np.float32)
            losses.append(loss)
            self.slots.append({"call": call, "slot": i, "rows": len(r), "score": float(out[0][i]),
                               "rank": int(out[1][i]), "loss": loss.tolist()})
        return tuple(out) + (losses,)


def wrap(model):
    """Give ``model`` (with a stand-in context already set) a trace-serving context."""
    model._ctx = TraceContext(model._ctx, model.name)
    return model._ctx
