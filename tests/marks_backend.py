"""CPU stand-in for the epoch marks (TEST INFRASTRUCTURE).

``MarksContext`` wraps a stand-in context (cpu_backend.OracleBackedContext, or one of the
recording stand-ins of width_cases / distmult_backend) and answers
``posttrain_rank(..., marks=[e_0, ...])`` by the definition itself (include/kelpie_hip.h,
"Epoch marks"): mark j of a slot is what the stand-in returns for that slot on the same batch
with ``hp.epochs = e_j``.  The shorter run reads a prefix of the slot's draws: ComplEx /
DistMult the first e_j permutations, ConvE the first steps' keep-bit words, TransE the first
e_j blocks [order | entities | head_or_tail].

``force_epochs`` makes every call run that many epochs whatever ``hp`` says, on the draws of
the longer run: a stand-in engine "whose slots ran e epochs", which ``compute_curves``'
``curve[j]`` has to equal.
"""
from __future__ import annotations

import numpy as np


def hp_with_epochs(hp, epochs):
    out = type(hp).from_buffer_copy(hp)
    out.epochs = int(epochs)
    return out


def prefix_draws(model_name, hp, row_off, rng_off, rng, epochs):
    """The batch's draws cut to ``epochs`` epochs: (rng_off, rng).  Only TransE's stand-in needs
    the cut (it reshapes a slot's block by its epoch count); the other families read from the
    front of a slot's draws."""
    if model_name != "TransE":
        return rng_off, rng
    parts, off = [], [0]
    for i in range(len(row_off) - 1):
        R = int(row_off[i + 1] - row_off[i])
        blob = np.asarray(rng[rng_off[i]:rng_off[i + 1]])
        assert len(blob) >= int(hp.epochs) * 3 * R
        parts.append(blob[:epochs * 3 * R])
        off.append(off[-1] + len(parts[-1]))
    return np.asarray(off, np.int64), (np.concatenate(parts) if off[-1] else np.zeros(1, np.int32))


class MarksContext:
    def __init__(self, inner, model_name, force_epochs=None):
        self.inner = inner
        self.model_name = model_name
        self.force_epochs = force_epochs
        self.mark_calls = []   # per call: the marks asked for (None: none)
        self.mark_slots = []   # per call with marks: per slot, per mark, the inner record of that run

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def _run(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, epochs):
        ro, rg = prefix_draws(self.model_name, hp, row_off, rng_off, rng, epochs)
        return self.inner.posttrain_rank(hp_with_epochs(hp, epochs), x0, row_off, rows, ro, rg, pred, filt_off, filt,
                                         want_x=True)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, marks=None):
        args = (np.asarray(x0), np.asarray(row_off), np.asarray(rows), np.asarray(rng_off), np.asarray(rng),
                np.asarray(pred), np.asarray(filt_off), np.asarray(filt))
        self.mark_calls.append(None if marks is None else [int(e) for e in marks])
        if self.force_epochs is not None:
            s, r, x = self._run(hp, *args, epochs=self.force_epochs)
        else:
            s, r, x = self.inner.posttrain_rank(hp, *args, want_x=True)
        out = (s, r, x if want_x else None)
        if marks is None:
            return out
        n = len(args[1]) - 1
        ep = [int(e) for e in marks]
        assert ep == sorted(set(ep)) and 1 <= len(ep) <= 16 and ep[0] >= 0 and ep[-1] <= int(hp.epochs)
        m_s = np.zeros((n, len(ep)), np.float32)
        m_r = np.zeros((n, len(ep)), np.int64)
        m_x = np.zeros((n, len(ep), np.asarray(x).shape[1]), np.float32)
        records = [[None] * len(ep) for _ in range(n)]
        slots = getattr(self.inner, "slots", None)
        calls = getattr(self.inner, "calls", None)
        for j, e in enumerate(ep):
            n0 = len(slots) if slots is not None else 0
            c0 = len(calls) if calls is not None else 0
            sj, rj, xj = self._run(hp, *args, epochs=e)
            m_s[:, j], m_r[:, j], m_x[:, j] = sj, rj, xj
            if slots is not None:  # the recording stand-ins' records of this run, taken back out of theirs
                for i, rec in enumerate(slots[n0:]):
                    records[i][j] = rec
                del slots[n0:]
            if calls is not None:  # the mark runs are not the engine's batches
                del calls[c0:]
        self.mark_slots.append(records)
        return out + ((m_s, m_r, m_x if want_x else None),)
