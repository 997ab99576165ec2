"""The rank margins in numpy float64 (TEST INFRASTRUCTURE): a restatement of the definition in
include/kelpie_hip.h, "Rank margins", written from the header's text and sharing no code with
the library.

``margins(mode, c, masked, o, tol)`` takes one rank row: the compared values ``c`` of the
columns 0 .. n_ent (the kelpie entity last; squared distances for TransE L2, logits for ConvE),
the boolean mask of the filtered columns, the target column ``o`` and the tolerance.  ConvE
rows also pass ``saturated``: per column, whether the float32 sigmoid of its logit is 1.0.

``count_bounds`` serves the device tests: with a per-column error bound
``eps`` on the compared values, the counts a correct implementation may return lie between
the counts without and with the columns inside ``eps`` of a threshold.
"""
from __future__ import annotations

import numpy as np

DOT, SIGMOID, DIST, DIST1 = "dot", "sigmoid", "dist", "dist1"
MINIMIZERS = (DIST, DIST1)
FIELDS = ("rank_lo", "rank_hi", "ties", "gap_better", "gap_worse", "id_better", "id_worse")


def units(mode, c):
    """A compared value in score units."""
    return np.sqrt(c) if mode == DIST else c


def thresholds(mode, c_t, tol):
    """(thr_lo, thr_hi) in compared units."""
    c_t = np.float64(c_t)
    tol = np.float64(tol)
    if tol == 0.0:
        return c_t, c_t
    v_t = np.float64(units(mode, c_t))
    delta = tol * max(np.float64(1.0), abs(v_t))
    if mode == DIST:
        lo = max(v_t - delta, np.float64(0.0))
        hi = v_t + delta
        return min(lo * lo, c_t), max(hi * hi, c_t)  # never across c_t, whatever the root's rounding
    if mode == DIST1:
        return c_t - delta, c_t + delta
    return c_t + delta, c_t - delta


def own_count(mode, masked, o):
    """What the rank counts for the target column itself: a minimizer restores its target
    before counting, a maximizer leaves a filtered target out."""
    return 1 if mode in MINIMIZERS or not bool(masked[o]) else 0


def others(masked, o):
    """The unmasked columns other than the target."""
    keep = ~np.asarray(masked, bool)
    keep[o] = False
    return keep


def as_good(mode, c, thr):
    return c <= thr if mode in MINIMIZERS else c >= thr


def margins(mode, c, masked, o, tol, saturated=None):
    c = np.asarray(c, np.float64)
    o = int(o)
    keep = others(masked, o)
    c_t = c[o]
    thr_lo, thr_hi = thresholds(mode, c_t, tol)
    own = own_count(mode, masked, o)
    hit_lo, hit_hi = as_good(mode, c, thr_lo), as_good(mode, c, thr_hi)
    if mode == SIGMOID and saturated is not None and bool(saturated[o]):
        sat = np.asarray(saturated, bool)
        hit_lo, hit_hi = hit_lo | sat, hit_hi | sat
    out = {"rank_lo": own + int((hit_lo & keep).sum()), "rank_hi": own + int((hit_hi & keep).sum()),
           "ties": int(((c == c_t) & keep).sum())}
    better = (c < c_t if mode in MINIMIZERS else c > c_t) & keep
    worse = (c > c_t if mode in MINIMIZERS else c < c_t) & keep
    v, v_t = units(mode, c), units(mode, c_t)
    for side, sel, take_min in (("better", better, mode not in MINIMIZERS), ("worse", worse, mode in MINIMIZERS)):
        ids = np.nonzero(sel)[0]
        if len(ids) == 0:
            out["id_" + side], out["gap_" + side] = -1, float("inf")
            continue
        # the closest in compared order: among the better columns of a maximizer the smallest
        # value (the largest of a minimizer), the other way round on the worse side
        best = c[ids].min() if take_min else c[ids].max()
        e = int(ids[c[ids] == best].min())  # the lower column id on equal values
        out["id_" + side], out["gap_" + side] = e, float(abs(v[e] - v_t))
    return out


def count_bounds(mode, c, masked, o, tol, eps, saturated=None):
    """Per threshold the counts without and with the columns within ``eps`` (per column, on the
    compared values; the target's own error included by the caller) of it:
    {"rank_lo": (least, most, undecided), "rank_hi": ...}."""
    c = np.asarray(c, np.float64)
    eps = np.broadcast_to(np.asarray(eps, np.float64), c.shape)
    o = int(o)
    keep = others(masked, o)
    own = own_count(mode, masked, o)
    out = {}
    sat_all = np.zeros(len(c), bool)
    if mode == SIGMOID and saturated is not None and bool(saturated[o]):
        sat_all = np.asarray(saturated, bool)
    for name, thr in zip(("rank_lo", "rank_hi"), thresholds(mode, c[o], tol)):
        near = (np.abs(c - thr) <= eps) & keep & ~sat_all
        sure = (as_good(mode, c, thr) | sat_all) & keep & ~near
        out[name] = (own + int(sure.sum()), own + int(sure.sum()) + int(near.sum()), int(near.sum()))
    return out
