"""The rank margins' cases (TEST INFRASTRUCTURE), read by test_margins_gpu.py and by its CPU
companion test_margins_cpu.py.

The batches are width_cases.py's: on the 517-entity graph, two ordinary subjects with the base
post-training and two singleton candidates each, 8 epochs; one case per family at its smallest
compiled width.  ``TABLES`` are the same batches on graphs of 255, 256 and 257 entities: the
fp64 count scores 256 columns per workgroup, so the last workgroup of the kelpie-less table is
full, absent, or holds one column.

``host_compared`` recomputes a rank row's compared values in numpy float64 from a kelpie row
the device returned, with the any-order summation bound of every column:
``eps_e = 2 (w + 2) 2^-53 sum_i |term_i|`` over the w terms of the column's sum (the products
q_i E_ei of a dot product, the squares or absolute values of q_i - E_ei of a distance), once for
the device's order and once for numpy's.  ``check_against_host`` holds a device margin against
margins_reference.py under that bound.
"""
from __future__ import annotations

import numpy as np

import kelpie_amd as ka
import margins_reference as mr
import width_cases as wc
from golden_io import seed_all
from kelpie_amd import _lib
from marks_cases import Capture

TOLS = (0.0, 1e-6, 1e-4, 1e-2)
TOL = 1e-4

# one case per family at its smallest compiled width; ``seed`` (of the weights) as width_cases /
# marks_cases choose it for these widths, but ConvE's: at their seed 3 none of the stand-in's
# rank rows has a band at tol = 1e-4 (at seed 7 four of 24 have; test_margins_cpu.py asserts it)
FAMILY = [
    wc._case("ComplEx", 32, seed=4),
    wc._case("DistMult", 40, seed=4),
    wc._case("ConvE", 60, seed=7),
    wc._case("TransE", 50, seed=4),
    wc._case("TransE", 260, tag="L1", norm=1),
]
TABLES = [wc._case(m, d, n_ent=n, seed=s) for m, d, s in (("ComplEx", 32, 4), ("TransE", 50, 4)) for n in (255, 256, 257)]
HOST = ("ComplEx", "DistMult", "TransE")  # the families whose compared values numpy recomputes


def ids(cases):
    return [c["id"] for c in cases]


def mode_of(model):
    if model.name == "TransE":
        return mr.DIST1 if int(getattr(model, "norm", 2)) == 1 else mr.DIST
    return mr.SIGMOID if model.name == "ConvE" else mr.DOT


def run(case, ctx_of, tol=TOL, mode="necessary", epochs=None, **engine_attrs):
    """The case's engine batches with margins through ``ctx_of(model)`` wrapped in Capture: the
    captured batches, the model and the reports of compute_margins per subject."""
    ds, ordinary = wc.graph(case["n_ent"])[1:3]
    model = wc.make_model(case)
    model._ctx = cap = Capture(ctx_of(model))
    seed_all(42)
    reports = []
    for pred, ep, n in wc.subjects(case):
        hp = dict(wc.hp_of(case), epochs=ep if epochs is None else epochs)
        if mode == "necessary":
            eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
        else:
            eng = ka.SufficientPostTrainingEngine(model, ds, hp)
            eng.entities_to_convert = [int(p[0]) for p in ordinary if p[0] != pred[0]][:2]
        for name, value in engine_attrs.items():
            setattr(eng, name, value)
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        reports.append(eng.compute_margins(pred, [[c] for c in cands], tol=tol))
    return cap.batches, model, reports


def take_slots(args, idx):
    """The captured batch arguments with the slots ``idx`` (in that order, repeats allowed)."""
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = args

    def csr(off, flat):
        parts = [np.asarray(flat[off[i]:off[i + 1]]) for i in idx]
        new = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        body = np.concatenate(parts) if new[-1] else np.zeros((1,) + np.asarray(flat).shape[1:], np.asarray(flat).dtype)
        return new, body

    ro, rw = csr(row_off, rows)
    go, rg = csr(rng_off, rng)
    fo, fl = csr(filt_off, filt)
    return (hp, np.asarray(x0)[idx], ro.astype(np.int32), rw, go.astype(np.int64), rg, np.asarray(pred)[idx],
            fo.astype(np.int32), fl)


def own_probes(args, copies=1):
    """``copies`` probes per slot, each the slot's own (p, o) with its own filter."""
    _, _, row_off, _, _, _, pred, filt_off, filt = args
    n = len(row_off) - 1
    p_tr = np.repeat(np.asarray(pred)[:, 1:3].astype(np.int32), copies, axis=0)
    fl = [np.asarray(filt[filt_off[i]:filt_off[i + 1]], np.int32) for i in range(n) for _ in range(copies)]
    fo = np.concatenate([[0], np.cumsum([len(v) for v in fl])]).astype(np.int32)
    body = np.concatenate(fl) if fo[-1] else np.zeros(1, np.int32)
    return np.arange(n + 1, dtype=np.int32) * copies, p_tr, fo, body


def margin_rows(mg):
    """A kind's dict of arrays as a list of per-row dicts (row-major)."""
    flat = {k: np.asarray(v).reshape(-1) for k, v in mg.items()}
    return [{k: flat[k][i].item() for k, _ in _lib.MARGIN_FIELDS} for i in range(len(flat["rank_lo"]))]


# ----------------------------------------------------------------------------- the host's values
def host_compared(model, p, x):
    """(c, eps): the compared values of (kelpie, p, .) over the columns 0 .. n_ent on the kelpie
    row ``x`` in numpy float64, and the summation bound of every column."""
    E, R = model.entity_embeddings.astype(np.float64), model.relation_embeddings.astype(np.float64)
    x = np.asarray(x, np.float32).astype(np.float64)
    T = np.vstack([E, x[None]])
    if model.name == "TransE":
        diff = (x + R[p])[None] - T
        terms = np.abs(diff) if mode_of(model) == mr.DIST1 else diff * diff
    else:
        if model.name == "ComplEx":
            d = model.real_dimension
            a, b, cr, ci = x[:d], x[d:], R[p, :d], R[p, d:]
            q = np.concatenate([a * cr - b * ci, a * ci + b * cr])
        else:
            q = x * R[p]
        terms = q[None] * T
    w = terms.shape[1]
    return terms.sum(1), 2.0 * (w + 2) * 2.0 ** -53 * np.abs(terms).sum(1)


def check_against_host(model, kelpie_triple, x, filt, tol, got):
    """One device margin ``got`` (a dict) against the definition on the host's values.  Returns
    the number of undecided columns of the row (over both thresholds).

    A column is undecided at a threshold when its host value lies within eps_e + eps_t' of it:
    eps_e for the column's own two sums, eps_t' for the threshold, which moves with the target's
    two sums (eps_t, times d thr / d c_t = sqrt(thr / c_t) for the squared L2 thresholds).  Each
    device count lies between the host's without and with the undecided columns; a gap lies
    within the two columns' bounds (in score units) of the host's; an id equals the host's where
    the host's two nearest values on that side lie further apart than twice their bounds."""
    mode = mode_of(model)
    _, p, o = (int(v) for v in kelpie_triple)
    c, eps = host_compared(model, p, x)
    masked = np.zeros(len(c), bool)
    f = np.asarray(filt, np.int64)
    masked[f[(f >= 0) & (f < len(c))]] = True
    ref = mr.margins(mode, c, masked, o, tol)
    thr = mr.thresholds(mode, c[o], tol)
    undecided = 0
    for name, t in zip(("rank_lo", "rank_hi"), thr):
        scale = np.sqrt(t / c[o]) if mode == mr.DIST and c[o] > 0 else 1.0
        lo, hi, near = mr.count_bounds(mode, c, masked, o, tol, eps + eps[o] * scale)[name]
        assert lo <= got[name] <= hi, (name, got[name], lo, hi, ref[name])
        undecided += near
    keep = mr.others(masked, o)
    tie_near = int(((np.abs(c - c[o]) <= eps + eps[o]) & keep).sum())
    assert ref["ties"] - tie_near <= got["ties"] <= tie_near, (got["ties"], ref["ties"], tie_near)

    def in_units(v, e):  # a compared value's bound in score units
        return e / (2.0 * np.sqrt(v)) + 2.0 ** -52 * np.sqrt(v) if mode == mr.DIST else e

    for side in ("better", "worse"):
        e_ref = ref["id_" + side]
        if e_ref < 0:
            # no column on that side for the host: the device may see one only inside the bound
            assert got["id_" + side] < 0 or abs(c[got["id_" + side]] - c[o]) <= eps[got["id_" + side]] + eps[o], side
            continue
        sel = keep & ((c < c[o]) if (side == "better") == (mode in mr.MINIMIZERS) else (c > c[o]))
        order = np.argsort(np.abs(c[sel] - c[o]), kind="stable")
        cand = np.nonzero(sel)[0][order]
        bound = in_units(c[e_ref], eps[e_ref]) + in_units(c[o], eps[o])
        # the nearest must itself be clear of the target, or the device may class it as a tie
        clear = abs(c[e_ref] - c[o]) > eps[e_ref] + eps[o]
        apart = len(cand) < 2 or abs(c[cand[1]] - c[cand[0]]) > 2 * (eps[cand[1]] + eps[cand[0]])
        if clear:
            assert abs(got["gap_" + side] - ref["gap_" + side]) <= bound + (0 if apart else in_units(
                c[cand[1]], eps[cand[1]]) + abs(mr.units(mode, c[cand[1]]) - mr.units(mode, c[cand[0]]))), (
                side, got["gap_" + side], ref["gap_" + side], bound)
        if clear and apart:
            assert got["id_" + side] == e_ref, (side, got["id_" + side], e_ref)
    return undecided
