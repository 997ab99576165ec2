"""CPU: the cases of baseline_cases.py do what they claim, and the two tolerances are measured.

No GPU: the oracle (numpy.linalg.inv, float32 scores), the plain elimination
(criage_plain.py), the float64 restatement of the data poisoning (baseline_cases.dp_plain)
and the product's host layer over cpu_backend.OracleBackedContext.  Run with ``-s`` for the
swap counts per case, the zero-swap result of the old full-rank inputs and the measured
distances beside TOL_CRIAGE and TOL_DP.
"""
import numpy as np
import pytest

import baseline_cases as bc
import kelpie_amd.baselines as kb
from oracle import kelpie_oracle as ko

NUDGE_SEED = 7


def _swaps(prob, pred, cands):
    """(swapped columns, cross-group swaps, candidates whose value changes bits without pivoting)."""
    sw = cross = differ = 0
    for c in cands:
        v, s, x = prob.plain(pred, c)
        sw, cross = sw + s, cross + x
        differ += int(prob.plain(pred, c, pivot=False)[0] != v)
    return sw, cross, differ


def _distances(prob, pred, cands):
    """Largest distance of criage_plain and of the nudged oracle from the oracle."""
    d_plain = d_nudged = 0.0
    for c in cands:
        ref = prob.oracle(pred, c)
        d_plain = max(d_plain, bc.rel_dist(prob.plain(pred, c)[0], ref))
        d_nudged = max(d_nudged, bc.rel_dist(prob.oracle_nudged(pred, c, NUDGE_SEED), ref))
    return d_plain, d_nudged


# ----------------------------------------------------------------------------- swaps
@pytest.mark.parametrize("pinned", [True, False], ids=["P", "T"])
def test_graded_cases_swap_rows(pinned):
    """Every P and T case from the graded tables: at least a quarter of the columns swap,
    and from D = 200 some swaps cross a 64-row group (another wave's rows)."""
    for dim in (bc.P_DIMS if pinned else bc.T_DIMS):
        prob, pred, cands = bc.graded(dim, pinned)
        sw, cross, differ = _swaps(prob, pred, cands)
        cols = len(cands) * prob.D
        print(f"{prob.name}: {sw} of {cols} columns swap, {cross} across 64-row groups; "
              f"{differ} of {len(cands)} values change bits without pivoting")
        assert 4 * sw >= cols, (prob.name, sw, cols)
        if prob.D >= 200:
            assert cross > 0, prob.name
        if pinned and prob.D >= 34:
            assert differ >= 1, prob.name


def test_old_fullrank_inputs_never_swap():
    """The inputs of test_baselines' full-rank case at dim 200 swap no column, so a solver
    that never pivots gives the same bits there: that test cannot see the pivoting."""
    prob, pred, cands = bc.old_fullrank(200)
    sw, cross, differ = _swaps(prob, pred, cands)
    print(f"{prob.name}: {sw} of {len(cands) * prob.D} columns swap; {differ} values change bits without pivoting")
    assert sw == 0 and cross == 0 and differ == 0


# ----------------------------------------------------------------------------- P
def test_pinned_cases_are_exact_and_agree_with_the_oracle():
    for prob, pred, cands in bc.p_cases():
        assert not prob.om.E[0].any()
        H, w = prob.plain.hessian(0)
        assert w.min() == 0.25 and w.max() == 0.25, prob.name  # min sig' == 0.25: every sigmoid is 0.5
        worst = 0.0
        for c in cands:
            z = prob.plain.z(c[0], c[1])
            assert ko._np_sigmoid(np.dot(prob.om.E[0], z)) == 0.5
            v = prob.plain(pred, c)[0]
            assert v is not None
            worst = max(worst, bc.rel_dist(v, prob.oracle(pred, c)))
        print(f"{prob.name}: criage_plain within {worst:.2e} of the oracle")
        assert worst <= bc.TOL_CRIAGE


# ----------------------------------------------------------------------------- TOL_CRIAGE
def _several_pairs():
    prob, jobs, (spred, striples, ents) = bc.several()
    pairs = [(pred, c) for pred, cands in jobs for c in cands]
    pairs += [((spred[0], spred[1], e), (t[0], t[1], e)) for t in striples for e in ents]
    return prob, pairs


def test_tol_criage_is_eight_times_the_measured_distance():
    worst = 0.0
    for prob, pred, cands in bc.t_cases():
        dp, dn = _distances(prob, pred, cands)
        print(f"{prob.name}: criage_plain {dp:.2e}, nudged oracle {dn:.2e}")
        worst = max(worst, dp, dn)
    prob, pairs = _several_pairs()
    for pred, c in pairs:
        dp, dn = _distances(prob, pred, [c])
        worst = max(worst, dp, dn)
    print(f"{prob.name}: largest over {len(pairs)} systems so far {worst:.2e}")
    print(f"measured {worst:.3e}, 8 x = {8 * worst:.3e}, TOL_CRIAGE = {bc.TOL_CRIAGE:.3e}")
    assert 8 * worst <= bc.TOL_CRIAGE
    assert bc.TOL_CRIAGE <= 16 * worst  # the constant is the measurement, not a round number above it


def test_several_entities_counts():
    """The counts first meant (E_COUNTS: 1 and D - 1 tail triples) leave H rank-deficient and
    A singular up to rounding: the oracle's own value moves by more than the tolerance when
    its float32 weights move by one ulp, so neither side's answer means anything.  The counts
    in use are the first of D + 10 k at which it does not move by more than the T cases do."""
    worst_t = max(max(_distances(prob, pred, cands)) for prob, pred, cands in bc.t_cases())
    prob, jobs, _ = bc.several(bc.E_COUNTS)
    asked = [max(_distances(prob, pred, cands)) for pred, cands in jobs]
    prob, jobs, _ = bc.several()
    used = [max(_distances(prob, pred, cands)) for pred, cands in jobs]
    print(f"tail counts {bc.E_COUNTS}: distances {['%.2e' % d for d in asked]}")
    print(f"tail counts {bc.E_COUNTS_USED}: distances {['%.2e' % d for d in used]} (T cases: {worst_t:.2e})")
    assert asked[0] > bc.TOL_CRIAGE and asked[1] > bc.TOL_CRIAGE
    assert max(used) <= worst_t
    for n in bc.E_COUNTS_USED:
        assert n > 0


# ----------------------------------------------------------------------------- S
@pytest.mark.parametrize("col", [35, 3])
def test_singular_cases(col):
    prob, jobs, flags = bc.singular(col)
    nec = kb.NecessaryCriageEngine(prob.model("cpu"), prob.ds)
    multi = nec.compute_relevance_multi(jobs, "tail")
    for (pred, cands), sing, got in zip(jobs, flags, multi):
        for c, g in zip(cands, got):
            v, sw, _ = prob.plain(pred, c)
            if sing:
                with pytest.raises(np.linalg.LinAlgError):
                    prob.oracle(pred, c)
                assert v is None and g is None, (pred, c, v, g)
            else:
                ref = prob.oracle(pred, c)
                assert np.isfinite(ref) and v is not None and g == -ref
                assert bc.rel_dist(v, ref) <= bc.TOL_CRIAGE
    # where the elimination stops: the first exactly zero pivot is column ``col``
    pred, cands = jobs[0]
    z = prob.plain.z(cands[0][0], cands[0][1])
    H, _ = prob.plain.hessian(0)
    assert z[col] == 0 and z[bc.S_DIM + col] == 0 and not H[:, col].any() and not H[:, bc.S_DIM + col].any()
    assert np.linalg.matrix_rank(H[:, :col]) == col  # the columns before it are independent
    suf = kb.SufficientCriageEngine(prob.model("cpu"), prob.ds)
    suf.entities_to_convert = [0]
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        suf.compute_relevance_batch(jobs[0][0], jobs[0][1], "tail")
    suf.entities_to_convert = [1]
    assert np.isfinite(suf.compute_relevance_batch(jobs[1][0], jobs[1][1], "tail")).all()


# ----------------------------------------------------------------------------- host protocol
def test_criage_cases_through_the_stand_in_context():
    """Every P, T and E run through the product's host layer over the oracle-backed context
    equals the oracle called directly: the items, slots and tail lists the engines ship."""
    for prob, pred, cands in bc.p_cases() + bc.t_cases():
        nec = kb.NecessaryCriageEngine(prob.model("cpu"), prob.ds)
        got = nec.compute_relevance_batch(pred, cands, "tail")
        assert got == [-prob.oracle(pred, c) for c in cands], prob.name
    prob, jobs, (spred, striples, ents) = bc.several()
    nec = kb.NecessaryCriageEngine(prob.model("cpu"), prob.ds)
    multi = nec.compute_relevance_multi(jobs, "tail")
    for (pred, cands), got in zip(jobs, multi):
        assert got == [-prob.oracle(pred, c) for c in cands]
        assert got == nec.compute_relevance_batch(pred, cands, "tail")
    suf = kb.SufficientCriageEngine(prob.model("cpu"), prob.ds)
    suf.entities_to_convert = ents
    got = suf.compute_relevance_batch(spred, striples, "tail")
    for t, g in zip(striples, got):
        assert g == pytest.approx(prob.oracle_sufficient(spred, t, ents), rel=1e-12)


# ----------------------------------------------------------------------------- D
def _dp_items():
    """(rd, block index, triple, oracle value, plain value, scale) of every D item."""
    out = []
    for rd in bc.DP_RDS:
        prob, blocks = bc.dp_case(rd)
        for bi, (mode, pred, persp, triples, ents) in enumerate(blocks):
            for t in triples:
                ref = float(ko.dp_relevance(prob.om, pred, persp, t, bc.DP_EPS, mode, ents))
                v, scale = bc.dp_plain(prob.om, pred, persp, t, bc.DP_EPS, mode, ents)
                out.append((rd, bi, t, ref, v, scale))
    return out


def test_tol_dp_is_eight_times_the_measured_distance():
    items = _dp_items()
    worst = max(abs(ref - v) / scale for _, _, _, ref, v, scale in items)
    print(f"{len(items)} items: measured {worst:.3e} of the sum of |products|, 8 x = {8 * worst:.3e}, "
          f"TOL_DP = {bc.TOL_DP:.3e}")
    assert 8 * worst <= bc.TOL_DP
    assert bc.TOL_DP <= 16 * worst
    # the bound decides: every item's value is at least ten times its bound
    margin = min(abs(v) / (bc.TOL_DP * scale) for _, _, _, _, v, scale in items)
    print(f"smallest |value| / bound = {margin:.1f}")
    for rd, bi, t, ref, v, scale in items:
        assert abs(v) >= 10 * bc.TOL_DP * scale, (rd, bi, t, v, bc.TOL_DP * scale)


def test_dp_cases_through_the_stand_in_context():
    for rd in bc.DP_RDS:
        prob, blocks = bc.dp_case(rd)
        model = prob.model("cpu")
        for mode, pred, persp, triples, ents in blocks:
            eng = bc.dp_engine(model, prob.ds, mode, ents)
            got = eng.compute_relevance_batch(pred, persp, triples)
            for t, g in zip(triples, got):
                assert isinstance(g, np.float32)
                assert g == np.float32(ko.dp_relevance(prob.om, pred, persp, t, bc.DP_EPS, mode, ents)), (rd, mode, t)
            assert eng.compute_relevance(pred, persp, triples[0]) == got[0]
        nec_blocks = [b for b in blocks if b[0] == "necessary" and b[2] == "head"]
        eng = bc.dp_engine(model, prob.ds, "necessary", None)
        multi = eng.compute_relevance_multi([(b[1], b[3]) for b in nec_blocks], "head")
        for b, m in zip(nec_blocks, multi):
            assert m == eng.compute_relevance_batch(b[1], "head", b[3])
