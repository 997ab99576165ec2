"""GPU: the baseline kernels at their pivoting, singular and width edges.

The cases are baseline_cases.py's; test_baseline_cases_cpu.py shows on the CPU that they
swap rows (across waves from D = 200), that the pinned ones are exact, which candidates are
singular, and measures TOL_CRIAGE and TOL_DP.

  P  kp_criage_solve promises the bits of the unblocked column-by-column elimination.  With
     the perspective entity's row zero every sigmoid is exactly 0.5 and nothing else in the
     pipeline depends on an order of float32 sums, so the necessary engine's value equals
     -criage_plain(...) under numpy.array_equal: no tolerance.  A solver that pivots
     differently, or not at all, changes bits here (the CPU test shows it for every width
     from D = 32) where it would pass any tolerance.
  T, E  within TOL_CRIAGE of the oracle (numpy.linalg.inv), relative to max(1e-3, |ref|).
  S  exactly singular systems: None from the necessary engine, LinAlgError from the
     sufficient one, the regular systems of the same launch untouched.
  D  kp_dp_complex within TOL_DP of the float64 restatement, relative to the sum of the
     |products| of its two scores.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import numpy as np
import pytest

import baseline_cases as bc
import kelpie_amd.baselines as kb

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(prob):
    """One device model (and context) per problem."""
    if prob.name not in _MODELS:
        _MODELS[prob.name] = prob.model("gpu")
    return _MODELS[prob.name]


# ----------------------------------------------------------------------------- P
@pytest.mark.parametrize("dim", bc.P_DIMS, ids=[f"D{2 * d}" for d in bc.P_DIMS])
def test_pinned_equals_plain_elimination_bitwise(dim):
    prob, pred, cands = bc.graded(dim, True)
    got = kb.NecessaryCriageEngine(_model(prob), prob.ds).compute_relevance_batch(pred, cands, "tail")
    exp = [prob.plain(pred, c) for c in cands]
    equal = sum(int(g is not None and np.array_equal(np.float64(g), -v)) for g, (v, _, _) in zip(got, exp))
    worst = max((bc.rel_dist(g, -v) for g, (v, _, _) in zip(got, exp) if g is not None), default=float("nan"))
    print(f"{prob.name}: {equal} of {len(cands)} values bitwise equal, largest distance {worst:.2e}; "
          f"{sum(e[1] for e in exp)} columns swapped, {sum(e[2] for e in exp)} across waves")
    for c, g, (v, _, _) in zip(cands, got, exp):
        assert g is not None and np.array_equal(np.float64(g), -v), (prob.name, c, g, -v)


# ----------------------------------------------------------------------------- T
T_CASES = [("ComplEx", d) for d in bc.T_DIMS] + [("ConvE", d) for d in bc.T_CONVE]


@pytest.mark.parametrize("family,dim", T_CASES, ids=[f"{m}-d{d}" for m, d in T_CASES])
def test_values_within_tol_of_oracle(family, dim):
    prob, pred, cands = bc.graded(dim, False) if family == "ComplEx" else bc.conve(dim)
    got = kb.NecessaryCriageEngine(_model(prob), prob.ds).compute_relevance_batch(pred, cands, "tail")
    dist = [bc.rel_dist(g, -prob.oracle(pred, c)) for c, g in zip(cands, got)]
    print(f"{prob.name}: largest distance {max(dist):.2e}, TOL_CRIAGE {bc.TOL_CRIAGE:.1e}")
    assert None not in got
    assert max(dist) <= bc.TOL_CRIAGE, (prob.name, dist)


# ----------------------------------------------------------------------------- E
def test_several_entities_necessary():
    """Three perspective entities in one launch (kp_criage_hessian's blockIdx.y, three
    Hessians behind one item list)."""
    prob, jobs, _ = bc.several()
    nec = kb.NecessaryCriageEngine(_model(prob), prob.ds)
    multi = nec.compute_relevance_multi(jobs, "tail")
    worst = 0.0
    for (pred, cands), got in zip(jobs, multi):
        assert len(got) == len(cands) and None not in got
        for c, g in zip(cands, got):
            d = bc.rel_dist(g, -prob.oracle(pred, c))
            worst = max(worst, d)
            assert d <= bc.TOL_CRIAGE, (pred, c, g, d)
        # one workgroup per item, one Hessian per entity: no arithmetic across items
        assert got == nec.compute_relevance_batch(pred, cands, "tail"), pred
    print(f"{prob.name}: largest distance {worst:.2e}, TOL_CRIAGE {bc.TOL_CRIAGE:.1e}")


def test_several_entities_sufficient():
    prob, _, (pred, triples, ents) = bc.several()
    suf = kb.SufficientCriageEngine(_model(prob), prob.ds)
    suf.entities_to_convert = ents
    got = suf.compute_relevance_batch(pred, triples, "tail")
    dist = [bc.rel_dist(g, prob.oracle_sufficient(pred, t, ents)) for t, g in zip(triples, got)]
    print(f"{prob.name} sufficient: largest distance {max(dist):.2e}, TOL_CRIAGE {bc.TOL_CRIAGE:.1e}")
    assert max(dist) <= bc.TOL_CRIAGE, dist
    assert suf.compute_relevance(pred, triples[0], "tail") == got[0]


# ----------------------------------------------------------------------------- S
@pytest.mark.parametrize("col", [35, 3], ids=["second-panel", "first-panel"])
def test_singular_systems(col):
    prob, jobs, flags = bc.singular(col)
    model = _model(prob)
    nec = kb.NecessaryCriageEngine(model, prob.ds)
    regular = [j for j, s in zip(jobs, flags) if not s]
    alone = [nec.compute_relevance_batch(pred, cands, "tail") for pred, cands in regular]
    for (pred, cands), got in zip(regular, alone):
        for c, g in zip(cands, got):
            assert g is not None and bc.rel_dist(g, -prob.oracle(pred, c)) <= bc.TOL_CRIAGE, (pred, c, g)
    multi = nec.compute_relevance_multi(jobs, "tail")
    for (pred, cands), sing, got in zip(jobs, flags, multi):
        assert len(got) == len(cands)
        if sing:
            assert got == [None] * len(cands), (pred, got)
    assert [g for g, s in zip(multi, flags) if not s] == alone  # bitwise, beside singular neighbours
    suf = kb.SufficientCriageEngine(model, prob.ds)
    suf.entities_to_convert = [0]
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        suf.compute_relevance_batch(jobs[0][0], jobs[0][1], "tail")
    suf.entities_to_convert = [2]
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        suf.compute_relevance_batch(jobs[2][0], jobs[2][1], "tail")
    again = [nec.compute_relevance_batch(pred, cands, "tail") for pred, cands in regular]
    assert again == alone  # the context is unharmed


# ----------------------------------------------------------------------------- D
@pytest.mark.parametrize("rd", bc.DP_RDS)
def test_data_poisoning_widths_and_roles(rd):
    prob, blocks = bc.dp_case(rd)
    model = _model(prob)
    worst = 0.0
    for mode, pred, persp, triples, ents in blocks:
        eng = bc.dp_engine(model, prob.ds, mode, ents)
        got = eng.compute_relevance_batch(pred, persp, triples)
        assert len(got) == len(triples)
        for t, g in zip(triples, got):
            v, scale = bc.dp_plain(prob.om, pred, persp, t, bc.DP_EPS, mode, ents)
            worst = max(worst, abs(float(g) - v) / scale)
            assert isinstance(g, np.float32)
            assert abs(float(g) - v) <= bc.TOL_DP * scale, (rd, mode, pred, persp, t, g, v, bc.TOL_DP * scale)
        assert eng.compute_relevance(pred, persp, triples[0]) == got[0]
    print(f"{prob.name}: largest distance {worst:.2e} of the sum of |products|, TOL_DP {bc.TOL_DP:.1e}")
    # several predictions in one launch: one wave per item
    for persp in ("head", "tail"):
        nec_blocks = [b for b in blocks if b[0] == "necessary" and b[2] == persp]
        eng = bc.dp_engine(model, prob.ds, "necessary", None)
        multi = eng.compute_relevance_multi([(b[1], b[3]) for b in nec_blocks], persp)
        for b, m in zip(nec_blocks, multi):
            assert m == eng.compute_relevance_batch(b[1], persp, b[3])
