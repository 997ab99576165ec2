"""The pivoting, singular and width-edge cases of the baseline kernels (TEST INFRASTRUCTURE).

One table, read by test_baseline_edges_gpu.py and by its CPU companion
test_baseline_cases_cpu.py, which shows that every case does what it claims (its swap
counts, its exact sigmoids, its singular candidates) and measures the two tolerances.

  G  graded ComplEx tables: ne = 700, nr = 6, E and R ~ N(0, 0.2^2) in float32, complex
     coordinate j of E (columns j and dim + j) scaled by s_j = exp(U(-ln 4, ln 4)); entity
     0 has D + 60 tail triples from distinct heads.  The grading makes the partial pivoting
     of kp_criage_solve swap rows (a diagonal grading cancels in z_p . A^-1 z_t, so the
     value stays as insensitive to float32 assembly noise as the ungraded one).
  P  G with E[0] = 0: every sigmoid is exactly 0.5 and the device's float64 value is the
     plain elimination's (criage_plain.py) bit for bit.
  T  G as it stands, and ungraded ConvE (width_cases.make_model), within TOL_CRIAGE.
  E  several perspective entities in one launch, both engines.
  S  exactly singular systems beside regular ones.
  D  kp_dp_complex at every trip count of its lane loop and every grid tail.
"""
from __future__ import annotations

import functools
from collections import defaultdict

import numpy as np

import kelpie_amd as ka
import width_cases as wc
from cpu_backend import OracleBackedContext
from criage_plain import Plain
from oracle import kelpie_oracle as ko

F32 = np.float32

TOL_CRIAGE = 3.0e-5
"""Relative bound of a device CRIAGE value against the oracle's, denominator
max(1e-3, |ref|): 8 x the largest distance, over every T and E case, between the oracle
and (i) criage_plain, (ii) the oracle with every float32 w_k and c moved to a random
neighbour.  Measured: 3.72e-6 (the nudged oracle at ComplEx D = 200; criage_plain is within
1.6e-12 everywhere), 8 x = 2.98e-5; test_baseline_cases_cpu.py re-measures it."""

TOL_DP = 6.8e-7
"""Bound of a device data-poisoning value against dp_plain, relative to the sum of the
|products| of its two scores: 8 x the largest distance between oracle.dp_relevance and
dp_plain over every D case.  Measured: 8.47e-8 over 196 items, 8 x = 6.77e-7 (eleven
float32 roundings of 2^-24); test_baseline_cases_cpu.py re-measures it."""

P_DIMS = (1, 16, 17, 32, 33, 100, 200)   # D = 2, 32, 34, 64, 66, 200, 400
T_DIMS = (17, 33, 100, 200)              # D = 34, 66, 200, 400
T_CONVE = (100, 200)                     # Dp = 128, 224
P_CANDS, T_CANDS = 12, 6
# dim -> seed of the graded tables, where not 1000 + dim.  A 2 x 2 system swaps only where
# |H_10| > |H_00|, which one seed in some thousands gives (both columns carry the same s_0);
# at dim 16 the default seed swaps 19 % of the columns, short of the quarter asked of every case
G_SEED = {1: 2460, 16: 1024}
DP_RDS = (1, 8, 63, 64, 65, 100, 200)
DP_EPS = 0.5


def rel_dist(v, ref):
    return abs(v - ref) / max(1e-3, abs(ref))


def tail_index(train):
    tails = defaultdict(list)
    for h, r, t in np.asarray(train).tolist():
        tails[t].append((h, r, t))
    return tails


class Problem:
    """A model, a training set and what the engines are asked about it."""

    def __init__(self, name, model_of, ne, nr, train):
        self.name = name
        self._model_of = model_of
        self.ne, self.nr = ne, nr
        self.train = np.asarray(train, np.int64)
        self.test = self.train[:1]
        self.tails = tail_index(self.train)
        self.ds = ka.Dataset(ne, nr, self.train, self.test[:0], self.test)
        self.ods = ko.OracleDataset(ne, nr, self.train, self.test[:0], self.test)

    def model(self, backend):
        """A fresh model: on the device, or over the oracle-backed stand-in context."""
        m = self._model_of(self.ds)
        if backend == "cpu":
            m._ctx = OracleBackedContext(m)
        return m

    @functools.cached_property
    def om(self):
        return OracleBackedContext(self._model_of(self.ds)).om

    @functools.cached_property
    def plain(self):
        return Plain(self.om, self.tails)

    @property
    def D(self):
        return self.om.E.shape[1]

    # the oracle in tail perspective, as oracle.kelpie_oracle.criage_relevance runs it, with
    # the Hessian of an entity kept; the values have the kernel's (the sufficient) sign
    @functools.lru_cache(maxsize=None)
    def oracle_hessian(self, ent, nudge_seed=None):
        if nudge_seed is None:
            return ko.criage_hessian(self.om, ent, self.tails.get(ent, []))
        return _nudged_hessian(self.om, ent, self.tails.get(ent, []), np.random.default_rng(nudge_seed))

    @functools.lru_cache(maxsize=None)
    def oracle(self, pred, triple):
        """Raises numpy.linalg.LinAlgError where numpy.linalg.inv does."""
        ent = pred[2]
        return float(ko.criage_variation(self.om, ko.criage_z(self.om, pred), ko.criage_z(self.om, triple), ent,
                                         self.oracle_hessian(ent), "sufficient"))

    def oracle_sufficient(self, pred, triple, entities):
        vals = [self.oracle((pred[0], pred[1], e), (triple[0], triple[1], e)) for e in entities]
        return sum(vals) / len(vals)

    def oracle_nudged(self, pred, triple, seed):
        """The oracle with every float32 w_k and c moved to a random float32 neighbour: a
        model of the device's expf and of the order of its float32 dot products."""
        ent = pred[2]
        rng = np.random.default_rng([seed, pred[0], pred[1], triple[0], triple[1]])
        return float(_nudged_variation(self.om, ko.criage_z(self.om, pred), ko.criage_z(self.om, triple), ent,
                                       self.oracle_hessian(ent, seed), rng))


def _neighbour(v, rng):
    v = np.asarray(v, F32)
    return np.nextafter(v, np.where(rng.random(v.shape) < 0.5, F32(-np.inf), F32(np.inf)).astype(F32))


def _nudged_hessian(om, entity, tail_triples, rng):
    """oracle.kelpie_oracle.criage_hessian with w_k moved to a float32 neighbour."""
    e = om.E[entity]
    D = om.E.shape[1]
    H = np.zeros((D, D))
    for s, p, _ in tail_triples:
        x = (om.E[s] * om.R[p]).astype(F32).reshape(1, -1)
        sig = ko._np_sigmoid(np.dot(e, x.T))
        H += _neighbour(sig * (1 - sig), rng) * np.dot(x.T, x)
    return H


def _nudged_variation(om, z_pred, z_triple, entity, H, rng):
    """oracle.kelpie_oracle.criage_variation (sufficient sign) with c moved to a float32 neighbour."""
    sig = ko._np_sigmoid(np.dot(om.E[entity], z_triple.T))
    A = H + _neighbour(sig * (1 - sig), rng) * np.dot(z_triple.T, z_triple)
    m = np.linalg.inv(A)
    return np.dot(z_pred, ((1 - sig) * np.dot(z_triple, m)).T)[0][0]


def _complex_problem(name, E, R, ne, nr, train):
    return Problem(name, lambda ds: ka.ComplEx(ds, E, R, init_scale=1e-3), ne, nr, train)


def _tail_rows(rng, ent, count, ne, rels, exclude=()):
    """``count`` triples (h, r, ent) from distinct heads."""
    pool = np.setdiff1d(np.arange(ne), np.asarray([ent, *exclude]))
    heads = rng.choice(pool, size=count, replace=False)
    return [(int(h), int(rng.choice(rels)), ent) for h in heads]


def graded_tables(dim, seed, ne=700, nr=6):
    rng = np.random.default_rng(seed)
    D = 2 * dim
    E = (0.2 * rng.standard_normal((ne, D))).astype(F32)
    R = (0.2 * rng.standard_normal((2 * nr, D))).astype(F32)
    s = np.exp(rng.uniform(-np.log(4.0), np.log(4.0), dim)).astype(F32)
    E = (E * np.concatenate([s, s])[None, :]).astype(F32)
    return rng, E, R


# ----------------------------------------------------------------------------- G, P, T
@functools.lru_cache(maxsize=None)
def graded(dim, pinned):
    """(problem, pred, candidates): candidates are entity 0's first tail triples."""
    ne, nr, D = 700, 6, 2 * dim
    rng, E, R = graded_tables(dim, G_SEED.get(dim, 1000 + dim), ne, nr)
    train = _tail_rows(rng, 0, D + 60, ne, np.arange(nr))
    train += [(int(rng.integers(1, ne)), int(rng.integers(nr)), int(rng.integers(1, ne))) for _ in range(400)]
    if pinned:
        E = E.copy()
        E[0] = 0
    prob = _complex_problem(f"ComplEx-D{D}-{'pinned' if pinned else 'graded'}", E, R, ne, nr, train)
    pred = (train[1][0], 1, 0)
    n = P_CANDS if pinned else T_CANDS
    return prob, pred, [tuple(t) for t in train[:n]]


@functools.lru_cache(maxsize=None)
def conve(dim):
    """Ungraded ConvE (its z comes out of the encoder and does not scale with E's columns,
    so a grading would make the value ill-conditioned): width_cases' weights, entity 0 with
    dim + 60 tail triples."""
    case = wc._case("ConvE", dim)
    src = wc.make_model(case)
    ne, nr = src.dataset.num_entities, src.dataset.num_relations
    rng = np.random.default_rng(2000 + dim)
    train = _tail_rows(rng, 0, dim + 60, ne, np.arange(nr))
    train += [(int(rng.integers(1, ne)), int(rng.integers(nr)), int(rng.integers(1, ne))) for _ in range(400)]

    def model_of(ds):
        m = wc.make_model(case)
        m.dataset = ds
        return m

    prob = Problem(f"ConvE-D{dim}", model_of, ne, nr, train)
    return prob, (train[1][0], 1, 0), [tuple(t) for t in train[:T_CANDS]]


def p_cases():
    return [graded(d, True) for d in P_DIMS]


def t_cases():
    return [graded(d, False) for d in T_DIMS] + [conve(d) for d in T_CONVE]


def old_fullrank(dim):
    """The inputs of test_baselines._criage_fullrank, restated: N(0, 0.3^2), ungraded."""
    rng = np.random.default_rng(dim)
    ne, nr, D = 700, 6, 2 * dim
    heads = rng.choice(np.arange(1, ne), size=D + 60, replace=False)
    train = ([(int(h), int(rng.integers(nr)), 0) for h in heads] +
             [(int(rng.integers(1, ne)), int(rng.integers(nr)), int(rng.integers(1, ne))) for _ in range(400)])
    E = (0.3 * rng.standard_normal((ne, D))).astype(F32)
    R = (0.3 * rng.standard_normal((2 * nr, D))).astype(F32)
    prob = _complex_problem(f"ComplEx-D{D}-fullrank", E, R, ne, nr, train)
    return prob, (int(heads[1]), 1, 0), [tuple(t) for t in train[:6]]


# ----------------------------------------------------------------------------- E
E_DIM = 33
E_COUNTS = (1, 2 * E_DIM - 1, 2 * E_DIM + 60)
"""Tail triples of the necessary launch's three perspective entities 1, 2 and 0 as first
meant: 1, D - 1 and D + 60.  With fewer than D tails H_e is rank-deficient, A singular up to
rounding, and the oracle's own value moves by 3e0 (1 tail) and 2e-3 (D - 1 tails) when its
float32 weights move by one ulp.  E_COUNTS_USED are the counts the cases run with: the first
of D + 10 k at which it moves no more than in the T cases (test_baseline_cases_cpu.py)."""
E_COUNTS_USED = (2 * E_DIM + 10, 2 * E_DIM + 20, 2 * E_DIM + 60)
E_CONVERT = (0, 3, 4)


@functools.lru_cache(maxsize=None)
def several(counts=None):
    """ComplEx D = 66, tail perspective.  Necessary: jobs over the perspective entities 1, 2
    and 0 with ``counts`` tail triples, at most four candidates each.  Sufficient: one
    prediction, four candidate triples, entities_to_convert 0, 3 and 4 (D + 60 tails each)."""
    counts = tuple(counts or E_COUNTS_USED)
    dim, ne, nr = E_DIM, 700, 6
    D = 2 * dim
    rng, E, R = graded_tables(dim, 3000 + dim, ne, nr)
    ents = (1, 2, 0)
    special = (0, 1, 2, 3, 4)
    rows = {}
    for ent, n in zip(ents, counts):
        rows[ent] = _tail_rows(rng, ent, n, ne, np.arange(nr), exclude=special)
    for ent in E_CONVERT[1:]:
        rows[ent] = _tail_rows(rng, ent, D + 60, ne, np.arange(nr), exclude=special)
    train = [t for ent in (1, 2, 0, 3, 4) for t in rows[ent]]
    train += [(int(rng.integers(5, ne)), int(rng.integers(nr)), int(rng.integers(5, ne))) for _ in range(200)]
    prob = _complex_problem(f"ComplEx-D{D}-entities{counts}", E, R, ne, nr, train)
    jobs = []
    for ent in ents:
        cands = [tuple(t) for t in rows[ent][:4]]
        jobs.append(((int(rows[0][5 + ent][0]), 1 + ent, ent), cands))
    suff = ((int(rows[0][9][0]), 2, 0), [tuple(t) for t in rows[0][:4]], list(E_CONVERT))
    return prob, jobs, suff


# ----------------------------------------------------------------------------- S
S_DIM = 40


@functools.lru_cache(maxsize=None)
def singular(col):
    """ComplEx dim 40 (D = 80, Dp = 96); relation 2's row is zero at columns ``col`` and
    40 + ``col``, so x = E_h * R_2 and z(., 2) are exactly zero there.
      entity 0: every tail triple uses relation 2; relation-2 candidates: A has two zero
                rows and columns, the first zero pivot is column ``col``
      entity 1: tails and candidates of the other relations: regular
      entity 2: no tail triples, relation-2 candidates: singular
    Returns (problem, jobs, singular flags per job)."""
    dim, ne, nr = S_DIM, 300, 6
    D = 2 * dim
    rng = np.random.default_rng(4000 + col)
    E = (0.3 * rng.standard_normal((ne, D))).astype(F32)
    R = (0.3 * rng.standard_normal((2 * nr, D))).astype(F32)
    R[2, col] = R[2, dim + col] = 0
    special = (0, 1, 2)
    a = _tail_rows(rng, 0, D + 60, ne, [2], exclude=special)
    b = _tail_rows(rng, 1, D + 60, ne, [0, 1, 3, 4, 5], exclude=special)
    train = a + b + [(int(rng.integers(3, ne)), int(rng.integers(nr)), int(rng.integers(3, ne))) for _ in range(100)]
    prob = _complex_problem(f"ComplEx-D{D}-zero{col}", E, R, ne, nr, train)
    jobs = [((a[1][0], 2, 0), [tuple(t) for t in a[:3]]),
            ((b[1][0], 1, 1), [tuple(t) for t in b[:3]]),
            ((a[2][0], 0, 2), [(a[3][0], 2, 2), (b[3][0], 2, 2)])]
    return prob, jobs, [True, False, True]


# ----------------------------------------------------------------------------- D
def dp_products(om, h, r, t, lhs=None, rhs=None):
    """The four float64 products per complex coordinate of ComplEx's score of (h, r, t),
    over float32 rows: (a0 c0) b0, -(a1 c1) b0, (a0 c1) b1, (a1 c0) b1."""
    d = om.dim
    a = np.asarray(om.E[h] if lhs is None else lhs, np.float64)
    c = np.asarray(om.R[r], np.float64)
    b = np.asarray(om.E[t] if rhs is None else rhs, np.float64)
    return np.stack([a[:d] * c[:d] * b[:d], -(a[d:] * c[d:] * b[:d]), a[:d] * c[d:] * b[d:], a[d:] * c[:d] * b[d:]])


def dp_plain_item(om, pred, perspective, triple, eps, mode):
    """(value, scale) of one item in float64: the gradient, the step and the perturbed row
    in float32 as the reference forms them, both scores summed in float64; scale is the sum
    of the |products| of the two scores."""
    s, p, o = pred
    h, r, t = triple
    ent = s if perspective == "head" else o
    g = ko.complex_score_grad(om, pred, ent)
    step = (F32(eps) * g).astype(F32)
    pert = (om.E[ent] - step if mode == "necessary" else om.E[ent] + step).astype(F32)  # maximizer
    orig = dp_products(om, h, r, t)
    per = dp_products(om, h, r, t, lhs=pert) if h == ent else dp_products(om, h, r, t, rhs=pert)
    diff = orig.sum() - per.sum()
    return (diff if mode == "necessary" else -diff), float(np.abs(orig).sum() + np.abs(per).sum())


def dp_plain(om, pred, perspective, triple, eps, mode, entities=None):
    if mode == "necessary":
        return dp_plain_item(om, tuple(pred), perspective, tuple(triple), eps, mode)
    vals = []
    pred_s = pred[0]
    for ent in entities:  # the reference rebinds triple and pred inside its loop
        triple = ko.replace_entity(tuple(triple), pred_s, ent)
        pred = ko.replace_entity(tuple(pred), pred_s, ent)
        vals.append(dp_plain_item(om, pred, perspective, triple, eps, mode))
    return sum(v for v, _ in vals) / len(vals), sum(s for _, s in vals) / len(vals)


DP_SEED = {}  # rd -> seed, where not the default


@functools.lru_cache(maxsize=None)
def dp_case(rd):
    """(problem, blocks); a block is (mode, pred, perspective, triples, entities_to_convert).
    Launches of 1, 4, 5 and 9 items in necessary mode (the grid's tail of four waves per
    workgroup), 8 and 15 in sufficient mode; with e the perspective entity, the roles
      head perspective, the triple's head is e             (lhs gradient, lhs perturbed)
      head perspective, e only at the triple's tail        (lhs gradient, rhs perturbed)
      tail perspective, the triple's tail is e             (rhs gradient, rhs perturbed)
      tail perspective, the triple's head is e             (rhs gradient, lhs perturbed)
      a triple without e                                   (the reference perturbs its rhs)
      a self-loop prediction s == o, either perspective."""
    ne, nr = 40, 4
    rng = np.random.default_rng(DP_SEED.get(rd, 5000 + rd))
    E = (0.3 * rng.standard_normal((ne, 2 * rd))).astype(F32)
    R = (0.3 * rng.standard_normal((2 * nr, 2 * rd))).astype(F32)
    train = [(int(rng.integers(ne)), int(rng.integers(nr)), int(rng.integers(ne))) for _ in range(60)]
    prob = _complex_problem(f"ComplEx-rd{rd}", E, R, ne, nr, train)
    s, p, o, a = 3, 1, 7, 11
    blocks = [
        ("necessary", (s, p, o), "head",
         [(s, 0, 5), (9, 2, s), (s, p, o), (12, 3, 13), (s, 3, s), (o, 1, s), (s, 2, o), (14, 0, o), (20, 1, 21)], None),
        ("necessary", (s, p, o), "tail", [(5, 0, o), (o, 2, 9), (s, p, o), (12, 3, 13), (o, 3, o)], None),
        ("necessary", (a, 2, a), "head", [(a, 0, 5), (9, 2, a), (a, 2, a), (12, 3, 13)], None),
        ("necessary", (a, 2, a), "tail", [(15, 1, a)], None),
        ("sufficient", (s, p, o), "head", [(s, 0, 5), (9, 2, s), (12, 3, 13), (s, p, o)], [16, 17]),
        ("sufficient", (s, p, o), "tail", [(5, 0, o), (o, 2, 9), (s, p, o), (12, 3, 13), (s, 1, 22)], [18, 19, 23]),
    ]
    return prob, blocks


def dp_engine(model, ds, mode, entities):
    import kelpie_amd.baselines as kb
    if mode == "necessary":
        return kb.NecessaryDPEngine(model, ds, DP_EPS)
    eng = kb.SufficientDPEngine(model, ds, DP_EPS)
    eng.entities_to_convert = list(entities)
    return eng
