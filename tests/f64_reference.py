"""The Kelpie MultiClassNLL post-training restated in numpy float64 (TEST INFRASTRUCTURE).

The definition of include/kelpie_hip.h, "fp64": what the reference returns when every tensor
of the run is a float64 one (tools/conditioning.py's ``fp64`` variant) -- the fp32 tables
upcast, the fp32 draw upcast and scaled by ``init_scale`` in float64 (the caller's ``x0``),
the Python doubles as hyper-parameters, and the row, the query, the logits, the softmax,
the gradient, the N3 / N2 term, the optimizer state and the update in float64 in torch's
op order (multiclass_nll_optimizer.py:57-164, complex.py:58-112, distmult.py:38-68,
regularizers.py:25-46, torch/optim/adagrad.py, adam.py, sgd.py), the score and the rank from
the float64 row (post_training_engine.py:101-125).

The oracle's ``posttrain_complex`` keeps the row and the optimizer state in float32 and is
not this.  Two float64 implementations of one definition (this one and torch's) differ in
summation order and libm only; ``MEASURED_F64`` below is the largest relative distance
between them over every fp64 run the goldens record (test_f64_cpu.py measures it again,
prints it and holds it to the tolerance), and ``TOL_F64`` = 8 x that, the margin for the
device's third summation order and its ``exp`` / ``log``.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64

# The largest relative distance (score: |a - b| / max(1, |b|); row: max |a - b| / max |b|)
# between this restatement and the reference's own fp64 runs, measured on the CPU over
# tests/golden/complex200_reg_fullwidth.json (none / N3 / N2, 36 post-trainings, scores) and
# tests/golden/distmult_tiny.json (4 post-trainings, scores and rows): 6.2e-16 without a
# regulariser, 8.68e-14 with N3 (the element whose fp32 run is 1.5e-3 off; N2 no larger),
# 4.2e-17 / 1.6e-16 on the DistMult scores / rows.
MEASURED_F64 = 8.7e-14
TOL_F64 = 8 * MEASURED_F64


def _query(model_name, lhs, rel):
    """q = lhs o rel of the rows (complex.py:65-72, distmult.py:52-54)."""
    if model_name == "DistMult":
        return lhs * rel
    d = lhs.shape[1] // 2
    a, b, c, e = lhs[:, :d], lhs[:, d:], rel[:, :d], rel[:, d:]
    return np.hstack([a * c - b * e, a * e + b * c])


def _scores(model_name, q, Eall):
    """q against every row of Eall (complex.py:74-78: the two halves' products added)."""
    if model_name == "DistMult":
        return q @ Eall.T
    d = q.shape[1] // 2
    return q[:, :d] @ Eall[:, :d].T + q[:, d:] @ Eall[:, d:].T


def _factor(model_name, rows):
    """The regulariser's factor of each row: the moduli (complex.py:80-84, distmult.py:66)."""
    if model_name == "DistMult":
        return np.sqrt(rows ** 2)
    d = rows.shape[1] // 2
    return np.sqrt(rows[:, :d] ** 2 + rows[:, d:] ** 2)


def posttrain(model_name, E, R, x0, rows, draws, hp):
    """The kelpie row after KelpieMultiClassNLLOptimizer.train on ``rows`` (the kelpie triples
    followed by their inverses, the kelpie entity as id ``len(E)``), float64.  ``draws``: the
    shipped ``epochs x len(rows)`` randperm values, or empty for a one-step slot (whose
    permutation only reorders the batch); ``hp``: the explanation's training block."""
    E = np.asarray(E, np.float32).astype(F64)
    R = np.asarray(R, np.float32).astype(F64)
    x = np.asarray(x0, F64).copy()
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    draws = np.asarray(draws, np.int64).reshape(-1)
    K, n = E.shape[0], len(rows)
    epochs, batch_size = int(hp["epochs"]), int(hp["batch_size"])
    if n == 0 or epochs == 0:
        return x
    bs = min(batch_size, n)
    name = hp["optimizer_name"]
    lr = float(hp["lr"])
    b1, b2 = float(hp.get("decay1", 0.9)), float(hp.get("decay2", 0.999))
    w_reg = float(hp.get("regularizer_weight", 0.0))
    n2 = hp.get("regularizer_name", "N3") == "N2"
    s1, s2, t = np.zeros_like(x), np.zeros_like(x), 0
    for ep in range(epochs):
        perm = draws[ep * n:(ep + 1) * n] if draws.size >= epochs * n else np.arange(n)
        prow = rows[perm]
        for start in range(0, n, batch_size):
            batch = prow[start:start + bs]
            B = len(batch)
            Eall = np.vstack([E, x[None]])
            lhs, rel, rhs = Eall[batch[:, 0]], R[batch[:, 1]], Eall[batch[:, 2]]
            q = _query(model_name, lhs, rel)
            logits = _scores(model_name, q, Eall)
            # CrossEntropyLoss(mean): log_softmax, whose backward is (softmax - onehot) / B
            z = logits - logits.max(1, keepdims=True)
            P = np.exp(z - np.log(np.exp(z).sum(1, keepdims=True)))
            P[np.arange(B), batch[:, 2]] -= 1.0
            G = P / B
            g = G[:, K] @ q  # the kelpie row as a candidate tail
            hk = batch[:, 0] == K
            if hk.any():  # the kelpie row as the head: through q = x o rel
                dq = G[hk] @ Eall
                r_ = rel[hk]
                if model_name == "DistMult":
                    g = g + (dq * r_).sum(0)
                else:
                    d = x.size // 2
                    dr, di, c, e = dq[:, :d], dq[:, d:], r_[:, :d], r_[:, d:]
                    g = g + np.hstack([(dr * c + di * e).sum(0), (di * c - dr * e).sum(0)])
            if w_reg != 0.0:
                # N3: w sum |f|^3 / B -> 3 w / B |f| x per row holding x (head or tail);
                # N2: w sum_rows ||f||^3 / B -> 3 w / B ||f|| x
                cnt = int(hk.sum()) + int((batch[:, 2] == K).sum())
                f = _factor(model_name, x[None])[0]
                mod = np.sqrt((f ** 2).sum()) if n2 else (f if model_name == "DistMult" else np.hstack([f, f]))
                g = g + cnt * (3 * w_reg / B * mod * x)
            t += 1
            if name == "Adagrad":
                s1 = s1 + g * g
                x = x + (-lr * g) / (np.sqrt(s1) + 1e-10)
            elif name == "Adam":
                s1 = s1 + (1 - b1) * (g - s1)
                s2 = s2 * b2 + ((1 - b2) * g) * g
                step_size = lr / (1 - b1 ** t)
                den = np.sqrt(s2) / np.sqrt(1 - b2 ** t) + 1e-8
                x = x + (-step_size * s1) / den
            else:
                x = x + (-lr) * g
    return x


def score_row(model_name, E, R, x, rel):
    """The scores of (kelpie, rel, .) over the n_ent + 1 columns, the kelpie column last."""
    E = np.asarray(E, np.float32).astype(F64)
    R = np.asarray(R, np.float32).astype(F64)
    Eall = np.vstack([E, np.asarray(x, F64)[None]])
    q = _query(model_name, Eall[-1:], R[int(rel)][None])
    return _scores(model_name, q, Eall)[0]


def triple_results(row, obj, filt):
    """get_triple_results of a maximizer on a score row: (target score, filtered rank)."""
    s = np.asarray(row, F64).copy()
    target = float(s[int(obj)])
    s[np.asarray(filt, np.int64)] = -1e6
    return target, int((s >= target).sum())


def rank_bounds(row, obj, filt, tol=TOL_F64):
    """The project's derived rank bound [#{s_e >= t + delta}, #{s_e >= t - delta}], delta =
    tol * max(1, |t|), over the unfiltered entities other than the ranked object, plus one
    when the object counts itself (unfiltered)."""
    s = np.asarray(row, F64).copy()
    target = float(s[int(obj)])
    delta = tol * max(1.0, abs(target))
    filt = np.asarray(filt, np.int64)
    own = 0 if int(obj) in set(filt.tolist()) else 1
    s[filt] = -1e6
    s[int(obj)] = -2e6
    return own + int((s >= target + delta).sum()), own + int((s >= target - delta).sum())
