"""The attributions restated in numpy (TEST INFRASTRUCTURE), written from the text of
include/kelpie_hip.h, "Attributions", and from nothing else: one row at a time, no merging of
rows by relation or pair, no attention, no row map.

Two modes:

``"f64"``   every quantity in float64 (the inputs are the float32 tables, rows and
            hyper-parameters read as doubles);
``"f32"``   the device's roundings emulated where it rounds: the kelpie row, the Adagrad
            state, the per-item contribution rows (the rows of a minibatch that share a relation,
            or a frozen (h, r) pair, summed in float64 and rounded once), the step gradient and the
            update in float32 arithmetic, the regulariser's moduli in float32; the attributions
            themselves and delta in float64.

``grad_fn(x, row) -> (gamma, rho)`` replaces the hand-derived row gradients (test_attrib_cpu.py
passes torch autograd of the reference-shaped loss there).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


# ----------------------------------------------------------------------------- the products
def fwd(prod, v, r):
    """J_r v = v o r: the family's product of a row with a relation row."""
    if prod == "DistMult":
        return v * r
    h = v.shape[-1] // 2
    a, b, c, e = v[..., :h], v[..., h:], r[..., :h], r[..., h:]
    return np.concatenate([a * c - b * e, a * e + b * c], -1)


def bwd(prod, v, r):
    """J_r^T v."""
    if prod == "DistMult":
        return v * r
    h = v.shape[-1] // 2
    a, b, c, e = v[..., :h], v[..., h:], r[..., :h], r[..., h:]
    return np.concatenate([a * c + b * e, -a * e + b * c], -1)


def modulus(prod, x):
    """The family's modulus of every coordinate, in the row's shape and dtype: the complex
    modulus of a (re, im) pair for ComplEx, |x_i| for DistMult."""
    if prod == "DistMult":
        return np.abs(x)
    h = len(x) // 2
    m = np.sqrt(x[:h] * x[:h] + x[h:] * x[h:])
    return np.concatenate([m, m])


def norm2(prod, x):
    """||f|| of the row: the L2 norm of the moduli (one per factor)."""
    m = modulus(prod, x)
    if prod != "DistMult":
        m = m[:len(x) // 2]
    return np.sqrt((m * m).sum(dtype=x.dtype))


def score_gradient(prod, E, R, p, o):
    """c = grad_x score(kelpie, p, o) = J_{R_p}^T E_o, float64."""
    return bwd(prod, E[o].astype(np.float64), R[p].astype(np.float64))


# ----------------------------------------------------------------------------- the definition
def rows_gamma(prod, E, R, x, rows):
    """gamma_i(x) = grad_x [lse_i(x) - s_{i,target}(x)] of every row of ``rows`` [b][3], float64
    [b][dim], everything but x frozen.  Row by row: one softmax over [E; x] per row, nothing
    shared between rows (the rows are only stacked for numpy)."""
    K = len(E)
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    Eall = np.vstack([E, x[None]])
    head = rows[:, 0] == K
    q = fwd(prod, Eall[rows[:, 0]], R[rows[:, 1]])
    sc = q @ Eall.T
    p = np.exp(sc - sc.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    g = (p[:, K] - (rows[:, 2] == K))[:, None] * q  # through the kelpie column
    through_q = bwd(prod, p @ Eall - Eall[rows[:, 2]], R[rows[:, 1]])  # through the query
    return g + np.where(head[:, None], through_q, 0.0)


def row_gamma(prod, E, R, x, row):
    return rows_gamma(prod, E, R, x, [row])[0]


def occurrences(row, K):
    return int(row[0] == K) + int(row[2] == K)


def row_rho(prod, x, row, K, w, n2, mod=None, nrm=None):
    """rho_i(x) = occ_i 3 w |x| o x (N3) or occ_i 3 w ||f|| x (N2), float64; ``mod`` / ``nrm``:
    the moduli to use instead of float64 ones (the "f32" mode's)."""
    if w == 0:
        return np.zeros(len(x))
    if n2:
        m = float(norm2(prod, x) if nrm is None else nrm)
    else:
        m = modulus(prod, x) if mod is None else mod.astype(np.float64)
    return occurrences(row, K) * 3.0 * w * m * x


def minibatches(n_rows, batch_size, epochs, perms):
    """The index arrays of every step of a slot, in step order."""
    if n_rows == 0:
        return
    nst = -(-n_rows // batch_size)
    for e in range(epochs):
        if nst == 1:
            yield np.arange(n_rows)
            continue
        perm = np.asarray(perms[e * n_rows:(e + 1) * n_rows], np.int64)
        for st in range(0, n_rows, batch_size):
            yield perm[st:st + min(batch_size, n_rows)]


def _items(rows, idx, K):
    """The minibatch's rows grouped as the device groups them: per relation the rows with the
    kelpie as head (first-seen order), then per frozen (h, r) pair the others."""
    q, t = {}, {}
    for i in idx:
        h, r, _ = (int(v) for v in rows[i])
        (q.setdefault(r, []) if h == K else t.setdefault((h, r), [])).append(int(i))
    return list(q.values()) + list(t.values())


def attributions(prod, E, R, hp, x0, rows, perms, pred, mode="f64", grad_fn=None):
    """One slot: {"fit" [rows], "reg" [rows], "delta", "x" (the final row), "c"}.  ``hp``: an
    object with optimizer (0 Adagrad, 2 SGD), epochs, batch_size, lr, eps, reg_weight, reg_kind
    (1: N2), as kelpie_amd._lib.HP has them."""
    assert mode in ("f64", "f32") and int(hp.optimizer) in (0, 2)
    E64, R64 = np.asarray(E, np.float64), np.asarray(R, np.float64)
    K = len(E64)
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    n = len(rows)
    adagrad = int(hp.optimizer) == 0
    lr, eps, w, n2 = float(hp.lr), float(hp.eps), float(hp.reg_weight), int(hp.reg_kind) == 1
    c = score_gradient(prod, E64, R64, int(pred[1]), int(pred[2]))
    fit, reg = np.zeros(n), np.zeros(n)
    ft = F32 if mode == "f32" else np.float64
    x = np.asarray(x0, F32).astype(ft)
    x_first = x.astype(np.float64)
    state = np.zeros(len(x), ft)
    for idx in minibatches(n, int(hp.batch_size), int(hp.epochs), perms):
        b = len(idx)
        x64 = x.astype(np.float64)
        mod = nrm = None
        if mode == "f32" and w != 0:
            mod, nrm = modulus(prod, x), norm2(prod, x)  # float32 arithmetic, as the update's
        gam, rho = {}, {}
        if grad_fn is None:
            G = rows_gamma(prod, E64, R64, x64, rows[idx])
        for k, i in enumerate(idx):
            if grad_fn is not None:
                gam[i], rho[i] = grad_fn(x64, rows[i])
            else:
                gam[i] = G[k]
                rho[i] = row_rho(prod, x64, rows[i], K, w, n2, mod, nrm)
        if mode == "f64":
            g = (sum(gam[i] for i in idx) + sum(rho[i] for i in idx)) / b
            if adagrad:
                state = state + g * g
                D = lr / (np.sqrt(state) + eps)
            else:
                D = np.full(len(x), lr)
            x = x - D * g
        else:
            acc = np.zeros(len(x), F32)
            for item in _items(rows, idx, K):
                acc = acc + sum(gam[i] for i in item).astype(F32)  # the item's row, rounded once
            inv_b = F32(1.0) / F32(b)
            g = acc * inv_b
            if w != 0:
                occ = F32(sum(occurrences(rows[i], K) for i in idx))
                k3 = F32(3.0) * F32(w) * inv_b * occ * (nrm if n2 else mod)
                g = g + k3 * x
            if adagrad:
                state = state + g * g
                std = np.sqrt(state) + F32(eps)
                D = F32(lr) / std
                x = x + (-F32(lr) * g) / std
            else:
                D = np.full(len(x), F32(lr))
                x = x + (-F32(lr)) * g
            assert g.dtype == F32 and x.dtype == F32 and state.dtype == F32 and D.dtype == F32
        v = c * D.astype(np.float64)
        for i in idx:
            fit[i] -= (v @ gam[i]) / b
            reg[i] -= (v @ rho[i]) / b
    xT = x.astype(np.float64)
    return {"fit": fit, "reg": reg, "delta": float(c @ (xT - x_first)), "x": x.astype(F32), "c": c}


def batch(prod, E, R, hp, x0, row_off, rows, rng_off, rng, pred, mode="f32"):
    """Every slot of a posttrain_rank batch: (fit [rows], reg [rows], delta [n], x [n][dim])."""
    n = len(row_off) - 1
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    fit, reg = np.zeros(int(row_off[-1])), np.zeros(int(row_off[-1]))
    delta, xs = np.zeros(n), []
    for s in range(n):
        a, z = int(row_off[s]), int(row_off[s + 1])
        perms = np.asarray(rng[int(rng_off[s]):int(rng_off[s + 1])], np.int64)
        out = attributions(prod, E, R, hp, x0[s], rows[a:z], perms, pred[s], mode)
        fit[a:z], reg[a:z], delta[s] = out["fit"], out["reg"], out["delta"]
        xs.append(out["x"])
    return fit, reg, delta, np.stack(xs) if xs else np.zeros((0, np.asarray(E).shape[1]), F32)
