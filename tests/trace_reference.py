"""The post-training trace's definition in fp64 numpy (TEST INFRASTRUCTURE).

A restatement of one step's loss from include/kelpie_hip.h ("Post-training trace"), given
the kelpie row before the step and the step's minibatch: what kp_posttrain_rank_trace
returns per step, before its one fp32 rounding.  ComplEx and DistMult
(multiclass_nll_optimizer.py:122-135 on complex.py:58-86 / distmult.py:51-68,
regularizers.py:25-46) and TransE (pairwise_ranking_optimizer.py:139-157 on transe.py:67-75,
regularizers.py:15-22) and ConvE (bce_optimizer.py:92-112,190-208 on conve.py:133-158).
"""
from __future__ import annotations

import numpy as np


def slot_steps(model, epochs, batch_size, rows):
    """kp_trace_steps' rule for one slot: rows [R][3], inverses included."""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    n = len(rows)
    if model == "ConvE":
        n = len({(int(h), int(r)) for h, r, _ in rows})
    if n == 0 or epochs <= 0:
        return 0
    return int(epochs) * ((n + batch_size - 1) // batch_size)


def _factors(model, rows):
    """The regulariser's factor moduli of embedding rows [n][dim] -> [n][w]."""
    rows = np.asarray(rows, np.float64)
    if model == "ComplEx":
        h = rows.shape[1] // 2
        return np.sqrt(rows[:, :h] ** 2 + rows[:, h:] ** 2)
    return np.abs(rows)


def _product(model, lhs, rel):
    if model == "ComplEx":
        h = lhs.shape[1] // 2
        a, b, c, e = lhs[:, :h], lhs[:, h:], rel[:, :h], rel[:, h:]
        return np.hstack([a * c - b * e, a * e + b * c])
    return lhs * rel


def step_loss(model, E, R, x, batch, reg_name="N3", reg_weight=0.0):
    """``l`` of step_on_batch on ``batch`` [B][3] (kelpie-form rows; the kelpie entity is id
    len(E)) with the kelpie row ``x``: CrossEntropyLoss(mean) over the n_ent + 1 columns plus
    the regulariser's value over all three factors of every row of the batch."""
    E = np.asarray(E, np.float64)
    R = np.asarray(R, np.float64)
    x = np.asarray(x, np.float64)[:E.shape[1]]
    batch = np.asarray(batch, np.int64).reshape(-1, 3)
    table = np.vstack([E, x[None, :]])
    lhs, rel, rhs = table[batch[:, 0]], R[batch[:, 1]], table[batch[:, 2]]
    scores = _product(model, lhs, rel) @ table.T
    m = scores.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(scores - m).sum(1))
    fit = float(np.mean(lse - scores[np.arange(len(batch)), batch[:, 2]]))
    if reg_weight == 0:
        return fit
    total = 0.0
    for f in (_factors(model, lhs), _factors(model, rel), _factors(model, rhs)):
        if reg_name == "N3":
            total += float(np.sum(np.abs(f) ** 3))
        elif reg_name == "N2":
            total += float(np.sum(np.sqrt(np.sum(f ** 2, 1)) ** 3))
        else:
            raise ValueError(reg_name)
    return fit + float(reg_weight) * total / len(batch)


def transe_batches(rows, draws, ratio, batch_size, step):
    """(positive, negative) rows of step ``step`` of one epoch from its draws [row order |
    negative entity | head_or_tail] (kp_batch.rng's layout): position j steps
    rows[order[j // ratio]], corrupted in the head when head_or_tail[j] == 1, else in the tail."""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    R = len(rows)
    d = np.asarray(draws, np.int64).reshape(3, R)
    j = np.arange(step * batch_size, min(R, (step + 1) * batch_size))
    pos = rows[d[0][j // ratio]]
    neg = pos.copy()
    head = d[2][j] == 1
    neg[head, 0] = d[1][j][head]
    neg[~head, 2] = d[1][j][~head]
    return pos, neg


def transe_step_loss(E, R, x, pos, neg, norm=2, margin=0.0, reg_weight=0.0):
    """``l`` of the pairwise optimizer's step_on_batch: mean(max(0, f+ - f- + margin)) +
    reg_weight * (L2(pos) + L2(neg)) / 2, f = ||lhs + rel - rhs||_norm, L2 = (mean lhs^2 +
    mean rel^2 + mean rhs^2) / 3 over the batch's rows."""
    E = np.asarray(E, np.float64)
    R = np.asarray(R, np.float64)
    table = np.vstack([E, np.asarray(x, np.float64)[None, :E.shape[1]]])

    def side(batch):
        batch = np.asarray(batch, np.int64).reshape(-1, 3)
        lhs, rel, rhs = table[batch[:, 0]], R[batch[:, 1]], table[batch[:, 2]]
        v = lhs + rel - rhs
        f = np.abs(v).sum(1) if norm == 1 else np.sqrt((v ** 2).sum(1))
        return f, (np.mean(lhs ** 2) + np.mean(rel ** 2) + np.mean(rhs ** 2)) / 3.0

    fp, lp = side(pos)
    fn, ln = side(neg)
    return float(np.mean(np.maximum(0.0, fp - fn + margin)) + reg_weight * (lp + ln) / 2.0)


def conve_encode64(w, lhs, rel, masks=(None, None, None), eps=1e-5):
    """ConvE's encoder (conve.py:133-153) in fp64 with the batch norms in eval mode: lhs, rel
    [b][d]; ``masks`` = the dropouts' multipliers (input [b][2d], feature map [b][32], hidden
    [b][d]; None: not drawn); ``w``: synth.make_weights' ConvE dict."""
    f = lambda k: np.asarray(w[k], np.float64)  # noqa: E731
    b, d = lhs.shape
    eh = d // 20

    def bn(x, i, shape):
        a = f(f"bn{i}_weight") / np.sqrt(f(f"bn{i}_var") + eps)
        return x * a.reshape(shape) + (f(f"bn{i}_bias") - f(f"bn{i}_mean") * a).reshape(shape)

    img = bn(np.concatenate([lhs.reshape(b, 20, eh), rel.reshape(b, 20, eh)], axis=1), 1, (1, 1, 1))
    if masks[0] is not None:
        img = img * masks[0].reshape(b, 40, eh)
    W = f("conv_weight").reshape(32, 3, 3)
    conv = np.zeros((b, 32, 38, eh - 2))
    for ky in range(3):
        for kx in range(3):
            conv += img[:, None, ky:ky + 38, kx:kx + eh - 2] * W[None, :, ky, kx, None, None]
    fm = np.maximum(bn(conv + f("conv_bias").reshape(1, 32, 1, 1), 2, (1, 32, 1, 1)), 0.0)
    if masks[1] is not None:
        fm = fm * masks[1].reshape(b, 32, 1, 1)
    fc = fm.reshape(b, -1) @ f("fc_weight").T + f("fc_bias")
    if masks[2] is not None:
        fc = fc * masks[2]
    return np.maximum(bn(fc, 3, (1, d)), 0.0)


def conve_step_loss(w, x, pairs, er, masks, label_smoothing, with_logits=False):
    """``l`` of the BCE optimizer's step_on_batch on the (head, relation) ``pairs`` with tails
    ``er[pair]``: BCELoss (mean over b x (n_ent + 1), each log clamped at -100) of the train-mode
    forward against (1 - ls) y + 1 / (n_ent + 1); the kelpie entity is id n_ent, its row ``x``."""
    table = np.vstack([np.asarray(w["entity_embeddings"], np.float64), np.asarray(x, np.float64)[None]])
    R = np.asarray(w["relation_embeddings"], np.float64)
    hs, rs = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    s = conve_encode64(w, table[hs], R[rs], masks) @ table.T
    y = np.zeros_like(s)
    for i, pr in enumerate(pairs):
        y[i, er[pr]] = 1.0
    if label_smoothing:
        y = (1.0 - label_smoothing) * y + 1.0 / y.shape[1]
    lp = np.minimum(s, 0.0) - np.log1p(np.exp(-np.abs(s)))  # log sigmoid(s)
    l = float(np.mean(-(y * np.maximum(lp, -100.0) + (1.0 - y) * np.maximum(lp - s, -100.0))))
    return (l, s) if with_logits else l
