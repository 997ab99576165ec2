"""CRIAGE's float64 solve as a plain elimination (TEST INFRASTRUCTURE).

What kp_criage_solve (kelpie_amd/csrc/kp_baselines.hip) documents, restated in numpy
float64 without the kernel's blocking: no panels, no identity border, no row map, one
column at a time on the D x D system.

  assembly        as oracle.kelpie_oracle.criage_hessian / criage_variation: float32 terms
                  w_k * (x_ki * x_kj), x_k = E_h * R_r, w_k = sig'(e . x_k), summed in
                  float64 in triple order; A = H + float64(fl32(c * fl32(z_i z_j))) with
                  c = fl32(sig (1 - sig)), sig = sigmoid(e . z_t) in float32; b = z_t
  elimination     per column the pivot is the first row of maximal |a| (exactly 0: singular),
                  the multiplier a / pivot, every update a product rounded and then
                  subtracted (numpy never fuses the two), in pivot order
  back            i descending: y_i = b_i / U_ii, then b_j -= U_ji * y_i for j < i
  output          256 partial sums acc_t = sum_{j = t (mod 256)} float64(z_p[j]) * (om * y_j),
                  om = float64(fl32(1 - sig)), reduced by a halving tree 128 ... 1

With a perspective entity whose row is zero every sigmoid is exactly 0.5 and every other
operation is one IEEE operation, so the value is the device's to the last bit.  Elsewhere
the float32 dot products and exp differ from the device's in their last bits.

The value has the kernel's sign (the sufficient engine's); the necessary engine negates it.
"""
from __future__ import annotations

import numpy as np

from oracle import kelpie_oracle as ko

F32 = np.float32


def sigmoid32(x):
    """The float32 sigmoid of the kernels: 1 / (1 + exp(-x))."""
    return F32(1) / (F32(1) + np.exp(-F32(x), dtype=F32))


def hessian(om, entity, tail_triples):
    """H_e in float64 from float32 terms, in triple order; also the weights w_k."""
    e = om.E[entity]
    D = om.E.shape[1]
    H = np.zeros((D, D))
    ws = []
    for s, p, _ in tail_triples:
        x = (om.E[s] * om.R[p]).astype(F32)
        sg = sigmoid32(np.dot(e, x))
        w = F32(sg * (F32(1) - sg))
        ws.append(w)
        H += (w * (x[:, None] * x[None, :]).astype(F32)).astype(F32).astype(np.float64)
    return H, np.asarray(ws, F32)


def eliminate(A, b, pivot=True):
    """Unblocked Gaussian elimination with partial pivoting of A y = b (float64).
    Returns (y or None when a pivot is exactly 0, columns that swapped, swaps whose two
    rows sit in different 64-row groups counted from the first row of the column's
    32-column panel).  ``pivot=False`` never swaps (and divides by whatever the diagonal
    holds): it only serves to show which inputs can tell the two apart."""
    A = np.array(A, dtype=np.float64)
    b = np.array(b, dtype=np.float64)
    D = len(b)
    swaps = cross = 0
    with np.errstate(all="ignore"):
        for j in range(D):
            p = j + int(np.argmax(np.abs(A[j:, j]))) if pivot else j  # argmax: the first maximum
            if A[p, j] == 0.0:
                return None, swaps, cross
            if p != j:
                A[[j, p]] = A[[p, j]]
                b[[j, p]] = b[[p, j]]
                swaps += 1
                k0 = j // 32 * 32
                cross += int((p - k0) // 64 != (j - k0) // 64)
            mult = A[j + 1:, j] / A[j, j]
            A[j + 1:, j + 1:] -= mult[:, None] * A[j, j + 1:][None, :]
            b[j + 1:] -= mult * b[j]
        for i in range(D - 1, -1, -1):
            b[i] = b[i] / A[i, i]
            b[:i] -= A[:i, i] * b[i]
    return b, swaps, cross


def output(z_p, y, om):
    """z_p . (om y) in the kernel's fixed order."""
    D = len(y)
    acc = np.zeros(256)
    for t in range(min(256, D)):
        for j in range(t, D, 256):
            acc[t] += np.float64(z_p[j]) * (om * y[j])
    s = 128
    while s > 0:
        acc[:s] += acc[s:2 * s]
        s //= 2
    return float(acc[0])


def variation(om, H, entity, z_p, z_t, pivot=True):
    """(value or None, swapped columns, cross-group swaps) of one candidate."""
    z_p = np.asarray(z_p, F32).reshape(-1)
    z_t = np.asarray(z_t, F32).reshape(-1)
    sig = sigmoid32(np.dot(om.E[entity], z_t))
    c = F32(sig * (F32(1) - sig))
    A = H + (c * (z_t[:, None] * z_t[None, :]).astype(F32)).astype(F32).astype(np.float64)
    y, swaps, cross = eliminate(A, z_t.astype(np.float64), pivot)
    if y is None:
        return None, swaps, cross
    return output(z_p, y, np.float64(F32(F32(1) - sig))), swaps, cross


class Plain:
    """criage_plain over one model and one tail index, Hessians kept per entity."""

    def __init__(self, om, tails):
        self.om = om
        self.tails = tails
        self._H = {}
        self._z = {}

    def hessian(self, ent):
        if ent not in self._H:
            self._H[ent] = hessian(self.om, ent, self.tails.get(ent, []))
        return self._H[ent]

    def z(self, s, p):
        if (s, p) not in self._z:
            self._z[(s, p)] = ko.criage_z(self.om, (s, p, 0))[0]
        return self._z[(s, p)]

    def __call__(self, pred, triple, perspective="tail", pivot=True):
        ps, pp, po = (int(v) for v in pred)
        ent = po if perspective == "tail" else ps
        if perspective == "head":
            ps, po = po, ps
        H, _ = self.hessian(ent)
        return variation(self.om, H, ent, self.z(ps, pp), self.z(int(triple[0]), int(triple[1])), pivot)


def criage_plain(om, tails, pred, triple, perspective="tail", pivot=True):
    """One candidate: (value or None, swapped columns, cross-group swaps)."""
    return Plain(om, tails)(pred, triple, perspective, pivot)
