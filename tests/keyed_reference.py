"""Keyed draws restated in numpy from their definition (include/kelpie_hip.h, "Keyed draws"),
not from the library's C++: the reference the native driver, the device kernels and the CPU
stand-in are compared with.

Philox4x32-10, vectorised over counters; word ``w`` of stream ``s``, epoch ``e`` under key
``k`` is lane ``w % 4`` of ``Philox((w // 4, e, s, 0), (lo32(k), hi32(k)))``."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
X0, PERM, NEG, HOT = 0, 1, 2, 3


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (arrays or scalars, broadcast) under the key (k0, k1):
    four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(key, stream, epoch, n):
    """Words [0, n) of a stream: uint32 [n]."""
    key = int(key)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    lanes = philox(q, epoch, stream, 0, key & 0xFFFFFFFF, key >> 32)
    return np.stack(lanes, axis=1).reshape(-1)[:n]


def x0_uniform(init_key, dim, init_scale):
    """ComplEx / DistMult: float32(word >> 8) * 2^-24, then * init_scale in float32."""
    u = (words(init_key, X0, 0, dim) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u * np.float32(init_scale)).astype(np.float32)


def x0_normal(init_key, dim, std):
    """TransE: Box-Muller in float64 on words (2 i, 2 i + 1), rounded once to float32."""
    w = words(init_key, X0, 0, 2 * dim).astype(np.float64).reshape(dim, 2)
    u1 = (w[:, 0] + 1.0) * 2.0 ** -32
    u2 = w[:, 1] * 2.0 ** -32
    std = float(np.float32(std))
    return ((std * np.sqrt(-2.0 * np.log(u1))) * np.cos(2.0 * np.pi * u2)).astype(np.float32)


def permutation(slot_key, epoch, R):
    """Stable ascending argsort of the epoch's key words."""
    return np.argsort(words(slot_key, PERM, epoch, R), kind="stable").astype(np.int32)


def negatives(slot_key, epoch, R, n):
    return ((words(slot_key, NEG, epoch, R).astype(np.uint64) * np.uint64(n)) >> S32).astype(np.int32)


def head_or_tail(slot_key, epoch, R):
    return (words(slot_key, HOT, epoch, R) >> np.uint32(31)).astype(np.int32)


def rng_words(model_name, R, epochs, batch_size):
    """The slot's word count in kp_batch.rng's layout."""
    if model_name == "TransE":
        return epochs * 3 * R
    return epochs * R if R > batch_size else 0


def slot_rng(model_name, slot_key, R, epochs, batch_size, n=0):
    """One slot's words: TransE epochs x [order | negatives | head_or_tail]; ComplEx /
    DistMult epochs x permutation when R > batch_size, else nothing."""
    if rng_words(model_name, R, epochs, batch_size) == 0:
        return np.zeros(0, np.int32)
    parts = []
    for e in range(epochs):
        parts.append(permutation(slot_key, e, R))
        if model_name == "TransE":
            parts += [negatives(slot_key, e, R, n), head_or_tail(slot_key, e, R)]
    return np.concatenate(parts).astype(np.int32)


def slot_x0(model_name, init_key, dim, scale):
    return x0_normal(init_key, dim, scale) if model_name == "TransE" else x0_uniform(init_key, dim, scale)


def batch_draws(model_name, dim, epochs, batch_size, row_off, init_keys, slot_keys, scale, n=0):
    """(x0 [ns][dim], rng_off int64 [ns + 1], rng int32) of a batch: kp_keyed_draws' outputs."""
    ns = len(row_off) - 1
    x0 = np.zeros((ns, dim), np.float32)
    parts, off = [], np.zeros(ns + 1, np.int64)
    for s in range(ns):
        R = int(row_off[s + 1] - row_off[s])
        x0[s] = slot_x0(model_name, init_keys[s], dim, scale)
        parts.append(slot_rng(model_name, slot_keys[s], R, epochs, batch_size, n))
        off[s + 1] = off[s] + parts[-1].size
    rng = np.concatenate(parts).astype(np.int32) if parts and off[-1] else np.zeros(0, np.int32)
    return x0, off, rng


def ulp_distance(a, b):
    """Distance in float32 units in the last place, elementwise (finite inputs)."""
    def order(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(order(a) - order(b))
