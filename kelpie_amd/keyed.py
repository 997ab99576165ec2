"""Keys of the keyed draws (include/kelpie_hip.h, "Keyed draws").

In keyed mode (``engine.draws = "keyed"``) every slot's random numbers are a pure function
of two 64-bit keys, generated on the device by Philox4x32-10.  This module derives the keys;
nothing here draws a number or touches a generator.

Both keys are the first 8 bytes, read little-endian, of ``hashlib.blake2b(data,
digest_size=8)`` over a canonical encoding in which every integer is little-endian:

``init_key``
    ``b"kelpie-keyed/init\\0"`` | seed int64 | s, p, o int32

``slot_key``
    ``b"kelpie-keyed/slot\\0"`` | seed int64 | s, p, o int32 | role uint8 (0 base, 1 edited)
    | mode uint8 (0 necessary, 1 sufficient) | count uint32 | the rule's triples SORTED,
    each h, r, t int32

``(s, p, o)`` is the prediction the slot ranks in the dataset's ids: for a conversion entity
of the sufficient engine, the prediction after ``replace_entity_in_triple``, and the rule's
triples after ``replace_entity_in_triples``.  A prediction's base slot and all of its edited
slots share ``init_key``, hence the initial kelpie row (common random numbers); the order of
a rule's triples does not matter.
"""
from __future__ import annotations

import hashlib
import struct

MODES = {"necessary": 0, "sufficient": 1}
ROLE_BASE, ROLE_EDITED = 0, 1


def _digest(data: bytes) -> int:
    return int.from_bytes(hashlib.blake2b(data, digest_size=8).digest(), "little")


def _head(tag: bytes, seed: int, pred) -> bytes:
    s, p, o = (int(v) for v in pred)
    return tag + struct.pack("<qiii", int(seed), s, p, o)


def init_key(seed: int, pred) -> int:
    """The key of the initial kelpie row of every slot that ranks ``pred``."""
    return _digest(_head(b"kelpie-keyed/init\0", seed, pred))


def slot_key(seed: int, pred, role: int, mode: str, triples=()) -> int:
    """The key of a slot's epoch permutations, negatives and head-or-tail words."""
    if role not in (ROLE_BASE, ROLE_EDITED):
        raise ValueError(f"role must be 0 (base) or 1 (edited), got {role!r}")
    rule = sorted(tuple(int(v) for v in t) for t in triples)
    data = _head(b"kelpie-keyed/slot\0", seed, pred) + struct.pack("<BBI", role, MODES[mode], len(rule))
    for h, r, t in rule:
        data += struct.pack("<iii", h, r, t)
    return _digest(data)
