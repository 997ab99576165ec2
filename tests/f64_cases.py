"""The cases of the fp64 device tests (TEST INFRASTRUCTURE), shared by test_f64_gpu.py and by
test_f64_cpu.py, which shows on the restatement (f64_reference.py) that the derived rank
bound at TOL_F64 is a single rank for every slot of every case.

The shapes are width_cases.py's: the 517-entity graph (17 key tiles of 32, 5 entities in the
last; 33 tiles of kp_attn64's 16 keys), two subjects x (base + two candidates), 8 epochs.
"""
from __future__ import annotations

import numpy as np

import kelpie_amd as ka
import width_cases as wc
from f64_backend import F64Context
from golden_io import seed_all
from kelpie_amd.rng import ReferenceRNG

case = wc._case

# every DB the issue names: ComplEx 1, 4, 13, 16 (Adam, N3), 25; DistMult 2, 13, 16
WIDTHS = [
    case("ComplEx", 3, seed=8),                                                  # row 6: DB 1
    case("ComplEx", 20, seed=4),                                                 # row 40: DB 4
    case("ComplEx", 100),                                                        # row 200: DB 13
    case("ComplEx", 128, tag="Adam-N3", opt="Adam", lr=0.01, reg="N3", seed=4),  # row 256: DB 16
    case("ComplEx", 200),                                                        # row 400: DB 25
    case("DistMult", 24, seed=4),                                                # DB 2
    case("DistMult", 200, seed=4),                                               # DB 13
    case("DistMult", 256),                                                       # DB 16
]
assert [c["db"] for c in WIDTHS] == [1, 4, 13, 16, 25, 2, 13, 16]

# key-count edges: less than one 32-key tile, exactly one, one key past it, one past sixteen
KEYS = [case("ComplEx", 32, n_ent=n) for n in (31, 32, 33, 513)]
# forced key ranges (KP_ATTN_RANGES): 3 ranges of six 32-key tiles; 16 asked for on 17 tiles
# gives nine ranges of two tiles and seven empty ones
RANGES = [dict(case("ComplEx", 50, tag=f"S{s}"), ranges=s) for s in (1, 3, 16)]
# the hub subject with a batch size below its rows: several minibatches per epoch, a plan per
# (epoch, step) from the shipped permutations
HUB = [dict(case(m, d, tag="hub", hub=True), batch_size=48) for m, d in (("ComplEx", 32), ("DistMult", 40))]
# launches of exactly 1, 16, 17 and 65 queries
QUERIES = [dict(case("ComplEx", 32, tag=f"nq{nq}"), nq=nq) for nq in (1, 16, 17, 65)]
# the crafted batch of test_distmult_gpu.py
CRAFTED = [case("DistMult", 24, tag="crafted", seed=4), case("ComplEx", 32, tag="crafted")]

ALL = WIDTHS + KEYS + RANGES + HUB + QUERIES + CRAFTED


def hp_of(c):
    hp = wc.hp_of(c)
    if "batch_size" in c:
        hp["batch_size"] = c["batch_size"]
    return hp


def run_necessary(c, ctx_of):
    """width_cases.run_necessary with ``precision = "fp64"``; the context's recorded slots."""
    ds = wc.graph(c["n_ent"])[1]
    model = wc.make_model(c)
    model._ctx = ctx_of(model)
    seed_all(42)
    for pred, epochs, n in wc.subjects(c):
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(hp_of(c), epochs=epochs))
        eng.precision = "fp64"
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        eng.compute_relevance_batch(pred, [[cd] for cd in cands])
    return model.ctx.slots


def query_args(c, model):
    """width_cases.query_batch's arguments for posttrain_rank_f64: the double hyper-parameters
    and a float64 x0."""
    args = wc.query_batch(c, model)
    return (model.kp_hp64(hp_of(c)), np.asarray(args[1], np.float64)) + tuple(args[2:])


def crafted_args(model):
    """test_distmult_gpu._crafted on this graph: a self-loop (K, r, K) and its inverse; a slot
    without rows (rank only: x0's result); rows repeating one relation and one frozen (h, r)
    pair; a ranked object that is the kelpie entity."""
    K, nr, d = model.dataset.num_entities, model.dataset.num_relations, model.dimension
    rng = np.random.default_rng(5)
    x0 = (rng.random((4, d)) * 0.2).astype(np.float32).astype(np.float64)
    slots = [
        ([(K, 3, K), (K, 3, 17), (40, 5, K)], (K, 3, 17)),
        ([], (K, 2, 9)),
        ([(K, 7, 11), (K, 7, 12), (K, 7, 11), (60, 9, K), (60, 9, K), (61, 9, K)], (K, 7, 12)),
        ([(K, 1, 5), (30, 4, K)], (K, 1, K)),
    ]
    row_off, rows, pred = [0], [], []
    for trip, p in slots:
        t = np.array(trip, np.int64).reshape(-1, 3)
        inv = t[:, [2, 1, 0]].copy()
        inv[:, 1] += nr
        rows.append(np.vstack([t, inv]))
        row_off.append(row_off[-1] + 2 * len(t))
        pred.append(p)
    filt_off = np.array([0, 2, 2, 5, 5])
    filt = np.array([3, 4, 100, 101, 102], np.int64)
    hp = model.kp_hp64(dict(wc.CX_HP))
    return (hp, x0, np.array(row_off), np.vstack(rows), np.zeros(5, np.int64), np.zeros(0, np.int32), np.array(pred),
            filt_off, filt)


def run(c, ctx_of):
    """The case's fp64 slots through ``ctx_of(model)`` (the restatement's stand-in or a
    recording wrapper of the device's context)."""
    if "nq" in c or c in CRAFTED:
        model = wc.make_model(c)
        ctx = ctx_of(model)
        args = query_args(c, model) if "nq" in c else crafted_args(model)
        ctx.posttrain_rank_f64(*args, want_x=True)
        return ctx.slots
    return run_necessary(c, ctx_of)


_REF = {}


def reference(c):
    """The restatement's side of a case, computed once."""
    if c["id"] not in _REF:
        _REF[c["id"]] = run(c, F64Context)
    return _REF[c["id"]]
