"""Probes on the device (kp_posttrain_rank_probes) against the CPU.

1. every case of probe_cases.py: the probes change nothing else (bitwise, against the same
   call without probes on a fresh context, with k = 0 and k = 5), the own-target probe
   returns the slot's score bit for bit and its rank, and every probe is held to a float64
   numpy restatement on the returned final row under the rank rule; KP_PROBE_CHUNK=16 makes
   the 65 probes of a call cross chunks;
2. error paths leave the context usable; the fp32 rank switch refuses probes;
3. the engines end to end, and the reference fixture (tests/golden/probes_tiny.json).

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kelpie_amd as ka
import probe_cases as pc
import width_cases as wc
from golden_io import seed_all
from kelpie_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probes_tiny.json")


# ----------------------------------------------------------------------------- 1. the cases
@pytest.mark.parametrize("case", pc.CASES, ids=pc.ids())
def test_probes_vs_numpy(case, monkeypatch):
    monkeypatch.setenv("KP_PROBE_CHUNK", "16")
    call, model = pc.run(case, lambda m: m.ctx)
    s, r, x, (ps, prk) = call["out"]
    assert len(ps) == len(prk) == sum(pc.COUNTS) and call["probes"][0].tolist() == [0, 16, 16, 33, 34, 49, 65]
    # consequence 2: nothing else changes (fresh contexts)
    plain, _ = pc.run(case, lambda m: m.ctx, with_probes=False)
    for a, b in zip(call["out"][:3], plain["out"][:3]):
        assert a.tobytes() == b.tobytes()
    with5, _ = pc.run(case, lambda m: m.ctx, topk=5)
    plain5, _ = pc.run(case, lambda m: m.ctx, topk=5, with_probes=False)
    for a, b in zip(with5["out"][:3] + with5["out"][3], plain5["out"][:3] + plain5["out"][3]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(with5["out"][:3] + with5["out"][4], call["out"][:3] + call["out"][3]):
        assert a.tobytes() == b.tobytes()  # and the lists change neither the slots nor the probes
    # consequence 1
    assert pc.check_own_target(call) == 5
    # every probe against the float64 restatement
    n, exact, sharp, widest = pc.check_probes(call, model, wc.oracle_context(model))
    print(case["id"], "probes", n, "exact ranks", exact, "sharp", sharp, "widest bounds", widest)
    assert n == 65
    # the planted kinds are there: the kelpie entity as object, an object its filter names
    p_off, tr, f_off, fl = call["probes"]
    assert tr[1, 1] == case["n_ent"] and tr[2, 1] in fl[f_off[2]:f_off[3]]


# ----------------------------------------------------------------------------- 2. error paths
def _raw_call(ctx, args, probes, nulls=()):
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = args
    n = len(row_off) - 1
    keep = [np.ascontiguousarray(x0, np.float32), np.ascontiguousarray(row_off, np.int32),
            np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(rng_off, np.int64),
            np.ascontiguousarray(rng, np.int32), np.ascontiguousarray(pred, np.int32),
            np.ascontiguousarray(filt_off, np.int32), np.ascontiguousarray(filt, np.int32),
            np.zeros(n, np.float32), np.zeros(n, np.int64)]
    p = [_lib._ptr(a) for a in keep]
    b = _lib.Batch(n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], None, p[8], p[9])
    if probes is None:
        return _lib.lib().kp_posttrain_rank_probes(ctx.h, C.byref(hp), C.byref(b), 0, None, None, None), None
    p_off, tr, f_off, fl = [np.ascontiguousarray(a, np.int32) for a in probes]
    m = len(tr)
    out = [np.zeros(m, np.float32), np.zeros(m, np.int64)]
    ptrs = {"probe_off": p_off, "probes": tr, "filt_off": f_off, "filt": fl, "out_score": out[0], "out_rank": out[1]}
    pr = _lib.Probes(m, *[None if k in nulls else _lib._ptr(a) for k, a in ptrs.items()])
    return _lib.lib().kp_posttrain_rank_probes(ctx.h, C.byref(hp), C.byref(b), 0, None, None, C.byref(pr)), out


def _direct(family="DistMult"):
    m, d = {"DistMult": ("DistMult", 40), "ConvE": ("ConvE", 60), "TransE": ("TransE", 50)}[family]
    case = dict(wc._case(m, d, tag="nq16"), nq=16)  # two slots
    model = wc.make_model(case)
    args = wc.query_batch(case, model)
    K = model.dataset.num_entities
    probes = (np.array([0, 2, 3]), np.array([[0, 5], [3, K], [1, 7]]), np.array([0, 1, 1, 3]), np.array([5, 2, K]))
    return model, args, probes


def test_malformed_probes_leave_the_context_usable():
    model, args, probes = _direct()
    ctx, K = model.ctx, model.dataset.num_entities
    good = ctx.posttrain_rank(*args, probes=probes)
    EINVAL = -22
    p_off, tr, f_off, fl = probes
    bad = [(np.array([1, 2, 3]), tr, f_off, fl), (np.array([0, 3, 2]), tr, f_off, fl),
           (np.array([0, 2, 2]), tr, f_off, fl), (p_off, np.array([[0, 5], [3, K + 1], [1, 7]]), f_off, fl),
           (p_off, np.array([[0, 5], [-1, K], [1, 7]]), f_off, fl), (p_off, tr, np.array([0, 2, 1, 3]), fl),
           (p_off, tr, np.array([1, 1, 1, 3]), fl), (p_off, tr, f_off, np.array([5, 2, K + 1]))]
    for b in bad:
        rc, out = _raw_call(ctx, args, b)
        assert rc == EINVAL and not out[0].any() and not out[1].any(), b
        assert b"probes" in _lib.lib().kp_last_error(ctx.h)
    for null in ("probe_off", "probes", "filt_off", "filt", "out_score", "out_rank"):
        assert _raw_call(ctx, args, probes, nulls=(null,))[0] == EINVAL, null
    assert _raw_call(ctx, args, None)[0] == 0  # no probes: kp_posttrain_rank_topk
    again = ctx.posttrain_rank(*args, probes=probes)
    for a, b in zip(good[:2] + good[3], again[:2] + again[3]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("family,var", [("TransE", "KP_TE_RANK"), ("ConvE", "KP_CV_RANK")])
def test_fp32_rank_switch_refuses_probes(family, var, monkeypatch):
    monkeypatch.setenv(var, "f32")  # read when the context is created
    model, args, probes = _direct(family)
    ctx = model.ctx
    monkeypatch.delenv(var)
    with pytest.raises(_lib.KelpieHipError, match="-95"):
        ctx.posttrain_rank(*args, probes=probes)
    s, r, _ = ctx.posttrain_rank(*args)  # the fp32 rank itself still runs
    assert len(s) == len(r) == 2 and (r >= 1).all()


# ----------------------------------------------------------------------------- 3. the engines
@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
@pytest.mark.parametrize("family", ["ComplEx-d32-n257", "TransE-L2-d50-n257"])
def test_engine_side_effects(family, mode):
    """compute_side_effects on the device: the relevances and generator states of
    compute_relevance_batch, and the own-target probe equal to the slot's own result
    (TransE: the library's scheduler makes the slot's filter, Python the probe's)."""
    import torch
    case = next(c for c in pc.CASES if c["id"] == family)
    ds, preds = pc.graph(case["n_ent"])
    pred = preds[0]
    rules = [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]
    cls = ka.NecessaryPostTrainingEngine if mode == "necessary" else ka.SufficientPostTrainingEngine
    ents = [e for e in range(ds.num_entities) if e != pred[0] and ds.entity_to_degree.get(e, 0) >= 2][:2]

    def engine():
        seed_all(42)
        eng = cls(pc.make_model(case), ds, pc.hp_of(case))
        if mode == "sufficient":
            eng.entities_to_convert = ents
        return eng

    want = engine().compute_relevance_batch(pred, rules)
    state = torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes()
    probes = [pred] + pc.graph(case["n_ent"])[0].entity_to_training_triples[pred[0]][:3]
    eng = engine()
    out = eng.compute_side_effects(pred, rules, probes=probes)
    assert (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes()) == state
    assert [o["relevance"] for o in out] == want
    for o in out:
        for side in ([o] if mode == "necessary" else o["conversions"]):
            for res in (side["base"], side["post"]):
                assert len(res["probes"]) == 4
                own = res["probes"][0]
                assert own["score"] == res["score"] and own["rank"] == res["rank"], (own, res)


def test_reference_fixture_on_the_device():
    import probe_golden as pg
    with open(GOLDEN) as f:
        golden = json.load(f)
    for rec in golden["cases"]:
        n = pg.compare(rec, pg.replay(rec, lambda m: m.ctx))
        print(rec["name"], rec["mode"], "probes reproduced", n)
