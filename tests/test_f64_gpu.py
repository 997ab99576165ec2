"""GPU: kp_posttrain_rank_f64 and ``engine.precision = "fp64"`` against the float64 restatement
(f64_reference.py) and the reference's own fp64 runs.

Per slot of every case (f64_cases.py; shapes of width_cases.py): the score within TOL_F64 *
max(1, |ref|), the final row within TOL_F64 of its largest magnitude, the rank inside the
derived bound [#{s_e >= t + delta}, #{s_e >= t - delta}], delta = TOL_F64 * max(1, |t|), on
the restatement's scores -- a single rank for every slot (test_f64_cpu.py shows it).  TOL_F64
is 8 x the distance measured on the CPU between the restatement and the reference's fp64 run
(f64_reference.py); nothing here widens it.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import json
import os

import numpy as np
import pytest

import distmult_backend as dmb
import f64_cases as fc
import f64_reference as fr
import kelpie_amd as ka
import test_reg_fullwidth as reg_fw
import width_cases as wc
from f64_backend import F64Recording, check_slots
from golden_io import seed_all

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _device(model):
    return F64Recording(model.ctx)


def _hold(case):
    got = fc.run(case, _device)
    exact, ws, wx = check_slots(got, fc.reference(case))
    print(f"{case['id']}: exact ranks {exact}/{len(got)}, score error {ws:.2e}, row error {wx:.2e} "
          f"(TOL_F64 {fr.TOL_F64:.2e})")
    assert exact == len(got)
    return got


# ----------------------------------------------------------------------------- widths
@pytest.mark.parametrize("case", fc.WIDTHS, ids=wc.ids(fc.WIDTHS))
def test_width_vs_restatement(case):
    _hold(case)


# ----------------------------------------------------------------------------- shape edges
@pytest.mark.parametrize("case", fc.KEYS, ids=wc.ids(fc.KEYS))
def test_key_count_edges(case):
    _hold(case)


@pytest.mark.parametrize("case", fc.QUERIES, ids=wc.ids(fc.QUERIES))
def test_query_count_edges(case):
    model = wc.make_model(case)
    dev = F64Recording(model.ctx)
    dev.posttrain_rank_f64(*fc.query_args(case, model), want_x=True)
    assert model.ctx.last_attn_plan()["attn_queries"] == case["nq"], model.ctx.last_attn_plan()
    check_slots(dev.slots, fc.reference(case))


@pytest.mark.parametrize("case", fc.RANGES, ids=wc.ids(fc.RANGES))
def test_forced_key_ranges_merge(case, monkeypatch):
    """KP_ATTN_RANGES at context creation, as test_gpu_attn_ranges.py forces it: the fp64
    partials of 1, 3 and 9 (+ 7 empty) key ranges merged by log-sum-exp in range order."""
    monkeypatch.setenv("KP_ATTN_RANGES", str(case["ranges"]))
    got = fc.run(case, lambda m: F64Recording(m.ctx))  # the context is created under the variable
    check_slots(got, fc.reference(case))
    m2 = wc.make_model(case)
    dev = F64Recording(m2.ctx)
    qc = dict(case, nq=17)
    dev.posttrain_rank_f64(*fc.query_args(qc, m2), want_x=True)
    assert m2.ctx.last_attn_plan()["attn_ranges"] == case["ranges"], m2.ctx.last_attn_plan()


@pytest.mark.parametrize("case", fc.HUB, ids=wc.ids(fc.HUB))
def test_hub_with_several_minibatches(case):
    _hold(case)


@pytest.mark.parametrize("case", fc.CRAFTED, ids=wc.ids(fc.CRAFTED))
def test_crafted_batch(case):
    """A self-loop, a kelpie object, a repeated pair; the slot without rows returns x0's
    result: its row bit for bit, and the score and rank the restatement gives x0."""
    model = wc.make_model(case)
    args = fc.crafted_args(model)
    dev = F64Recording(model.ctx)
    dev.posttrain_rank_f64(*args, want_x=True)
    check_slots(dev.slots, fc.reference(case))
    assert np.array_equal(dev.slots[1]["x"], args[1][1])


# ----------------------------------------------------------------------------- reference goldens
@pytest.mark.parametrize("reg", reg_fw.REGS)
def test_reg_fullwidth_equals_reference_fp64(reg):
    """Every rank of the regularised full-width case equals the reference's fp64 run, the
    flagged N3 element included; scores within TOL_F64."""
    rec, ds, w = reg_fw._case()
    hp = dict(rec["hp"]) if reg == "none" else dict(rec["hp"], regularizer_name=reg, regularizer_weight=0.05)
    model = ka.ComplEx(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=rec["init_scale"])
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    eng.precision = "fp64"
    got = []
    for pred, cands in zip(rec["preds"], rec["candidates"]):
        eng.set_cache()
        eng.compute_relevance_batch(tuple(pred), [[tuple(c)] for c in cands])
        got += [(pt["target_rank"], pt["target_score"], b["target_rank"], b["target_score"])
                for pt, b in eng.last_results]
    r64 = reg_fw._ref(rec, reg, "fp64")
    worst = max(max(abs(g[k] - b[k]) / max(1.0, abs(b[k])) for k in (1, 3)) for g, b in zip(got, r64))
    print(json.dumps({"reg": reg, "gpu_fp64": got, "ref_fp64": r64, "worst_score_error": worst}))
    assert len(got) == len(r64) == 12
    for g, b in zip(got, r64):
        assert g[0] == b[0] and g[2] == b[2], (reg, g, b)
    assert worst <= fr.TOL_F64, worst


def test_distmult_fixture_fp64_runs():
    rec, ds, model = dmb.load_fixture()
    x0 = model.kelpie_init64(np.asarray(rec["init"], np.float32), None)
    trip = np.asarray(rec["kelpie_training_triples"], np.int64)
    rows = np.vstack([trip, ds.invert_triples(trip)])
    for slot in rec["slots"]:
        perms = np.asarray(slot["perms"], np.int32).reshape(-1) if slot["perms"] else np.zeros(0, np.int32)
        filt = np.asarray(slot["filter"], np.int64)
        sc, rk, x = model.ctx.posttrain_rank_f64(model.kp_hp64(slot["hp"]), x0[None], np.array([0, len(rows)]), rows,
                                                 np.array([0, len(perms)]), perms, np.array([slot["kelpie_triple"]]),
                                                 np.array([0, len(filt)]), filt, want_x=True)
        f64 = slot["fp64"]
        row = np.asarray(f64["row"])
        es = abs(float(sc[0]) - f64["score"]) / max(1.0, abs(f64["score"]))
        ex = float(np.abs(x[0] - row).max() / np.abs(row).max())
        print(f"{slot['name']}: rank {int(rk[0])} ref {f64['rank']}, score error {es:.2e}, row error {ex:.2e}")
        assert int(rk[0]) == f64["rank"]
        assert es <= fr.TOL_F64 and ex <= fr.TOL_F64


def test_fullsize_fixture_rank_deltas_equal_fp64():
    """complex-fb15k237-necessary__p0: every rank delta equals the reference's fp64 run's."""
    import bench
    with open(os.path.join(HERE, "golden", "fullsize", "complex-fb15k237-necessary__p0.json")) as f:
        fx = json.load(f)
    wl = bench.WORKLOADS[fx["workload"]]
    ds, model, _ = bench.build(wl, 0, 0)
    eng = ka.NecessaryPostTrainingEngine(model, ds, wl["hp"])
    eng.precision = "fp64"
    _, _, _, par = bench.parity_sample(eng, wl, fx, None)
    print(json.dumps({"gpu_fp64": par["gpu_rank_deltas"], "ref_fp64": fx["runs"]["fp64"]["rank_deltas"],
                      "ref_fp32": fx["runs"]["fp32"]["rank_deltas"]}))
    assert par["gpu_rank_deltas"] == fx["runs"]["fp64"]["rank_deltas"]


# ----------------------------------------------------------------------------- repeatability
REP = fc.WIDTHS[2]  # ComplEx d = 100


def _batch(model, case=REP):
    return fc.query_args(dict(case, nq=17), model)


def test_two_fresh_contexts_are_bitwise_equal():
    outs = []
    for _ in range(2):
        model = wc.make_model(REP)
        outs.append(model.ctx.posttrain_rank_f64(*_batch(model), want_x=True))
        model.ctx.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.abs(outs[0][2]).max() > 0


def test_fp32_results_are_unchanged_by_an_fp64_call():
    """An fp32 batch before and after an fp64 call on one context, and on a fresh context:
    bitwise equal (the fp64 call has workspaces of its own)."""
    c32 = dict(REP, nq=17)
    model = wc.make_model(REP)
    a32 = wc.query_batch(c32, model)
    before = model.ctx.posttrain_rank(*a32, want_x=True)
    model.ctx.posttrain_rank_f64(*_batch(model), want_x=True)
    after = model.ctx.posttrain_rank(*a32, want_x=True)
    fresh_model = wc.make_model(REP)
    fresh = fresh_model.ctx.posttrain_rank(*a32, want_x=True)
    for a, b, c in zip(before, after, fresh):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ----------------------------------------------------------------------------- errors
def _cx_args(n_ent=40, d=8, nr=4):
    rows = np.array([[n_ent, 1, 3], [3, 1 + nr, n_ent]], np.int32)
    hp = ka._lib.HP(optimizer=0, epochs=2, batch_size=64, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-10)
    hp64 = ka._lib.HP64(hp, 0.01, 0.9, 0.999, 1e-10, 0.0)
    return (hp64, np.full((1, d), 0.1), [0, 2], rows, [0, 0], np.zeros(1, np.int32), np.array([[n_ent, 1, 3]]),
            [0, 0], np.zeros(1, np.int32))


def test_other_families_are_not_supported_and_stay_usable():
    rng = np.random.default_rng(0)
    E, R = rng.standard_normal((40, 60)).astype(np.float32), rng.standard_normal((8, 60)).astype(np.float32)
    d = 60
    hid = 32 * 38 * (d // 20 - 2)
    conve = {"conv_w": np.zeros((32, 9), np.float32), "conv_b": np.zeros(32, np.float32),
             "fc_w": np.zeros((d, hid), np.float32), "fc_b": np.zeros(d, np.float32),
             "bn_alpha": np.ones(33 + d, np.float32), "bn_beta": np.zeros(33 + d, np.float32)}
    for ctx in (ka._lib.Context("TransE", E, R, norm_p=2), ka._lib.Context("ConvE", E, R, conve=conve)):
        with pytest.raises(ka._lib.KelpieHipError, match=r"error -95.*fp64"):
            ctx.posttrain_rank_f64(*_cx_args(d=d))
        got = ctx.all_scores(np.array([1, 2]), np.array([0, 5]))
        assert got.shape == (2, 40) and np.isfinite(got).all()


def test_null_buffers_are_invalid_and_the_context_stays_usable():
    import ctypes as C
    L = ka._lib
    rng = np.random.default_rng(0)
    E, R = rng.standard_normal((40, 8)).astype(np.float32), rng.standard_normal((8, 8)).astype(np.float32)
    ctx = L.Context("ComplEx", E, R)
    hp64, x0, row_off, rows, rng_off, draws, pred, filt_off, filt = _cx_args()
    good = ctx.posttrain_rank_f64(hp64, x0, row_off, rows, rng_off, draws, pred, filt_off, filt, want_x=True)
    arrs = [np.ascontiguousarray(a, dtype=t) for a, t in ((row_off, np.int32), (rows, np.int32), (rng_off, np.int64),
                                                          (draws, np.int32), (pred, np.int32), (filt_off, np.int32),
                                                          (filt, np.int32))]
    out_r, out_s, x0c = np.zeros(1, np.int64), np.zeros(1, np.float64), np.ascontiguousarray(x0, np.float64)
    b = L.Batch(1, None, *[L._ptr(a) for a in arrs], None, None, L._ptr(out_r))
    for x0p, sp in ((None, L._ptr(out_s)), (L._ptr(x0c), None)):
        r = L.F64(x0p, 0.01, 0.9, 0.999, 1e-10, 0.0, None, sp)
        assert L.lib().kp_posttrain_rank_f64(ctx.h, C.byref(hp64.hp), C.byref(b), C.byref(r)) == -22
    assert L.lib().kp_posttrain_rank_f64(ctx.h, C.byref(hp64.hp), C.byref(b), None) == -22
    again = ctx.posttrain_rank_f64(hp64, x0, row_off, rows, rng_off, draws, pred, filt_off, filt, want_x=True)
    for a, c in zip(good, again):
        assert np.array_equal(a, c)
