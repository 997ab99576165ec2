"""GPU: every compiled kernel width, and the key- and query-count edges, against the oracle.

The cases are width_cases.py's (shared with test_width_cases_cpu.py, which shows that the
rank rule below decides every one of them).  Per post-trained slot, none left out:
score within 1e-4 * max(1, |ref|); rank inside the rank rule's bounds from the oracle's own
score row (width_cases.rank_bounds); for ComplEx and DistMult the final row within 1e-4 of
its largest magnitude.  The oracle's ConvE and TransE steps are float32 with no fp64
variant to derive a row bound from, so their row error is printed, not asserted, and so is
the number of ranks that equal the oracle's (both recorded in DESIGN.md section 3).

The oracle side of a case is computed once and shared by the runs that differ only in the
attention's partition (KP_ATTN_PART) or contraction (KP_ATTN=f32, kp_attn.hpp).

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import numpy as np
import pytest

import kelpie_amd as ka
import width_cases as wc

pytestmark = pytest.mark.gpu


def _asserts_rows(case):
    return case["model"] in ("ComplEx", "DistMult")


def _hold(case, slots, what=""):
    exact, row_err = wc.check_slots(slots, wc.reference(case), rows=_asserts_rows(case))
    print(f"{case['id']}{what}: exact ranks {exact}/{len(slots)}, row error {row_err:.2e} of the row's scale; "
          f"ranks {[s['rank'] for s in slots]}")


# --------------------------------------------------------------------------- width sweep
@pytest.mark.parametrize("case,part", wc.expand_parts(wc.SWEEP))
def test_width_vs_oracle(case, part, monkeypatch):
    """Necessary mode at every compiled width: two ordinary subjects with two singleton
    candidates each on the 517-entity graph (17 key tiles, the last with 5 entities); for
    TransE d = 260 also the hub subject, whose slots have more than 682 rows and so take the
    unstaged VPL = 2 kernel where the ordinary subjects take the staged one."""
    monkeypatch.setenv("KP_ATTN_PART", part)
    slots = wc.run_necessary(case, wc.device_context)
    if case["model"] == "TransE":
        # staged (3 R <= 4 NT) or not, by the rows the oracle side saw for the same slots
        n_rows = [b["n_rows"] for b in wc.reference(case)]
        nt = case["inst"][1]
        if case["hub"]:
            assert case["inst"] == (2, 512) and min(n_rows) > 682, n_rows
        else:
            assert 3 * max(n_rows) <= 4 * nt, n_rows
    _hold(case, slots, f" [{part}]")


F32_CASES = [c for c in wc.SWEEP if c["model"] in ("ComplEx", "ConvE")]


@pytest.mark.parametrize("case", F32_CASES, ids=wc.ids(F32_CASES))
def test_width_vs_oracle_fp32_attention(case, monkeypatch):
    """The same slots through the fp32-MFMA attention (KP_ATTN=f32: kp_attn.hpp, a second
    contraction with its own per-DB dispatch), held to the same oracle record."""
    monkeypatch.setenv("KP_ATTN", "f32")
    slots = wc.run_necessary(case, wc.device_context)
    _hold(case, slots, " [KP_ATTN=f32]")


SCORE_CASES = [c for c in wc.SWEEP if not c["hub"] and c["opt"] == "Adagrad" and not c["reg"]]


@pytest.mark.parametrize("case", SCORE_CASES, ids=wc.ids(SCORE_CASES))
def test_all_scores_per_width(case):
    """kp_cx_scoreq / kp_gemm_abt, kp_te_scores and the ConvE scorer at each width: 16
    (head, relation) pairs, one inverse relation among them, within
    1e-4 * max(1, max |ref|) of the fp64 product (ComplEx, DistMult) or the oracle."""
    model = wc.make_model(case)
    heads, rels = wc.score_pairs(case)
    ref = wc.reference_scores(case, model)
    got = model.all_scores(np.stack([heads, rels, np.zeros_like(heads)], 1))
    assert got.shape == ref.shape
    err = float(np.abs(got - ref).max())
    print(f"{case['id']}: all_scores error {err:.2e}, largest |ref| {np.abs(ref).max():.3f}")
    assert err <= wc.TOL * max(1.0, float(np.abs(ref).max()))


# --------------------------------------------------------------------------- key-count edges
@pytest.mark.parametrize("case,part", wc.expand_parts(wc.EDGES))
def test_key_count_edges_vs_oracle(case, part, monkeypatch):
    """Entity tables of 31 (less than one 32-key tile), 32 and 512 (full last tile: no tile
    is masked), 33 and 513 (one entity in the last tile); ``ranges`` puts a range boundary
    on the last tile."""
    monkeypatch.setenv("KP_ATTN_PART", part)
    slots = wc.run_necessary(case, wc.device_context)
    _hold(case, slots, f" [{part}]")


# --------------------------------------------------------------------------- query-count edges
@pytest.mark.parametrize("case", wc.QUERIES, ids=wc.ids(wc.QUERIES))
def test_query_count_edges_vs_oracle(case):
    """Step launches of exactly 1, 16, 17, 64 and 65 queries (the attention's 16-query waves
    and 64-query tiles) through posttrain_rank directly."""
    model = wc.make_model(case)
    args = wc.query_batch(case, model)
    dev = wc.RecordingContext(model.ctx)
    dev.posttrain_rank(*args, want_x=True)
    assert model.ctx.last_attn_plan()["attn_queries"] == case["nq"], model.ctx.last_attn_plan()
    _hold(case, dev.slots)


# --------------------------------------------------------------------------- limits
def _tables(width, n_ent=40, n_rel2=8):
    rng = np.random.default_rng(0)
    return (rng.standard_normal((n_ent, width)).astype(np.float32),
            rng.standard_normal((n_rel2, width)).astype(np.float32))


def test_complex_row_402_is_refused():
    E, R = _tables(402)
    with pytest.raises(ka._lib.KelpieHipError, match="row width > 400 not supported"):
        ka._lib.Context("ComplEx", E, R)


def test_conve_d420_is_refused():
    d = 420
    E, R = _tables(d)
    hid = 32 * 38 * (d // 20 - 2)
    conve = {"conv_w": np.zeros((32, 9), np.float32), "conv_b": np.zeros(32, np.float32),
             "fc_w": np.zeros((d, hid), np.float32), "fc_b": np.zeros(d, np.float32),
             "bn_alpha": np.ones(33 + d, np.float32), "bn_beta": np.zeros(33 + d, np.float32)}
    with pytest.raises(ka._lib.KelpieHipError, match="row width > 400 not supported"):
        ka._lib.Context("ConvE", E, R, conve=conve)


def test_transe_d528_is_refused_before_any_launch():
    """The context exists (all_scores has no width limit); kp_posttrain_rank refuses right
    after the batch check, before its first upload, and the context stays usable."""
    d, n_ent, nr = 528, 40, 4
    E, R = _tables(d, n_ent, 2 * nr)
    ctx = ka._lib.Context("TransE", E, R, norm_p=2)
    hp = ka._lib.HP(optimizer=ka._lib.KP_OPT["Adam"], epochs=2, batch_size=64, lr=0.01, beta1=0.9, beta2=0.999,
                    eps=1e-8, reg_weight=1.0, margin=5.0, neg_ratio=5)
    rows = np.array([[n_ent, 1, 3], [3, 1 + nr, n_ent]], np.int32)
    draws = np.zeros(2 * 3 * 2, np.int32)
    with pytest.raises(ka._lib.KelpieHipError, match="dimension > 512 not supported"):
        ctx.posttrain_rank(hp, np.zeros((1, d), np.float32), [0, 2], rows, [0, len(draws)], draws,
                           np.array([[n_ent, 1, 3]]), [0, 0], np.zeros(0, np.int32))
    heads, rels = np.array([1, 2]), np.array([0, 5])
    got = ctx.all_scores(heads, rels)
    ref = np.sqrt((((E[heads] + R[rels]).astype(np.float64)[:, None, :] - E[None].astype(np.float64)) ** 2).sum(-1))
    assert np.abs(got - ref).max() <= wc.TOL * max(1.0, ref.max())
