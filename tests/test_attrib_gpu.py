"""Attributions on the device (kp_posttrain_rank_attrib) against themselves and the definition.

Shapes: attrib_cases.py's batches -- 517 entities (17 key tiles, 5 entities in the last), 8
epochs; per case two ordinary subjects x (base + two candidates) in one step per epoch and the
hub subject's base + two candidates in three and two steps per epoch (plans per step, slots that
end at different steps); ComplEx d = 32 (DB 4) and 200 (DB 25), DistMult d = 40 (DB 4) and 200
(DB 13); Adagrad with none / N3 / N2, and SGD -- and the crafted batches at a row width of 24
(a self-loop row, an empty slot, a repeated relation and pair, a duplicate row, a one-slot launch).

Asserted:
1. with attributions every other output of the call (scores, ranks, rows, lists, probes, trace,
   marks, margins) is bitwise what it is without;
2. a fresh context gives the same attributions bitwise;
3. ``epochs`` = 0 gives zeros;
4. completeness, per slot: |sum_i (fit_i + reg_i) - delta| <= R_C S, S = sum_i (|fit_i| + |reg_i|)
   (R_C: attrib_cases.py, from the float32-emulating restatement x 8);
5. per row against the float32-emulating restatement fed the same draws: |dev - ref| <= 1e-4 S,
   the project's row rule (test_gpu_widths.py asserts it for returned rows; an attribution is
   those same updates projected on c);
6. ``delta`` recomputed in numpy from x0 and the returned rows, to float64 rounding;
7. the engines' ``compute_attributions`` and ``rank_facts`` on the device, ComplEx d = 32.

Recorded on an MI355X, not asserted: the largest per-row error 2.5e-6 S and
the largest completeness residual 4.2e-8 S.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import functools

import numpy as np
import pytest

import attrib_cases as ac
import attrib_reference as ar
import kelpie_amd as ka
import margins_cases as gc
import width_cases as wc
from golden_io import seed_all

pytestmark = pytest.mark.gpu

ALL = ac.ids(ac.CASES) + ["crafted-ComplEx", "crafted-DistMult"]


@functools.lru_cache(maxsize=None)
def _device(case_id):
    """(batches, model, the device's result of every batch with attributions and rows)."""
    bs, model = ac.crafted(case_id.split("-")[1]) if case_id.startswith("crafted-") else ac.batches(case_id)
    model._ctx = None  # the device's, made on first use
    return bs, model, [model.ctx.posttrain_rank(*b, want_x=True, attrib=True) for b in bs]


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _same_attrib(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case_id", ALL)
def test_nothing_else_moves_and_reruns(case_id):
    bs, model, outs = _device(case_id)
    for args, first in zip((bs[0], bs[-1]) if len(bs) > 1 else bs, (outs[0], outs[-1])):
        E = int(args[0].epochs)
        kw = {"topk": 5, "probes": gc.own_probes(args, copies=2), "trace": True, "marks": [0, 3, E], "margins": gc.TOL}
        plain = model.ctx.posttrain_rank(*args, want_x=True, **kw)
        with_a = model.ctx.posttrain_rank(*args, want_x=True, attrib=True, **kw)
        assert len(with_a) == len(plain) + 1
        s, r, x, (ids, top), (ps, pr), losses, (ms, mrk, mx), margins = plain
        s2, r2, x2, (ids2, top2), (ps2, pr2), losses2, (ms2, mrk2, mx2), margins2 = with_a[:-1]
        for a, c in ((s, s2), (r, r2), (x, x2), (ids, ids2), (top, top2), (ps, ps2), (pr, pr2), (ms, ms2), (mrk, mrk2),
                     (mx, mx2)):
            assert _same(a, c)
        assert len(losses) == len(losses2) and all(_same(a, c) for a, c in zip(losses, losses2))
        for a, c in zip(margins, margins2):
            assert all(_same(a[f], c[f]) for f in a)
        # the attributions do not depend on the other requests, and the bare call returned the same rows
        assert _same_attrib(with_a[-1], first[-1])
        assert all(_same(a, c) for a, c in zip(first[:3], plain[:3]))
        # 2. a fresh context
        again = model._make_ctx().posttrain_rank(*args, want_x=True, attrib=True)
        assert _same_attrib(again[-1], first[-1]) and _same(again[2], x)


@pytest.mark.parametrize("case_id", ALL)
def test_against_the_definition(case_id):
    bs, model, outs = _device(case_id)
    refs = ac.reference(case_id, "f32")
    prod = ac.product_of(model)
    E64, R64 = model.entity_embeddings.astype(np.float64), model.relation_embeddings.astype(np.float64)
    worst_row = worst_c = 0.0
    for args, out, ref in zip(bs, outs, refs):
        _, x0, row_off, _, _, _, pred = args[:7]
        x = out[2]
        fit, reg, delta = out[-1]
        assert len(fit) == len(reg) == row_off[-1] and len(delta) == len(row_off) - 1
        for s in range(len(row_off) - 1):
            a, z = int(row_off[s]), int(row_off[s + 1])
            # 6. delta from the returned rows
            c = ar.score_gradient(prod, E64, R64, int(pred[s][1]), int(pred[s][2]))
            terms = c * (x[s].astype(np.float64) - np.asarray(x0[s], np.float32).astype(np.float64))
            assert abs(delta[s] - terms.sum()) <= 2 * (len(c) + 2) * 2.0 ** -53 * np.abs(terms).sum() + 1e-300
            if a == z:  # an empty slot: nothing to write, and its row did not move
                assert delta[s] == 0.0 and _same(x[s], np.asarray(x0[s], np.float32))
                continue
            S = ac.slot_scale(ref[0], ref[1], row_off, s)
            # 4. completeness
            resid = abs(float((fit[a:z] + reg[a:z]).sum()) - float(delta[s]))
            print(f"{case_id} slot {s}: completeness residual {resid / S:.2e} S (R_C {ac.R_C:.2e})")
            worst_c = max(worst_c, resid / S)
            assert resid <= ac.R_C * S, (s, resid / S)
            # 5. per row
            err = max(float(np.abs(fit[a:z] - ref[0][a:z]).max()), float(np.abs(reg[a:z] - ref[1][a:z]).max()))
            worst_row = max(worst_row, err / S)
            assert err <= ac.ROW_TOL * S, (s, err / S)
            assert abs(delta[s] - ref[2][s]) <= ac.ROW_TOL * S
            if float(args[0].reg_weight) == 0:
                assert not reg[a:z].any()
            else:
                assert reg[a:z].all()
    print(f"{case_id}: largest per-row error {worst_row:.2e} S, largest completeness residual {worst_c:.2e} S")


@pytest.mark.parametrize("case_id", ["ComplEx-d32-DB4-Adagrad-N3", "DistMult-d200-DB13-Adagrad-none"])
def test_epochs_zero(case_id):
    bs, model, _ = _device(case_id)
    for args in (bs[0], bs[-1]):
        hp0 = type(args[0]).from_buffer_copy(args[0])
        hp0.epochs = 0
        s, r, x, (fit, reg, delta) = model.ctx.posttrain_rank(hp0, *args[1:], want_x=True, attrib=True)
        assert not fit.any() and not reg.any() and not delta.any() and len(fit) == args[2][-1]
        assert _same(x, np.asarray(args[1], np.float32))


@pytest.mark.parametrize("prod", ["ComplEx", "DistMult"])
def test_crafted_rows(prod):
    """Duplicate rows: equal in one step per epoch, parted by the permutations otherwise; the
    one-slot launch is the first slot of the three-slot launch."""
    bs, model, outs = _device(f"crafted-{prod}")
    (fit3, reg3, _), (fitm, _, _), (fit1, reg1, delta1) = (o[-1] for o in outs)
    assert fit3[0] == fit3[5] and reg3[0] == reg3[5] and fit3[3] == fit3[6]
    assert fit1[0] == fit1[5] and fit1[3] == fit1[6]
    assert fitm[0] != fitm[5] and fitm[3] != fitm[6]
    S = ac.slot_scale(fit1, reg1, bs[2][2], 0)
    assert np.abs(fit1 - fit3[:8]).max() <= ac.ROW_TOL * S and np.abs(reg1 - reg3[:8]).max() <= ac.ROW_TOL * S
    # the self-loop row holds the kelpie twice: twice the regulariser's share of a single row
    assert reg1[4] == 2 * reg1[0] != 0


def test_refusals_on_the_device():
    """Adam and a kelpie tail are refused by the library, and the context serves the next call."""
    bs, model, outs = _device("ComplEx-d32-DB4-Adagrad-none")
    args = bs[0]
    adam = type(args[0]).from_buffer_copy(args[0])
    adam.optimizer = 1
    with pytest.raises(Exception, match="not offered with Adam"):
        model.ctx.posttrain_rank(adam, *args[1:], attrib=True)
    pred = np.array(args[6]).copy()
    pred[1][2] = model.dataset.num_entities
    with pytest.raises(Exception, match="quadratic in the row"):
        model.ctx.posttrain_rank(*args[:6], pred, *args[7:], attrib=True)
    again = model.ctx.posttrain_rank(*args, want_x=True, attrib=True)
    assert _same_attrib(again[-1], outs[0][-1])


# ----------------------------------------------------------------------------- the engines on the device
@pytest.mark.parametrize("draws", ["reference", "keyed"])
@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
def test_engine_reports(mode, draws):
    """compute_attributions on the device, ComplEx d = 32 with N3: the relevances are
    compute_relevance_batch's bit for bit (the same seeds, or the same keys), every side is
    complete and score0 + delta is its score; rank_facts orders the base slot's facts."""
    case = ac.CASES[1]
    ds, ordinary = wc.graph(case["n_ent"])[1:3]
    pred = ordinary[0]
    rules = [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]
    cls = ka.NecessaryPostTrainingEngine if mode == "necessary" else ka.SufficientPostTrainingEngine
    outs, engines = [], []
    for attrib in (False, True):
        model = wc.make_model(case)
        seed_all(42)
        eng = cls(model, ds, ac.hp_of(case))
        if draws == "keyed":
            eng.draws, eng.seed = "keyed", 7
        if mode == "sufficient":
            eng.entities_to_convert = [int(p[0]) for p in ordinary if p[0] != pred[0]][:2]
        outs.append(eng.compute_attributions(pred, rules) if attrib else eng.compute_relevance_batch(pred, rules))
        engines.append(eng)
    plain, rep = outs
    assert [o["relevance"] for o in rep] == plain
    for o in rep:
        sides = [o["base"], o["post"]] if mode == "necessary" else [c[k] for c in o["conversions"] for k in ("base", "post")]
        for side in sides:
            S = sum(abs(f["fit"]) + abs(f["reg"]) for f in side["facts"])
            assert abs(sum(f["fit"] + f["reg"] for f in side["facts"]) - side["delta"]) <= ac.R_C * S
            assert side["score0"] + side["delta"] == side["score"] and S > 0
    if mode == "necessary":
        eng = engines[1]
        ranked = eng.rank_facts(pred)
        assert sorted(f["triple"] for f in ranked) == sorted(ds.entity_to_training_triples[pred[0]])
        fits = [f["fit"] for f in ranked]
        assert fits == sorted(fits, reverse=True) and eng.rank_facts(pred, k=2) == ranked[:2]
        # the cached base of compute_attributions is the one rank_facts reads
        base = rep[0]["base"]["facts"]
        assert sorted(ranked, key=lambda f: f["triple"]) == sorted(base, key=lambda f: f["triple"])
