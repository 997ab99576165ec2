"""Rank margins on the device (kp_posttrain_rank_margins) against themselves and the definition.

Shapes: margins_cases.py's batches (517 entities, two subjects x (base + two candidates), 8
epochs, one case per family at its smallest compiled width), the same batches on entity tables
of 255, 256 and 257 rows, batches of 1, 16 and 17 rank rows, a call with 3 marks and 2 probes
per slot, a filtered target, the kelpie column as the nearest competitor, and ConvE targets
whose float32 sigmoid is 1.0.

Exact checks, every family:
1. with margins every other output of the call (scores, ranks, rows, lists, probes, trace,
   marks) is bitwise what it is without;
2. a fresh context gives the same margins bitwise;
3. ``tol`` = 0 gives rank_lo == rank == rank_hi, the bands nest over tol 0 < 1e-6 < 1e-4 < 1e-2
   and hold the rank; ties, gaps and ids do not depend on tol;
4. a probe equal to its slot's own (p, o) and filter has the slot's margin, the mark at
   hp.epochs the slot's;
5. with k = 32, a probe whose object stands inside the slot's own top-k list has the list's
   neighbours as id_better / id_worse (rows without ties).

Against margins_reference.py (ComplEx, DistMult, TransE): the compared values are recomputed in
numpy float64 from the device's own returned rows; margins_cases.check_against_host states the
rule and its bound.  No more than one undecided column per row and threshold and no more than
5 % of a case's rows with any are accepted.  ConvE has no host recomputation of its device
encoder output: its evidence is the exact checks here and the stand-in suite.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import functools

import numpy as np
import pytest

import kelpie_amd as ka
import margins_cases as gc
from golden_io import seed_all
from kelpie_amd import _lib

pytestmark = pytest.mark.gpu

FIELDS = [name for name, _ in _lib.MARGIN_FIELDS]


@functools.lru_cache(maxsize=None)
def _device(case_id):
    """One device run of a case through the engine: captured batches, model, reports."""
    case = next(c for c in gc.FAMILY + gc.TABLES if c["id"] == case_id)
    return gc.run(case, lambda m: m.ctx)


def _call(model, args, fresh=False, **kw):
    ctx = model._make_ctx() if fresh else model.ctx._ctx  # (model.ctx is marks_cases.Capture around the device's)
    return ctx.posttrain_rank(*args, want_x=True, **kw)


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _same_margins(a, b):
    return all(_same(a[f], b[f]) for f in FIELDS)


def _check_rows_against_host(model, args, xs, mg, tol, counts):
    """Every row (triple i, kelpie row xs[i]) of one kind against the host; counts = [rows,
    rows with an undecided column]."""
    _, _, _, _, _, _, pred, filt_off, filt = args
    for i, got in enumerate(gc.margin_rows(mg)):
        und = gc.check_against_host(model, pred[i], xs[i], filt[filt_off[i]:filt_off[i + 1]], tol, got)
        assert und <= 1, (i, und)
        counts[0] += 1
        counts[1] += int(und > 0)


# ----------------------------------------------------------------------------- every family
@pytest.mark.parametrize("case", gc.FAMILY, ids=gc.ids(gc.FAMILY))
def test_nothing_else_moves_and_reruns(case):
    batches, model, _ = _device(case["id"])
    args = batches[0]["args"]
    E = int(args[0].epochs)
    kw = {"topk": 5, "probes": gc.own_probes(args, copies=2), "trace": True, "marks": [0, 3, E]}  # 2 probes, 3 marks
    plain = _call(model, args, **kw)
    with_m = _call(model, args, margins=gc.TOL, **kw)
    assert len(with_m) == len(plain) + 1
    s, r, x, (ids, top), (ps, pr), losses, (ms, mrk, mx) = plain
    s2, r2, x2, (ids2, top2), (ps2, pr2), losses2, (ms2, mrk2, mx2) = with_m[:-1]
    for a, c in ((s, s2), (r, r2), (x, x2), (ids, ids2), (top, top2), (ps, ps2), (pr, pr2), (ms, ms2), (mrk, mrk2),
                 (mx, mx2)):
        assert _same(a, c)
    assert len(losses) == len(losses2) and all(_same(a, c) for a, c in zip(losses, losses2))
    slots, probes, marks = with_m[-1]
    assert marks["rank_lo"].shape == (len(s), 3) and probes["rank_lo"].shape == (2 * len(s),)
    # the margins without the other requests are the same, and the engine's call returned them
    bare = _call(model, args, margins=gc.TOL)
    assert all(_same(a, c) for a, c in zip(bare[:3], plain[:3]))
    assert _same_margins(bare[-1][0], slots) and bare[-1][1] is None and bare[-1][2] is None
    assert _same_margins(batches[0]["out"][-1][0], slots)
    # 4. the probe equal to its slot, the mark at hp.epochs
    for k in (0, 1):
        assert _same_margins({f: probes[f][k::2] for f in FIELDS}, slots)
    assert _same_margins({f: marks[f][:, -1] for f in FIELDS}, slots)
    # 2. a fresh context
    again = _call(model, args, fresh=True, margins=gc.TOL, **kw)
    assert all(_same_margins(a, c) for a, c in zip(again[-1], with_m[-1]))
    assert _same(again[1], r)


@pytest.mark.parametrize("case", gc.FAMILY, ids=gc.ids(gc.FAMILY))
def test_tol_zero_and_nesting(case):
    batches, model, _ = _device(case["id"])
    wide = narrow = 0
    for b in batches:
        E = int(b["args"][0].epochs)
        outs = [_call(model, b["args"], margins=t, marks=[0, E]) for t in gc.TOLS]
        r = outs[0][1]
        mrk = outs[0][3][1]
        for kind, rank in ((0, r), (2, mrk)):
            per_tol = [o[-1][kind] for o in outs]
            assert _same(per_tol[0]["rank_lo"], rank) and _same(per_tol[0]["rank_hi"], rank)
            for a, c in zip(per_tol, per_tol[1:]):
                assert (c["rank_lo"] <= a["rank_lo"]).all() and (a["rank_hi"] <= c["rank_hi"]).all()
                for f in ("ties", "gap_better", "gap_worse", "id_better", "id_worse"):
                    assert _same(a[f], c[f]), f
            for m in per_tol:
                assert (m["rank_lo"] <= rank).all() and (rank <= m["rank_hi"]).all()
                assert (m["gap_better"] >= 0).all() and (m["gap_worse"] >= 0).all()
            at = per_tol[gc.TOLS.index(gc.TOL)]
            wide += int((at["rank_hi"] > at["rank_lo"]).sum())
            narrow += int((at["rank_hi"] == at["rank_lo"]).sum())
    print(f"{case['id']}: at tol {gc.TOL} {wide} rank rows with a band, {narrow} without")


@pytest.mark.parametrize("case", gc.FAMILY, ids=gc.ids(gc.FAMILY))
def test_neighbours_in_the_topk_list(case):
    batches, model, _ = _device(case["id"])
    args = batches[0]["args"]
    _, _, _, _, _, _, pred, filt_off, filt = args
    n = len(pred)
    first = _call(model, args, topk=32)
    ids = first[3][0]
    assert (ids >= 0).all()
    # probes: per slot the columns at places 5 and 20 of its own list, under the slot's filter
    places = (5, 20)
    p_off = np.arange(n + 1, dtype=np.int32) * len(places)
    p_tr = np.array([[pred[i][1], ids[i][j]] for i in range(n) for j in places], np.int32)
    pf = [np.asarray(filt[filt_off[i]:filt_off[i + 1]], np.int32) for i in range(n) for _ in places]
    pf_off = np.concatenate([[0], np.cumsum([len(v) for v in pf])]).astype(np.int32)
    out = _call(model, args, topk=32, probes=(p_off, p_tr, pf_off, np.concatenate(pf)), margins=gc.TOL)
    assert _same(out[3][0], ids)
    rows = gc.margin_rows(out[-1][1])
    ranks = out[4][1]
    checked = 0
    for i in range(n):
        own = int(pred[i][2])
        for k, j in enumerate(places):
            m, rank = rows[i * len(places) + k], int(ranks[i * len(places) + k])
            # the slot's list holds the slot's target with the target's value and every other
            # unmasked column with the value a probe compares: the probe's object keeps its
            # place unless the slot's target (masked for a maximizer's probe if filtered) moves
            if m["ties"] or own in ids[i].tolist() or rank != j + 1:
                continue
            assert m["id_better"] == ids[i][j - 1] and m["id_worse"] == ids[i][j + 1], (i, j, m, ids[i].tolist())
            checked += 1
    # and the slots whose own target stands inside their list
    srows = gc.margin_rows(out[-1][0])
    for i in range(n):
        r = int(out[1][i])
        if srows[i]["ties"] == 0 and 2 <= r < 32 and ids[i][r - 1] == int(pred[i][2]):
            assert srows[i]["id_better"] == ids[i][r - 2] and srows[i]["id_worse"] == ids[i][r], (i, srows[i])
            checked += 1
    assert checked >= n, (checked, n)


HOST_CASES = [c for c in gc.FAMILY + gc.TABLES if c["model"] in gc.HOST]


@pytest.mark.parametrize("case", HOST_CASES, ids=gc.ids(HOST_CASES))
def test_against_the_definition(case):
    batches, model, _ = _device(case["id"])
    counts = [0, 0]
    for b in batches:
        args = b["args"]
        E = int(args[0].epochs)
        for tol in (0.0, gc.TOL, 1e-2):
            s, r, x, (ms, mrk, mx), (slots, _, marks) = _call(model, args, marks=[0, 3, E], margins=tol)
            _check_rows_against_host(model, args, x, slots, tol, counts)
            for j in range(3):
                _check_rows_against_host(model, args, mx[:, j], {f: marks[f][:, j] for f in FIELDS}, tol, counts)
    assert counts[0] > 0 and 20 * counts[1] <= counts[0], counts
    print(f"{case['id']}: {counts[0]} rank rows held against the host, {counts[1]} with an undecided column")


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n_rows", [1, 16, 17])
@pytest.mark.parametrize("case", [gc.FAMILY[0], gc.FAMILY[3]], ids=gc.ids([gc.FAMILY[0], gc.FAMILY[3]]))
def test_rank_row_counts(case, n_rows):
    """1, 16 and 17 rank rows (a workgroup row of the count holds 16): as slots, and as probe
    rows in chunks of 16 with a last chunk of one."""
    batches, model, _ = _device(case["id"])
    src = batches[0]["args"]
    idx = [i % 3 for i in range(n_rows)]
    args = gc.take_slots(src, idx)
    plain = _call(model, args, probes=gc.own_probes(args))
    out = _call(model, args, margins=gc.TOL, probes=gc.own_probes(args))
    assert all(_same(a, c) for a, c in zip(plain[:3], out[:3])) and _same(plain[3][1], out[3][1])
    slots, probes, _ = out[-1]
    assert len(slots["rank_lo"]) == n_rows and (slots["rank_lo"] <= out[1]).all() and (out[1] <= slots["rank_hi"]).all()
    assert _same_margins(probes, slots)
    zero = _call(model, args, margins=0.0)
    assert _same(zero[-1][0]["rank_lo"], zero[1]) and _same(zero[-1][0]["rank_hi"], zero[1])
    counts = [0, 0]
    _check_rows_against_host(model, args, out[2], slots, gc.TOL, counts)
    assert counts == [n_rows, 0]


def test_probe_chunks(monkeypatch):
    """17 probe rows in chunks of 16: the margins of the unchunked call."""
    case = gc.FAMILY[0]
    batches, model, _ = _device(case["id"])
    args = gc.take_slots(batches[0]["args"], [i % 3 for i in range(17)])
    kw = {"probes": gc.own_probes(args), "marks": [0, 8], "margins": gc.TOL}
    whole = _call(model, args, **kw)
    monkeypatch.setenv("KP_PROBE_CHUNK", "16")
    monkeypatch.setenv("KP_MARKS_CHUNK", "16")
    chunked = _call(model, args, **kw)
    assert all(_same_margins(a, c) for a, c in zip(chunked[-1], whole[-1]))
    assert _same(chunked[1], whole[1])


@pytest.mark.parametrize("case", [gc.FAMILY[0], gc.FAMILY[1], gc.FAMILY[3]],
                         ids=gc.ids([gc.FAMILY[0], gc.FAMILY[1], gc.FAMILY[3]]))
def test_filtered_target(case):
    """The target in its own filter list and out of it: a maximizer's rank leaves a filtered
    target out (own = 0), a minimizer's restores it (own = 1); every other column is held the
    same either way."""
    batches, model, _ = _device(case["id"])
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = batches[0]["args"]
    outs = {}
    for inside in (False, True):
        fl = []
        for i in range(len(pred)):
            f = np.asarray(filt[filt_off[i]:filt_off[i + 1]])
            f = f[f != pred[i][2]]
            fl.append(np.append(f, pred[i][2]) if inside else f)
        fo = np.concatenate([[0], np.cumsum([len(v) for v in fl])]).astype(np.int32)
        args = (hp, x0, row_off, rows, rng_off, rng, pred, fo, np.concatenate(fl))
        out = outs[inside] = _call(model, args, margins=0.0)
        assert _same(out[-1][0]["rank_lo"], out[1]) and _same(out[-1][0]["rank_hi"], out[1])
        counts = [0, 0]
        _check_rows_against_host(model, args, out[2], out[-1][0], 0.0, counts)
        wide = _call(model, args, margins=1e-2)
        _check_rows_against_host(model, args, wide[2], wide[-1][0], 1e-2, counts)
    drop = 0 if model.is_minimizer() else 1
    assert (outs[True][1] == outs[False][1] - drop).all()
    for f in ("ties", "gap_better", "gap_worse", "id_better", "id_worse"):
        assert _same(outs[True][-1][0][f], outs[False][-1][0][f])


@pytest.mark.parametrize("case", gc.FAMILY[:2], ids=gc.ids(gc.FAMILY[:2]))
def test_kelpie_column_is_the_nearest(case):
    """hp.epochs = 0 leaves x0 as the row: with x0 a hair off the target's own row the kelpie
    column scores a hair off the target, nearer than any entity."""
    batches, model, _ = _device(case["id"])
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = batches[0]["args"]
    hp0 = type(hp).from_buffer_copy(hp)
    hp0.epochs = 0
    E = model.entity_embeddings
    x0 = np.stack([E[int(p[2])] * np.float32(1.0 + (1e-5 if i % 2 else -1e-5)) for i, p in enumerate(pred)])
    args = (hp0, x0.astype(np.float32), row_off, rows, rng_off, rng, pred, filt_off, filt)
    out = _call(model, args, margins=gc.TOL)
    assert _same(out[2], x0)
    n_ent = model.dataset.num_entities
    rows_m = gc.margin_rows(out[-1][0])
    assert all(n_ent in (m["id_better"], m["id_worse"]) for m in rows_m), rows_m
    counts = [0, 0]
    _check_rows_against_host(model, args, out[2], out[-1][0], gc.TOL, counts)
    # masked, the kelpie column takes no part
    fl = [np.append(np.asarray(filt[filt_off[i]:filt_off[i + 1]]), n_ent) for i in range(len(pred))]
    fo = np.concatenate([[0], np.cumsum([len(v) for v in fl])]).astype(np.int32)
    masked = _call(model, args[:7] + (fo, np.concatenate(fl)), margins=gc.TOL)
    assert all(n_ent not in (m["id_better"], m["id_worse"]) for m in gc.margin_rows(masked[-1][0]))


def test_conve_saturated_targets():
    """Targets whose float32 sigmoid is 1.0 (test_gpu_parity.test_conve_saturated_sigmoid_ties'
    model: BN3 scaled x30 at d = 60): every saturated column counts at both thresholds, so the
    band holds the rank's hundreds of ties at every tol and is the rank at tol = 0."""
    import width_cases as wc
    from kelpie_amd import synth
    CV_HP = wc.CV_HP
    dim = 60
    g = synth.make_graph("small", seed=9)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    w = synth.make_weights("ConvE", g.num_entities, g.num_relations, dim, seed=9, conve_random_bn=True,
                           trained_scale=0.5)
    w["bn3_weight"] = w["bn3_weight"] * 30
    w["bn3_bias"] = w["bn3_bias"] * 30
    bn = {i: {"weight": w[f"bn{i}_weight"], "bias": w[f"bn{i}_bias"], "running_mean": w[f"bn{i}_mean"],
              "running_var": w[f"bn{i}_var"]} for i in (1, 2, 3)}
    model = ka.ConvE(ds, w["entity_embeddings"], w["relation_embeddings"], w["conv_weight"].reshape(32, 3, 3),
                     w["conv_bias"], w["fc_weight"], w["fc_bias"], bn=bn)
    test = [tuple(int(v) for v in t) for t in g.test][:50]
    sc = model.ctx.all_scores(np.array([t[0] for t in test]), np.array([t[1] for t in test]))
    preds = [t for i, t in enumerate(test) if sc[i][t[2]] == 1.0][:3]
    assert len(preds) == 3, "no saturated targets"
    saturated = 0
    for pred in preds:
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:2]
        reports = {}
        for tol in (0.0, 1e-2):
            seed_all(42)
            eng = ka.NecessaryPostTrainingEngine(model, ds, dict(CV_HP, epochs=5))
            reports[tol] = eng.compute_margins(pred, [[c] for c in cands], tol=tol)
        for a, c in zip(reports[0.0], reports[1e-2]):
            assert a["relevance"] == c["relevance"]
            for side in ("base", "post"):
                assert a[side]["rank_lo"] == a[side]["rank"] == a[side]["rank_hi"]
                assert c[side]["rank_lo"] <= c[side]["rank"] <= c[side]["rank_hi"]
                if a[side]["score"] == 1.0:
                    saturated += 1
                    # the saturated columns are in the band's low end as well: far more than
                    # the handful of columns with a larger logit
                    assert c[side]["rank_lo"] > 50, c[side]
    assert saturated > 0, "no saturated post-trained target"


# ----------------------------------------------------------------------------- the engines on the device
@pytest.mark.parametrize("draws", ["reference", "keyed"])
@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
def test_engine_reports(mode, draws):
    """compute_margins on the device, ComplEx: the relevances are compute_relevance_batch's bit
    for bit (the same seeds, or the same keys), every band holds its rank and the relevance band
    holds the relevance up to the float32 rounding of the latter."""
    import width_cases as wc
    case = gc.FAMILY[0]
    ds, ordinary = wc.graph(case["n_ent"])[1:3]
    pred = ordinary[0]
    rules = [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]
    cls = ka.NecessaryPostTrainingEngine if mode == "necessary" else ka.SufficientPostTrainingEngine
    outs = []
    for margins in (False, True):
        model = wc.make_model(case)
        seed_all(42)
        eng = cls(model, ds, wc.hp_of(case))
        if draws == "keyed":
            eng.draws, eng.seed = "keyed", 7
        if mode == "sufficient":
            eng.entities_to_convert = [int(p[0]) for p in ordinary if p[0] != pred[0]][:2]
        outs.append(eng.compute_margins(pred, rules) if margins else eng.compute_relevance_batch(pred, rules))
    plain, rep = outs
    assert [o["relevance"] for o in rep] == plain
    for o in rep:
        slack = 2.0 ** -23 * max(1.0, abs(o["relevance"]))
        assert o["relevance_lo"] - slack <= o["relevance"] <= o["relevance_hi"] + slack
        sides = [o["base"], o["post"]] if mode == "necessary" else [c[k] for c in o["conversions"] for k in ("base", "post")]
        assert all(s["rank_lo"] <= s["rank"] <= s["rank_hi"] and s["ties"] >= 0 for s in sides)
