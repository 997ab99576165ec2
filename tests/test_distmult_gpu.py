"""DistMult on the device against the zero-imaginary stand-in (distmult_backend.py), the
reference fixture and the device ComplEx path on zero-imaginary tables.

Scores: |gpu - ref| <= 1e-4 * max(1, |ref|).  Final rows: within 1e-4 of the row's largest
magnitude.  Ranks: with delta = 1e-4 * max(1, |t|) and the reference's own scores s_e and
target t, the device rank lies in [#{e: s_e >= t + delta}, #{e: s_e >= t - delta}] (the
targets sit mid-table with neighbours 1e-6 to 1e-5 relative away, so an exact rank is not
what the score tolerance implies); no slot is left out, and each test prints how many ranks
matched exactly.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import functools

import numpy as np
import pytest

import kelpie_amd as ka
from distmult_backend import (TOL, DistMultOracleContext, RecordingContext, check_fixture_model, check_fixture_slots,
                              check_slots, complex_embedding, load_fixture, rank_bounds, zero_imaginary)
from golden_io import seed_all
from kelpie_amd import synth

pytestmark = pytest.mark.gpu

# test_gpu_parity.HP
HP = {"optimizer_name": "Adagrad", "batch_size": 512, "epochs": 20, "lr": 0.043, "decay1": 0.9, "decay2": 0.999,
      "regularizer_name": "N3", "regularizer_weight": 0}
HUB_EPOCHS = 3  # 2,053 triples: nine minibatches per epoch, a plan per (epoch, step)


@functools.lru_cache(maxsize=None)
def _small(dim, seed=3, scale=0.3):
    g = synth.make_graph("small", seed=seed)  # 2,000 entities: 63 key tiles, the last one partial
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    w = synth.make_weights("DistMult", g.num_entities, g.num_relations, dim, seed=seed, trained_scale=scale)
    deg = ds.entity_to_degree
    test = [tuple(int(v) for v in t) for t in g.test]
    ordinary = [t for t in test if 8 <= deg.get(t[0], 0) <= 40]
    hub = max(test, key=lambda t: deg.get(t[0], 0))
    assert deg[hub[0]] > 256
    return g, ds, w, ordinary, hub


def _model(dim, hot=False, init_scale=1e-3):
    g, ds, w, ordinary, hub = _small(dim)
    E = w["entity_embeddings"]
    if hot:
        # scores far above every split's first-tile maximum: the attention's exact-max second pass
        E = E.copy()
        E[-1] = 40.0
        init_scale = 1.0
    return ds, ka.DistMult(ds, E, w["relation_embeddings"], init_scale=init_scale), ordinary, hub


def _necessary(ctx_of, dim, hp, hot, hub, n_cands):
    """One ordinary subject (8 to 40 triples) with ``n_cands`` singleton candidates, then
    (``hub``) the hub subject with one candidate and HUB_EPOCHS epochs; the post-trained
    slots in call order and the relevances."""
    ds, model, ordinary, hub_pred = _model(dim, hot)
    model._ctx = ctx_of(model)
    seed_all(42)
    rels = []
    for pred, epochs, n in [(ordinary[0], hp["epochs"], n_cands)] + ([(hub_pred, HUB_EPOCHS, 1)] if hub else []):
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(hp, epochs=epochs))
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        rels.append(eng.compute_relevance_batch(pred, [[c] for c in cands]))
    return model.ctx.slots, rels


_REF = {}


def _reference(key, run):
    """The stand-in's side of a case, computed once and shared by the cases that differ only
    in how the device partitions its attention."""
    if key not in _REF:
        _REF[key] = run(DistMultOracleContext)
    return _REF[key]


def _hp(opt="Adagrad", reg=None, lr=0.043):
    return dict(HP, optimizer_name=opt, lr=lr, regularizer_name=reg or "N3", regularizer_weight=0.05 if reg else 0)


def _device(model):
    return RecordingContext(model.ctx)


# --------------------------------------------------------------------------- 1. all_scores
def test_all_scores_matches_fp64_product():
    ds, model, ordinary, hub = _model(200)
    t = np.array(ordinary[:16] + [hub], np.int64)
    got = model.all_scores(t)
    E, R = model.entity_embeddings.astype(np.float64), model.relation_embeddings.astype(np.float64)
    ref = (E[t[:, 0]] * R[t[:, 1]]) @ E.T
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= TOL * max(1.0, np.abs(ref).max())


# --------------------------------------------------------------------------- 2. necessary mode
NECESSARY = [  # dim, attention partition, optimizer, regulariser, lr, hot, hub, candidates
    pytest.param(200, "streamk", "Adagrad", None, 0.043, False, True, 2, id="d200-streamk"),
    pytest.param(200, "ranges", "Adagrad", None, 0.043, False, True, 2, id="d200-ranges"),
    pytest.param(24, "auto", "Adagrad", None, 0.043, False, False, 3, id="d24-DB2-padded"),
    pytest.param(8, "auto", "Adagrad", None, 0.043, False, False, 3, id="d8-DB1"),
    pytest.param(400, "auto", "Adagrad", None, 0.043, False, False, 1, id="d400-DB25"),
    pytest.param(200, "auto", "Adagrad", "N3", 0.043, False, True, 2, id="d200-N3"),
    pytest.param(200, "auto", "Adagrad", "N2", 0.043, False, True, 2, id="d200-N2"),
    pytest.param(8, "auto", "Adam", None, 0.01, False, False, 3, id="d8-Adam"),
    pytest.param(8, "auto", "SGD", None, 0.05, False, False, 3, id="d8-SGD"),
    pytest.param(200, "streamk", "Adagrad", None, 0.043, True, True, 2, id="d200-hot"),
]


@pytest.mark.parametrize("dim,part,opt,reg,lr,hot,hub,n_cands", NECESSARY)
def test_necessary_vs_standin(dim, part, opt, reg, lr, hot, hub, n_cands, monkeypatch):
    """d = 200 is DB 13 (208 columns, 8 of them padding) with the attention partition forced
    to stream-K and to key ranges; d = 24 DB 2 (padded), d = 8 DB 1, d = 400 DB 25.  ``hot``:
    the last entity row set to 40.0 and init_scale 1.0, as in
    test_gpu_parity.test_complex_vs_oracle_full_width."""
    monkeypatch.setenv("KP_ATTN_PART", part)
    hp = _hp(opt, reg, lr)

    def run(ctx_of):
        return _necessary(ctx_of, dim, hp, hot, hub, n_cands)

    ref_slots, _ = _reference((dim, opt, reg, lr, hot, hub, n_cands), run)
    slots, _ = run(_device)
    exact = check_slots(slots, ref_slots)
    print(f"exact ranks {exact}/{len(slots)}; ranks {[s['rank'] for s in slots]}")


# --------------------------------------------------------------------------- 3. crafted batch
def _crafted(model, K, nr):
    """Four slots through posttrain_rank directly: a self-loop (K, r, K) and its inverse (the
    kelpie-target count ck); no rows at all (rank only); rows repeating one relation and one
    frozen (h, r) pair (counts above 1); a ranked object that is the kelpie entity."""
    d = model.dimension
    rng = np.random.default_rng(5)
    x0 = (rng.random((4, d)) * 0.2).astype(np.float32)
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
    return (x0, np.array(row_off), np.vstack(rows), np.zeros(5, np.int64), np.zeros(0, np.int32), np.array(pred),
            filt_off, filt)


@pytest.mark.parametrize("dim", [24, 200])
def test_crafted_batch_vs_standin_and_device_complex(dim):
    ds, model, _, _ = _model(dim)
    K, nr = ds.num_entities, ds.num_relations
    hp = model.kp_hp(dict(HP, epochs=8))
    args = _crafted(model, K, nr)
    ref = DistMultOracleContext(model)
    ref.posttrain_rank(hp, *args, want_x=True)
    dev = RecordingContext(model.ctx)
    dev.posttrain_rank(hp, *args, want_x=True)
    exact = check_slots(dev.slots, ref.slots)
    assert np.array_equal(dev.slots[1]["x"], args[0][1]), "a slot without rows must only be ranked"
    # the same batch through the device ComplEx path on [E | 0], [R | 0]: an independent
    # second reference on the GPU, whose imaginary half must stay exactly 0
    cx = complex_embedding(model)
    s, r, x = cx.ctx.posttrain_rank(hp, zero_imaginary(args[0]), *args[1:], want_x=True)
    assert not x[:, dim:].any()
    cx_slots = [{"score": float(s[i]), "rank": int(r[i]), "x": x[i, :dim]} for i in range(len(s))]
    exact_cx = check_slots(cx_slots, ref.slots)
    print(f"exact ranks: DistMult {exact}/4, device ComplEx {exact_cx}/4; ranks {[a['rank'] for a in dev.slots]}")
    for a, b in zip(dev.slots, cx_slots):
        assert abs(a["score"] - b["score"]) <= TOL * max(1.0, abs(b["score"]))
        assert np.abs(a["x"] - b["x"]).max() <= TOL * np.abs(b["x"]).max()


# --------------------------------------------------------------------------- 4. sufficient mode
def test_sufficient_vs_standin():
    """d = 200: the conversion entities are chosen alike, and the base and the post-trained
    slot of every conversion entity is held against the stand-in's."""
    def run(ctx_of):
        ds, model, ordinary, _ = _model(200)
        model._ctx = ctx_of(model)
        seed_all(42)
        eng = ka.SufficientPostTrainingEngine(model, ds, HP)
        pred = ordinary[0]
        ents = eng.select_entities_to_convert(pred, 3, 40)
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:2]
        rels = eng.compute_relevance_batch(pred, [[c] for c in cands])
        return model.ctx.slots, (ents, rels)

    ref_slots, (ref_ents, _) = _reference("sufficient", run)
    slots, (ents, _) = run(_device)
    assert ents == ref_ents and len(ents) == 3
    assert len(slots) == 3 + 2 * 3  # a base slot per conversion entity, a post-trained one per (rule, entity)
    exact = check_slots(slots, ref_slots)
    print(f"exact ranks {exact}/{len(slots)}; ranks {[s['rank'] for s in slots]}")


# --------------------------------------------------------------------------- 5. batch = sequential
def test_batch_equals_sequential_and_is_deterministic():
    ds, model, ordinary, _ = _model(200)
    pred = ordinary[1]
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:6]
    runs = []
    for mode in ("batch", "batch", "seq"):
        seed_all(42)
        eng = ka.NecessaryPostTrainingEngine(model, ds, HP)
        if mode == "batch":
            runs.append(eng.compute_relevance_batch(pred, [[c] for c in cands]))
        else:
            runs.append([eng.compute_relevance(pred, [c]) for c in cands])
    assert runs[0] == runs[1]
    assert np.allclose(runs[0], runs[2], atol=1e-6)


# --------------------------------------------------------------------------- 6. predict_tails
def test_predict_tails_and_evaluator_vs_standin():
    g, ds, w, _, _ = _small(200)
    test = np.asarray(g.test[:50], np.int64)
    _, model, _, _ = _model(200)
    _, ref_model, _, _ = _model(200)
    ref_model._ctx = DistMultOracleContext(ref_model)
    scores, ranks = model.predict_tails(test)
    ref_scores, ref_ranks = ref_model.predict_tails(test)
    all_ref = ref_model.all_scores(test)
    exact = 0
    for i, (h, r, o) in enumerate(test.tolist()):
        assert abs(scores[i] - ref_scores[i]) <= TOL * max(1.0, abs(ref_scores[i]))
        lo, hi = rank_bounds(all_ref[i], all_ref[i][o], [e for e in ds.to_filter.get((h, r), []) if e != o])
        assert lo <= ranks[i] <= hi, (i, ranks[i], ref_ranks[i], lo, hi)
        exact += int(ranks[i] == ref_ranks[i])
    print(f"predict_tails: exact ranks {exact}/50")
    from kelpie_amd.evaluation import Evaluator
    m, mref = Evaluator(model).evaluate(test[:20]), Evaluator(ref_model).evaluate(test[:20])
    assert set(m) == set(mref)


# --------------------------------------------------------------------------- reference fixture
def test_device_reproduces_the_reference_fixture():
    rec, ds, model = load_fixture()
    check_fixture_model(rec, model)
    check_fixture_slots(rec, model, model.ctx)


# --------------------------------------------------------------------------- 7. error paths
def test_error_paths():
    g, ds, w, _, _ = _small(8)
    n_ent, nr2 = ds.num_entities, 2 * ds.num_relations
    with pytest.raises(ka._lib.KelpieHipError, match=r"\(-95\).*DistMult: row width > 400 not supported"):
        ka._lib.Context("DistMult", np.zeros((n_ent, 401), np.float32), np.zeros((nr2, 401), np.float32))
    with pytest.raises(ka._lib.KelpieHipError, match=r"\(-22\).*norm_p"):
        ka._lib.Context("DistMult", w["entity_embeddings"], w["relation_embeddings"], norm_p=1)
    ctx = ka._lib.Context("DistMult", w["entity_embeddings"], w["relation_embeddings"])
    hp = ka.DistMult(ds, w["entity_embeddings"], w["relation_embeddings"]).kp_hp(HP)
    with pytest.raises(ka._lib.KelpieHipError, match="ComplEx contexts only"):
        ctx.train_epoch(hp, g.train[:64], np.arange(64), 0)
    with pytest.raises(ka._lib.KelpieHipError):
        ctx.dp_relevance(np.zeros((1, 7), np.int32), 0.1, 1.0, 1, 1)
