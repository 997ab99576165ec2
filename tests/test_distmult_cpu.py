"""DistMult on the CPU tier: registry and hyper-parameters, an independent restatement of
the Kelpie step, the host layer over the zero-imaginary stand-in (distmult_backend.py),
the reference fixture and the world-2 sharding."""
import os
import socket

import numpy as np
import pydantic
import pytest
import torch

import kelpie_amd as ka
from distmult_backend import (TOL, DistMultOracleContext, check_fixture_model, check_fixture_slots, load_fixture,
                              rank_bounds)
from golden_io import seed_all
from kelpie_amd import hparams, synth

HP = {"optimizer_name": "Adagrad", "batch_size": 512, "epochs": 20, "lr": 0.043, "decay1": 0.9, "decay2": 0.999,
      "regularizer_name": "N3", "regularizer_weight": 0}


def _model(shape="tiny", dim=8, seed=7, scale=0.3, init_scale=1e-3, standin=True, **graph):
    g = synth.make_graph(shape, seed=seed, **graph)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    w = synth.make_weights("DistMult", g.num_entities, g.num_relations, dim, seed=seed, trained_scale=scale)
    model = ka.DistMult(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=init_scale)
    if standin:
        model._ctx = DistMultOracleContext(model)
    return g, ds, model


# ----------------------------------------------------------------------------- registry
def test_registry_and_hyperparameters():
    assert ka.MODEL_REGISTRY["DistMult"] is ka.DistMult
    assert ka._lib.KP_MODEL["DistMult"] == 3
    assert hparams.OPTIMIZER_HP["DistMult"] is hparams.MultiClassNLLOptimizerHyperParams
    assert hparams.MODEL_HP["DistMult"] is hparams.DistMultHyperParams
    assert hparams.model_params("DistMult", {"dimension": "8", "init_scale": 1}) == {"dimension": 8, "init_scale": 1.0}
    with pytest.raises(pydantic.ValidationError):
        hparams.model_params("DistMult", {"dimension": 8})  # init_scale missing
    with pytest.raises(pydantic.ValidationError):
        hparams.model_params("DistMult", {"dimension": "eight", "init_scale": 0.1})
    _, ds, model = _model()
    with pytest.raises(pydantic.ValidationError):
        ka.NecessaryPostTrainingEngine(model, ds, {k: v for k, v in HP.items() if k != "lr"})
    with pytest.raises(pydantic.ValidationError):
        ka.NecessaryPostTrainingEngine(model, ds, dict(HP, epochs="many"))


def test_model_surface_and_kelpie_init():
    _, ds, model = _model(dim=8, init_scale=0.25, standin=False)
    assert model.name == "DistMult" and model.dimension == 8 and not model.is_minimizer()
    assert not model.skip_needs_rows
    init = np.linspace(0.0, 1.0, 8, dtype=np.float32)
    row = model.kelpie_init(init, None)
    assert row.dtype == np.float32 and np.array_equal(row, init * np.float32(0.25))
    hp = model.kp_hp(dict(HP, regularizer_name="N2", regularizer_weight=0.05, optimizer_name="Adam"))
    assert (hp.optimizer, hp.reg_kind, hp.epochs, hp.batch_size) == (1, 1, 20, 512)
    with pytest.raises(ValueError):
        model.kp_hp(dict(HP, optimizer_name="RMSprop"))


def test_from_state_dict_and_adapter():
    g, ds, model = _model(dim=8, standin=False)
    state = {"entity_embeddings": torch.from_numpy(model.entity_embeddings),
             "relation_embeddings": torch.from_numpy(model.relation_embeddings)}
    m2 = ka.from_state_dict("DistMult", ds, state, {"dimension": 8, "init_scale": 0.5})
    assert isinstance(m2, ka.DistMult) and m2.init_scale == 0.5
    assert np.array_equal(m2.entity_embeddings, model.entity_embeddings)
    with pytest.raises(pydantic.ValidationError):
        ka.from_state_dict("DistMult", ds, state, {"dimension": 8})

    class Ref:  # what the adapter reads of a reference DistMult object (duck typing)
        name = "DistMult"
        init_scale = 0.125
        entity_embeddings = state["entity_embeddings"]
        relation_embeddings = state["relation_embeddings"]

    from kelpie_amd.adapters import model_from_reference
    m3 = model_from_reference(Ref(), ds)
    assert isinstance(m3, ka.DistMult) and m3.init_scale == 0.125 and m3.dimension == 8


def test_synth_weights():
    a = synth.make_weights("DistMult", 50, 4, 8, seed=1, init_scale=0.1)
    assert a["entity_embeddings"].shape == (50, 8) and a["relation_embeddings"].shape == (8, 8)
    assert a["entity_embeddings"].dtype == np.float32
    assert 0.0 <= a["entity_embeddings"].min() and a["entity_embeddings"].max() < 0.1
    b = synth.make_weights("DistMult", 50, 4, 8, seed=1, trained_scale=0.3)
    assert b["entity_embeddings"].min() < 0 and abs(float(b["entity_embeddings"].std()) - 0.3) < 0.05


def test_reference_construction_draws():
    from kelpie_amd.pipeline import reference_construction_draws
    torch.manual_seed(5)
    reference_construction_draws("DistMult", 30, 4, {"dimension": 8, "init_scale": 0.1})
    got = torch.get_rng_state()
    torch.manual_seed(5)
    torch.rand(30, 8)
    torch.rand(8, 8)
    assert torch.equal(got, torch.get_rng_state())


# ----------------------------------------------------------------------------- restatement
def _restated_step(E, R, x0, rows, perms, hp, pred):
    """The DistMult Kelpie post-training from the model's definition, with torch autograd
    (nothing shared with the oracle): E_all = cat(E, x), scores (lhs * rel) @ E_all^T, mean
    cross-entropy plus N3 / N2 over the factors (|lhs|, |rel|, |rhs|) divided by the batch
    size, torch.optim on the one row; minibatches of min(batch_size, n) rows every
    batch_size rows of each epoch's permutation."""
    E = torch.from_numpy(E)
    R = torch.from_numpy(R)
    x = torch.nn.Parameter(torch.from_numpy(x0.copy())[None])
    rows = torch.from_numpy(np.asarray(rows, np.int64))
    name = hp["optimizer_name"]
    if name == "Adagrad":
        opt = torch.optim.Adagrad([x], lr=hp["lr"])
    elif name == "Adam":
        opt = torch.optim.Adam([x], lr=hp["lr"], betas=(hp["decay1"], hp["decay2"]))
    else:
        opt = torch.optim.SGD([x], lr=hp["lr"])
    n = rows.shape[0]
    bs = min(hp["batch_size"], n)
    w = hp["regularizer_weight"]
    for perm in perms:
        prow = rows[torch.as_tensor(perm, dtype=torch.int64)]
        for start in range(0, n, hp["batch_size"]):
            batch = prow[start:start + bs]
            E_all = torch.cat([E, x], 0)
            lhs, rel, rhs = E_all[batch[:, 0]], R[batch[:, 1]], E_all[batch[:, 2]]
            loss = torch.nn.functional.cross_entropy((lhs * rel) @ E_all.T, batch[:, 2], reduction="mean")
            for f in (lhs.abs(), rel.abs(), rhs.abs()):
                if hp["regularizer_name"] == "N2":
                    loss = loss + w * torch.sum(torch.norm(f, 2, 1) ** 3) / batch.shape[0]
                else:
                    loss = loss + w * torch.sum(f ** 3) / batch.shape[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
    with torch.no_grad():
        E_all = torch.cat([E, x], 0).double()
        scores = ((E_all[pred[0]] * R[pred[1]].double()) @ E_all.T).numpy()
    return x.detach().numpy()[0], scores


@pytest.mark.parametrize("opt,reg,lr", [("Adagrad", None, 0.043), ("Adagrad", "N3", 0.043), ("Adagrad", "N2", 0.043),
                                        ("Adam", "N3", 0.01), ("SGD", "N2", 0.05)])
def test_restated_step_equals_the_zero_imaginary_standin(opt, reg, lr):
    """One slot with three minibatches per epoch on a 60-entity graph at d = 8, the same
    permutations on both sides: validates the zero-imaginary embedding without relying on
    the oracle's ComplEx code being right for it."""
    g, ds, model = _model(dim=8, seed=2, n_ent=60, n_rel=5, n_train=500, n_valid=20, n_test=20)
    K = ds.num_entities
    deg = ds.entity_to_degree
    s = next(e for e in sorted(deg) if 10 <= deg[e] <= 14)
    trip = np.array(sorted(ds.entity_to_training_triples[s]), np.int64)
    trip[trip == s] = K
    trip = np.vstack([trip, [[K, 1, K]]])  # a self-loop: the kelpie entity as head and as target
    rows = np.vstack([trip, ds.invert_triples(trip)])
    n, epochs = len(rows), 6
    hp = dict(HP, optimizer_name=opt, lr=lr, epochs=epochs, batch_size=(n + 2) // 3,
              regularizer_name=reg or "N3", regularizer_weight=0.05 if reg else 0.0)
    gen = torch.Generator().manual_seed(3)
    perms = [torch.randperm(n, generator=gen).numpy() for _ in range(epochs)]
    x0 = (np.random.default_rng(4).random(8) * 0.6).astype(np.float32)
    pred = next((K, int(r), int(o)) for h, r, o in trip.tolist() if h == K and o != K)
    filt = np.array([e for e in range(K) if e % 7 == 0 and e != pred[2]], np.int64)
    x_ref, scores = _restated_step(model.entity_embeddings, model.relation_embeddings, x0, rows, perms, hp, pred)
    sc, rk, x = model.ctx.posttrain_rank(model.kp_hp(hp), x0[None], np.array([0, n]), rows, np.array([0, epochs * n]),
                                         np.concatenate(perms).astype(np.int32), np.array([pred]),
                                         np.array([0, len(filt)]), filt, want_x=True)
    t = float(scores[pred[2]])
    print(f"{opt}/{reg}: row err {np.abs(x[0] - x_ref).max():.2e} of {np.abs(x_ref).max():.3f}, "
          f"score {float(sc[0]):.7f} vs {t:.7f}, rank {int(rk[0])}")
    assert np.abs(x[0] - x_ref).max() <= TOL * np.abs(x_ref).max()
    assert np.abs(x_ref - x0).max() > 100 * TOL * np.abs(x_ref).max(), "the row did not move"
    assert abs(float(sc[0]) - t) <= TOL * max(1.0, abs(t))
    lo, hi = rank_bounds(scores, t, filt)
    assert lo <= int(rk[0]) <= hi, (int(rk[0]), lo, hi)


# ----------------------------------------------------------------------------- host layer
def _preds(g, ds, lo=6, hi=20, n=2):
    deg = ds.entity_to_degree
    return [tuple(int(v) for v in t) for t in g.test if lo <= deg.get(int(t[0]), 0) <= hi][:n]


def test_necessary_engine_batch_equals_sequential_and_rng_consumption():
    d = 8
    hp = dict(HP, epochs=4, batch_size=16)  # the subjects' 2 x degree rows: several minibatches per epoch
    g, ds, model = _model(dim=d)
    pred = _preds(g, ds, lo=10)[0]
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:3]
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    seq = [eng.compute_relevance(pred, [c]) for c in cands]
    from kelpie_amd import rng as krng
    krng.sync()
    state = torch.get_rng_state()
    seed_all(42)
    eng2 = ka.NecessaryPostTrainingEngine(model, ds, hp)
    assert eng2.compute_relevance_batch(pred, [[c] for c in cands]) == seq
    krng.sync()
    assert torch.equal(state, torch.get_rng_state())
    # by hand: per call torch.rand(1, d); the base post-training once (cached afterwards) and
    # the call's own, a randperm of the rows (triples + inverses) per epoch each
    seed_all(42)
    n_base = 2 * len(ds.entity_to_training_triples[pred[0]])
    assert n_base > hp["batch_size"]
    for i, _ in enumerate(cands):
        torch.rand(1, d)
        for R in ([n_base] if i == 0 else []) + [n_base - 2]:
            for _e in range(hp["epochs"]):
                torch.randperm(R)
    assert torch.equal(state, torch.get_rng_state())


def test_sufficient_engine_builder_and_explain(tmp_path):
    hp = dict(HP, epochs=3)
    g, ds, model = _model(dim=8)
    pred = _preds(g, ds)[0]
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:2]
    seed_all(42)
    eng = ka.SufficientPostTrainingEngine(model, ds, hp)
    ents = eng.select_entities_to_convert(pred, 3, 200)
    assert len(ents) == 3 and pred[0] not in ents
    batch = eng.compute_relevance_batch(pred, [[c] for c in cands])
    seed_all(42)
    eng = ka.SufficientPostTrainingEngine(model, ds, hp)
    assert eng.select_entities_to_convert(pred, 3, 200) == ents
    assert [eng.compute_relevance(pred, [c]) for c in cands] == batch
    # the builder over the necessary engine
    seed_all(42)
    neng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    neng.set_cache()
    out = ka.StochasticBuilder(0.9, neng, window=4).build_explanations(pred, cands)
    assert out["#relevances"] >= len(cands) and out["rule_to_relevance"]
    # run_explain with a DistMult state dict
    from kelpie_amd import models
    from kelpie_amd.pipeline import run_explain
    made = []
    orig = models.from_state_dict

    def standin_model(*a, **k):
        m = orig(*a, **k)
        m._ctx = DistMultOracleContext(m)
        made.append(m)
        return m

    models.from_state_dict = standin_model
    try:
        state = {"entity_embeddings": torch.from_numpy(model.entity_embeddings),
                 "relation_embeddings": torch.from_numpy(model.relation_embeddings)}
        res = run_explain("DistMult", ds, state, {"dimension": 8, "init_scale": 1e-3}, hp, "necessary",
                          [list(ds.labels_triple(pred))], prefilter_k=3, xsi=0.9,
                          output_path=str(tmp_path / "output.json"))
    finally:
        models.from_state_dict = orig
    assert len(res) == 1 and res[0]["rule_to_relevance"] and isinstance(made[0], ka.DistMult)
    assert made[0].ctx.calls, "run_explain post-trained nothing"


def test_predict_tails_over_the_standin():
    g, ds, model = _model(dim=8)
    test = np.asarray(g.test[:10], np.int64)
    scores, ranks = model.predict_tails(test)
    E, R = model.entity_embeddings.astype(np.float64), model.relation_embeddings.astype(np.float64)
    for (h, r, o), s, k in zip(test.tolist(), scores, ranks):
        row = (E[h] * R[r]) @ E.T
        assert abs(s - row[o]) <= TOL * max(1.0, abs(row[o]))
        lo, hi = rank_bounds(row, row[o], [e for e in ds.to_filter.get((h, r), []) if e != o])
        assert lo <= k <= hi


# ----------------------------------------------------------------------------- reference fixture
def test_standin_reproduces_the_reference_fixture():
    rec, ds, model = load_fixture()
    model._ctx = DistMultOracleContext(model)
    check_fixture_model(rec, model)
    check_fixture_slots(rec, model, model.ctx)


# ----------------------------------------------------------------------------- world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sharded_run(sharding):
    hp = dict(HP, epochs=3)
    g, ds, model = _model(dim=8)
    out = {}
    preds = _preds(g, ds)
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp)
    eng.sharding = sharding
    out["necessary"] = []
    for pred in preds:
        eng.set_cache()
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:4]
        out["necessary"].append(eng.compute_relevance_batch(pred, [[c] for c in cands]))
    seed_all(42)
    seng = ka.SufficientPostTrainingEngine(model, ds, hp)
    seng.sharding = sharding
    out["entities"] = seng.select_entities_to_convert(preds[0], 3, 200)
    cands = sorted(ds.entity_to_training_triples[preds[0][0]])[:2]
    out["sufficient"] = seng.compute_relevance_batch(preds[0], [[c] for c in cands])
    return out


def _sharded_worker(rank, world, port, q):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from kelpie_amd import distributed as kd
    kd.init_from_env(backend="gloo")
    try:
        q.put((rank, _sharded_run(kd.SlotSharding(device="cpu"))))
    except BaseException as e:  # report instead of hanging the other rank's gather
        q.put((rank, repr(e)))
        raise
    finally:
        import torch.distributed as dist
        dist.destroy_process_group()


def test_sharding_world2_equals_world1():
    """Every rank schedules every batch and post-trains its share of the slots (DistMult
    skips another rank's draws as ComplEx does); the gathered relevances and the conversion
    entities equal the single-process run bit for bit."""
    import torch.multiprocessing as mp
    single = _sharded_run(None)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, res in out:
        assert not isinstance(res, str), res
        assert res == single, rank
