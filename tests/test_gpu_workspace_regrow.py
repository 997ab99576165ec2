"""A context's named device workspaces across batches of different sizes.

The workspaces grow on demand and are shared by name between the model files and the
rank path (kp_common.hpp).  Two buffers that alias each other, or a pointer kept across a
regrowth, would not raise: they would give wrong ranks.  So, per model family, on ONE
engine and context: a batch of 2 candidates, then one of 12 (every per-slot buffer
regrows: 12 + 1 slots is more than the 25 % headroom over 2 + 1), then the first 2
again.  The third result must equal the first bit for bit, and the middle one must equal
the same 12 candidates on a fresh context.  D = 200 for ComplEx and ConvE (the bf16x3
attention, the fused ConvE encoder), D = 32 for TransE; 3 epochs.

The rank's four sets of rows (the slots, the probes, the marks, the fp64 call's slots) share one
workspace type, so the same sequence runs once more with every request on -- the lists, two
probes, the trace, two marks and the margins -- at the narrowest widths that still reach every
buffer (ComplEx rows of 32 floats, TransE d = 16, ConvE d = 60), and every reported value has
to come back.

The ComplEx / DistMult step's workspaces are one type held twice, for fp32 and for fp64: two
instances bound, sized or indexed as each other would again only give wrong numbers.  So the
sequence runs with ``precision = "fp64"`` as well, and once with an fp32 batch of every request
regrowing the fp32 instance between two equal fp64 batches on one context."""
import pytest

from golden_io import seed_all

import kelpie_amd as ka

pytestmark = pytest.mark.gpu

HP = {
    "ComplEx": {"optimizer_name": "Adagrad", "batch_size": 512, "epochs": 3, "lr": 0.043, "decay1": 0.9,
                "decay2": 0.999, "regularizer_name": "N3", "regularizer_weight": 0},
    "TransE": {"batch_size": 2048, "epochs": 3, "lr": 0.01, "margin": 5, "negative_triples_ratio": 5,
               "regularizer_weight": 1.0},
    "ConvE": {"batch_size": 512, "label_smoothing": 0.1, "lr": 0.0432, "decay": 0.995, "epochs": 3},
}
DIM = {"ComplEx": 200, "TransE": 32, "ConvE": 200}


def _model(name, ds, w):
    if name == "ComplEx":
        return ka.ComplEx(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=1e-3)
    if name == "TransE":
        return ka.TransE(ds, w["entity_embeddings"], w["relation_embeddings"], norm=2)
    bn = {i: {"weight": w[f"bn{i}_weight"], "bias": w[f"bn{i}_bias"], "running_mean": w[f"bn{i}_mean"],
              "running_var": w[f"bn{i}_var"]} for i in (1, 2, 3)}
    return ka.ConvE(ds, w["entity_embeddings"], w["relation_embeddings"], w["conv_weight"].reshape(32, 3, 3),
                    w["conv_bias"], w["fc_weight"], w["fc_bias"], bn=bn, hidden_dropout_rate=0.2)


def _run(eng, pred, cands):
    """One batch from a cleared cache and fixed seeds: the relevances and every
    (post-trained, base) rank and score."""
    seed_all(42)
    eng.set_cache()
    rels = eng.compute_relevance_batch(pred, [[c] for c in cands])
    return rels, [(pt["target_rank"], pt["target_score"], b["target_rank"], b["target_score"])
                  for pt, b in eng.last_results]


@pytest.mark.parametrize("name", ["ComplEx", "TransE", "ConvE"])
def test_workspaces_survive_regrowth(name):
    from kelpie_amd import synth
    g = synth.make_graph("small", seed=9)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    extra = {"conve_random_bn": True, "trained_scale": 0.5} if name == "ConvE" else {}
    w = synth.make_weights(name, g.num_entities, g.num_relations, DIM[name], seed=9, **extra)
    deg = ds.entity_to_degree
    pred = next(tuple(int(v) for v in t) for t in g.test if 12 <= deg.get(int(t[0]), 0) <= 40)
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:12]
    assert len(cands) == 12

    eng = ka.NecessaryPostTrainingEngine(_model(name, ds, w), ds, HP[name])
    first = _run(eng, pred, cands[:2])
    middle = _run(eng, pred, cands)
    again = _run(eng, pred, cands[:2])
    fresh = _run(ka.NecessaryPostTrainingEngine(_model(name, ds, w), ds, HP[name]), pred, cands)

    assert len(first[1]) == 2 and len(middle[1]) == 12
    assert again == first, (first, again)
    assert middle == fresh, (middle, fresh)


DIM_NARROW = {"ComplEx": 16, "TransE": 16, "ConvE": 60}  # ComplEx: rows of 2 * 16 floats


def _extras_engine(name, ds, w, model=None):
    eng = ka.NecessaryPostTrainingEngine(model or _model(name, ds, w), ds, HP[name])
    eng.top_k = 3
    eng.trace = True
    eng.marks = [1, 3]
    eng.margin_tol = 1e-4
    return eng


def _run_extras(eng, pred, cands, probes):
    """One batch from a cleared cache and fixed seeds with every request on: the reports and the
    whole (post-trained, base) results -- score, rank, lists, probes, loss, marks, margins."""
    seed_all(42)
    eng.set_cache()
    reports = eng.compute_side_effects(pred, [[c] for c in cands], probes=probes)
    return reports, list(eng.last_results)


@pytest.mark.parametrize("name", ["ComplEx", "TransE", "ConvE"])
def test_workspaces_survive_regrowth_with_every_request(name):
    from kelpie_amd import synth
    g = synth.make_graph("small", seed=9)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    extra = {"conve_random_bn": True, "trained_scale": 0.5} if name == "ConvE" else {}
    w = synth.make_weights(name, g.num_entities, g.num_relations, DIM_NARROW[name], seed=9, **extra)
    train = ds.entity_to_training_triples
    pred = next(tuple(int(v) for v in t) for t in g.test if 14 <= len(train.get(int(t[0]), ())) <= 40)
    own = sorted(train[pred[0]])
    cands, probes = own[:12], own[12:14]  # two training triples of the subject that are no candidates
    assert len(cands) == 12 and len(probes) == 2

    eng = _extras_engine(name, ds, w)
    first = _run_extras(eng, pred, cands[:2], probes)
    middle = _run_extras(eng, pred, cands, probes)
    again = _run_extras(eng, pred, cands[:2], probes)
    fresh = _run_extras(_extras_engine(name, ds, w), pred, cands, probes)

    assert len(first[1]) == 2 and len(middle[1]) == 12
    for pt, _ in middle[1]:  # every request reached the results
        assert 0 < len(pt["top_ids"]) == len(pt["top_scores"]) <= 3
        assert len(pt["probes"]) == 2 and len(pt["marks"]) == 2
        assert pt["loss"] and pt["margins"]["tol"] == 1e-4
    assert again == first, (first, again)
    assert middle == fresh, (middle, fresh)


FP64 = {"ComplEx": 16, "DistMult": 24}  # rows of 32 floats (DB 2) and of 24 padded to 32 (DB 2)


def _fp64_model(name, ds, g, seed=9):
    from kelpie_amd import synth
    w = synth.make_weights(name, g.num_entities, g.num_relations, FP64[name], seed=seed)
    cls = ka.ComplEx if name == "ComplEx" else ka.DistMult
    return cls(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=1e-3)


def _fp64_engine(model, ds):
    eng = ka.NecessaryPostTrainingEngine(model, ds, HP["ComplEx"])
    eng.precision = "fp64"
    return eng


@pytest.mark.parametrize("name", ["ComplEx", "DistMult"])
def test_workspaces_survive_regrowth_fp64(name):
    from kelpie_amd import synth
    g = synth.make_graph("small", seed=9)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    deg = ds.entity_to_degree
    pred = next(tuple(int(v) for v in t) for t in g.test if 12 <= deg.get(int(t[0]), 0) <= 40)
    cands = sorted(ds.entity_to_training_triples[pred[0]])[:12]
    assert len(cands) == 12

    eng = _fp64_engine(_fp64_model(name, ds, g), ds)
    first = _run(eng, pred, cands[:2])
    middle = _run(eng, pred, cands)
    again = _run(eng, pred, cands[:2])
    fresh = _run(_fp64_engine(_fp64_model(name, ds, g), ds), pred, cands)

    assert len(first[1]) == 2 and len(middle[1]) == 12
    assert all(isinstance(v[1], float) and v[1] == v[1] for v in middle[1])  # the fp64 scores, none a NaN
    assert again == first, (first, again)
    assert middle == fresh, (middle, fresh)


def test_fp64_survives_fp32_requests():
    """The mirror of test_f64_gpu.py's test_fp32_results_are_unchanged_by_an_fp64_call, with
    regrowth between: an fp64 batch of 2, an fp32 batch of 12 with every request on, the fp64
    batch of 2 again, all on one context."""
    from kelpie_amd import synth
    g = synth.make_graph("small", seed=9)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    w = synth.make_weights("ComplEx", g.num_entities, g.num_relations, FP64["ComplEx"], seed=9)
    train = ds.entity_to_training_triples
    pred = next(tuple(int(v) for v in t) for t in g.test if 14 <= len(train.get(int(t[0]), ())) <= 40)
    own = sorted(train[pred[0]])
    cands, probes = own[:12], own[12:14]

    model = _model("ComplEx", ds, w)
    eng64 = _fp64_engine(model, ds)
    first = _run(eng64, pred, cands[:2])
    middle = _run_extras(_extras_engine("ComplEx", ds, w, model), pred, cands, probes)
    again = _run(eng64, pred, cands[:2])
    fresh = _run_extras(_extras_engine("ComplEx", ds, w), pred, cands, probes)

    assert len(first[1]) == 2 and len(middle[1]) == 12
    assert again == first, (first, again)
    assert middle == fresh, (middle, fresh)
