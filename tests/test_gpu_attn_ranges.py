"""GPU: the attention's key ranges per query tile do not change what a batch computes.

ComplEx at the production width (dim 200, rows of 400 floats: the asm read form) on a
517-entity graph: 17 key tiles, so 16 ranges are ranges of one and two tiles.  Every batch
holds at least 1,029 queries per step (17 query tiles; a query is a slot's distinct relation
with the kelpie entity as head), so ``KP_ATTN_RANGES=16`` launches
at least 272 one-shot workgroups, more than the 256 a device holds at once.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import numpy as np
import pytest

from golden_io import seed_all

import kelpie_amd as ka

pytestmark = pytest.mark.gpu

HP = {"optimizer_name": "Adagrad", "batch_size": 512, "epochs": 12, "lr": 0.043, "decay1": 0.9, "decay2": 0.999,
      "regularizer_name": "N3", "regularizer_weight": 0}
N_CANDS = 40


@pytest.fixture(scope="module")
def graph517():
    from kelpie_amd import synth
    g = synth.make_graph("small", seed=11, n_ent=517, n_rel=100, n_train=8000, n_valid=200, n_test=200)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    w = synth.make_weights("ComplEx", g.num_entities, g.num_relations, 200, seed=11, trained_scale=0.3)
    seen, preds = set(), []
    for t in g.test:
        t = tuple(int(v) for v in t)
        mine = ds.entity_to_training_triples.get(t[0], [])
        # 41 slots (40 candidates and the base), each with the entity's distinct relations as
        # head, less the removed triple's: at least 41 x 26 = 1,066 queries in every step
        rels = {r if h == t[0] else r + g.num_relations for h, r, _ in mine}
        if t[0] not in seen and len(mine) >= N_CANDS and 27 <= len(rels) and len(mine) <= 120:
            seen.add(t[0])
            preds.append(t)
    assert len(preds) >= 4
    items = [(p, [[c] for c in sorted(ds.entity_to_training_triples[p[0]])[:N_CANDS]]) for p in preds[:4]]
    return ds, w, items


def _details(eng):
    return [(pt["target_rank"], pt["target_score"], b["target_rank"], b["target_score"]) for pt, b in eng.last_results]


def _query_tiles(st):
    return (st["attn_queries"] + 63) // 64


def _ceil8(n):
    return (n + 7) // 8 * 8


def _same(a, b, what):
    assert len(a) == len(b) and len(a) >= N_CANDS, what
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[2] == y[2], (what, x, y)
        assert abs(x[1] - y[1]) <= 1e-4 * max(1.0, abs(y[1])), (what, x, y)
        assert abs(x[3] - y[3]) <= 1e-4 * max(1.0, abs(y[3])), (what, x, y)


def test_forced_ranges_agree_with_the_default_plan(graph517, monkeypatch):
    """The same batch with KP_ATTN_RANGES in {1, 2, 16} and with the planner's own choice:
    ranks equal, scores within 1e-4, and each setting bitwise equal to itself when run twice."""
    ds, w, items = graph517
    pred, rules = items[0]
    out, stats = {}, {}
    for setting in (None, "1", "2", "16"):
        if setting is None:
            monkeypatch.delenv("KP_ATTN_RANGES", raising=False)
        else:
            monkeypatch.setenv("KP_ATTN_RANGES", setting)
        model = ka.ComplEx(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=1e-3)
        runs = []
        for _ in range(2):
            seed_all(42)
            eng = ka.NecessaryPostTrainingEngine(model, ds, HP)
            rels = eng.compute_relevance_batch(pred, rules)
            runs.append((rels, _details(eng)))
            st = eng.last_batch_stats
        assert runs[0] == runs[1], setting
        model.close() if hasattr(model, "close") else None
        out[setting], stats[setting] = runs[0], st
        assert st["attn_queries"] >= 1029 and st["attn_inflight"] == 1, st
        if setting is not None:
            assert st["attn_ranges"] == int(setting) and st["attn_parts"] == int(setting), st
            assert st["attn_wg"] == _ceil8(_query_tiles(st) * int(setting)), st
    assert stats["16"]["attn_wg"] >= 272  # more workgroups than are resident at once
    assert 1 <= stats[None]["attn_ranges"] <= 16 and stats[None]["attn_wg"] <= 256, stats[None]
    for setting in ("1", "2", "16"):
        _same(out[setting][1], out[None][1], setting)
        assert np.allclose(out[setting][0], out[None][0], rtol=0, atol=1e-4), setting


def test_pipeline_hint_only_between_batches(graph517, monkeypatch):
    """Four batches through compute_relevance_pipeline with three in flight and with one:
    only the two middle batches of the deep call are planned with the in-flight hint (fewer
    ranges, one workgroup per unit); ranks equal, scores within 1e-4."""
    ds, w, items = graph517
    monkeypatch.delenv("KP_ATTN_RANGES", raising=False)
    monkeypatch.delenv("KP_ATTN_PART", raising=False)
    batches = [[it] for it in items]
    out = {}
    for depth in (3, 1):
        model = ka.ComplEx(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=1e-3)
        seed_all(42)
        eng = ka.NecessaryPostTrainingEngine(model, ds, HP)
        det = []
        finalize = eng._finalize_multi

        def recording(*a, _f=finalize, _e=eng, _d=det, **k):
            o = _f(*a, **k)
            _d.append(_details(_e))
            return o

        eng._finalize_multi = recording
        rels = eng.compute_relevance_pipeline(batches, depth=depth)
        out[depth] = (rels, det, eng.last_batch_stats)
        model.close() if hasattr(model, "close") else None
    assert [st["attn_inflight"] for st in out[3][2]] == [1, 3, 3, 1]
    assert [st["attn_inflight"] for st in out[1][2]] == [1, 1, 1, 1]
    for deep, flat in zip(out[3][2], out[1][2]):
        assert deep["attn_queries"] == flat["attn_queries"] >= 1029
        assert 1 <= deep["attn_ranges"] <= 16 and deep["attn_parts"] == deep["attn_ranges"], deep
        if deep["attn_inflight"] == 1:
            assert (deep["attn_ranges"], deep["attn_wg"]) == (flat["attn_ranges"], flat["attn_wg"])
        else:
            # one workgroup per (query tile, range) unit
            assert deep["attn_wg"] == _ceil8(_query_tiles(deep) * deep["attn_ranges"]), deep
    assert len(out[3][1]) == len(out[1][1]) == 4
    for b, (a3, a1) in enumerate(zip(out[3][1], out[1][1])):
        _same(a3, a1, f"batch {b}")
    for r3, r1 in zip(out[3][0], out[1][0]):
        assert np.allclose(r3, r1, rtol=0, atol=1e-4)
    # the first and last batch ran with the same plan either way: the same bits
    assert out[3][1][0] == out[1][1][0] and out[3][1][3] == out[1][1][3]
