"""The width and shape-edge cases of the step kernels (TEST INFRASTRUCTURE).

One table, read by the GPU tests (test_gpu_widths.py) and by their CPU companion
(test_width_cases_cpu.py): every row width the kernels are compiled for, the key-count
edges of the attention's 32-entity key tiles and the query-count edges of its 16-query
waves and 64-query tiles.  The reference of every case is the oracle
(oracle/kelpie_oracle.py) through cpu_backend.OracleBackedContext, for DistMult through
distmult_backend.DistMultOracleContext.

Per post-trained slot the oracle side records the score, the rank, the final row and the
oracle's own score row for (kelpie, p, .), and from that row the rank rule's bounds: with
delta = 1e-4 * max(1, |t|),
    maximizer (ComplEx, DistMult, ConvE):  [#{s_e >= t + delta}, #{s_e >= t - delta}]
    minimizer (TransE):                    [#{s_e <= t - delta}, #{s_e <= t + delta}]
over the entities e other than the ranked object that are not filtered, plus one where the
rank counts the object itself (include/kelpie_hip.h, out_rank: the minimizer restores the
ranked object before counting, the maximizer leaves a filtered object out).
"""
from __future__ import annotations

import functools

import numpy as np

import kelpie_amd as ka
from cpu_backend import OracleBackedContext
from distmult_backend import TOL, DistMultOracleContext, RecordingContext  # noqa: F401 (re-exported)
from golden_io import seed_all
from kelpie_amd import synth
from kelpie_amd.rng import ReferenceRNG

# test_gpu_parity.HP / CV_HP / TE_HP with fewer epochs
CX_HP = {"optimizer_name": "Adagrad", "batch_size": 512, "epochs": 8, "lr": 0.043, "decay1": 0.9, "decay2": 0.999,
         "regularizer_name": "N3", "regularizer_weight": 0}
CV_HP = {"batch_size": 512, "label_smoothing": 0.1, "lr": 0.0432, "decay": 0.995, "epochs": 8}
TE_HP = {"batch_size": 2048, "epochs": 8, "lr": 0.01, "margin": 5, "negative_triples_ratio": 5,
         "regularizer_weight": 1.0}
HUB_EPOCHS = 3
SATURATION = 16.0  # below the logit (~16.64) at which a float32 sigmoid is 1.0

DBS = (1, 2, 4, 8, 13, 16, 25)  # cx_pick_db's list (kp_complex.hip), restated


def pick_db(width):
    """cx_pick_db: the smallest compiled DB whose 16 * DB columns hold ``width``."""
    for db in DBS:
        if 16 * db >= width:
            return db
    return -1


def row_width(model, dim):
    return 2 * dim if model == "ComplEx" else dim


def te_inst(dim):
    """(VPL, NT) of kp_te_posttrain for a TransE dimension (kp_transe.hip)."""
    dp = (dim + 15) // 16 * 16
    return ((dp + 255) // 256, 512 if dp > 256 else 1024)


# ----------------------------------------------------------------------------- the case table
def _case(model, dim, n_ent=517, parts=("auto",), tag="", **kw):
    c = {"model": model, "dim": dim, "n_ent": n_ent, "parts": tuple(parts), "opt": "Adagrad", "reg": None,
         "norm": 2, "hub": False, "seed": 3}
    c.update(kw)
    if model == "TransE":
        c["inst"] = te_inst(dim)
        what = "VPL%d-NT%d" % c["inst"]
    else:
        c["db"] = pick_db(row_width(model, dim))
        what = "DB%d" % c["db"]
    c["id"] = f"{model}-d{dim}-{what}" + (f"-n{n_ent}" if n_ent != 517 else "") + (f"-{tag}" if tag else "")
    return c


BOTH = ("streamk", "ranges")

# ``seed`` (of the weights) is chosen per case so that the oracle alone meets check_vacuity
# the sweep: every compiled width, on the 517-entity graph (17 key tiles, 5 entities in the last)
SWEEP = [
    _case("ComplEx", 3, seed=8),          # row 6, odd half-width, padded
    _case("ComplEx", 12, seed=4),   # row 24: DB 2, which ComplEx reached in no test (DistMult d = 24 did)
    _case("ComplEx", 20, seed=4),         # row 40, padded
    _case("ComplEx", 32, seed=4),         # row 64, exact
    _case("ComplEx", 50),           # row 100, padded
    _case("ComplEx", 64),           # row 128, exact
    _case("ComplEx", 100),          # row 200: the asm read form at DB 13, 8 pad columns
    _case("ComplEx", 105, parts=BOTH),  # row 210: DB 16, 46 pad columns
    _case("ComplEx", 105, tag="Adam", opt="Adam", lr=0.01, seed=4),
    _case("ComplEx", 105, tag="N3", reg="N3"),
    _case("ComplEx", 128, parts=BOTH),  # row 256: DB 16, exact
    _case("ComplEx", 129),          # row 258: DB 25 with 142 pad columns
    _case("DistMult", 40, seed=4),
    _case("DistMult", 128, seed=5),
    _case("DistMult", 250, seed=4),
    _case("DistMult", 256),
    _case("ConvE", 100),
    _case("ConvE", 140),            # DB 13, asm form, 68 pad columns
    _case("ConvE", 240, parts=BOTH, seed=5),
    _case("ConvE", 300, seed=6),          # DB 25, FC 300 x 15,808
    _case("TransE", 50, seed=4),
    _case("TransE", 100, seed=4),
    _case("TransE", 256, seed=4),         # the last VPL = 1 width
    _case("TransE", 260),           # dp 272: VPL = 2, NT = 512
    _case("TransE", 260, tag="L1", norm=1),
    _case("TransE", 260, tag="hub", hub=True, seed=4),  # > 682 rows: the unstaged VPL = 2 kernel
    _case("TransE", 512),           # the documented maximum
]

# key-count edges: entity counts at the key tile's edges (a full last tile, one entity in the last
# tile, less than one tile)
EDGES = ([_case("ComplEx", d, n_ent=n, parts=("auto", "ranges") if n >= 512 else ("auto",),
                seed=4 if (d, n) == (128, 512) else 3)
          for d in (32, 128) for n in (31, 32, 33, 512, 513)]
         + [_case("ConvE", 100, n_ent=n, parts=("auto", "ranges"), seed=4 if n == 512 else 3) for n in (512, 513)]
         + [_case("TransE", 50, n_ent=n) for n in (33, 512)])

# query-count edges: queries per step launch at the wave (16) and query-tile (64) edges, as
# (slots, distinct relations per slot)
NQ_SPLIT = {1: (1, 1), 16: (2, 8), 17: (1, 17), 64: (4, 16), 65: (5, 13)}
QUERIES = [dict(_case(m, d, tag=f"nq{nq}"), nq=nq) for m, d in (("ComplEx", 128), ("ConvE", 100)) for nq in NQ_SPLIT]

# widths that other GPU tests already run: (model, mode, DB) -> the test
COVERED_BY = {
    ("ComplEx", "SOFTMAX_O", 1): "test_gpu_parity.py::test_complex_vs_oracle_full_width[8-False-auto-None]",
    ("ComplEx", "SOFTMAX_O", 25): "test_gpu_parity.py::test_complex_vs_oracle_full_width[200-False-streamk-None]",
    ("DistMult", "SOFTMAX_O", 1): "test_distmult_gpu.py::test_necessary_vs_standin[d8-DB1]",
    ("DistMult", "SOFTMAX_O", 2): "test_distmult_gpu.py::test_necessary_vs_standin[d24-DB2-padded]",
    ("DistMult", "SOFTMAX_O", 13): "test_distmult_gpu.py::test_necessary_vs_standin[d200-streamk]",
    ("DistMult", "SOFTMAX_O", 25): "test_distmult_gpu.py::test_necessary_vs_standin[d400-DB25]",
    ("ConvE", "BCE_O", 4): "test_gpu_parity.py::test_conve_vs_oracle_full_width[60-0.0-auto]",
    ("ConvE", "BCE_O", 13): "test_gpu_parity.py::test_conve_vs_oracle_full_width[200-0.2-streamk]",
}
# a ComplEx row is even and DistMult's d = 8 is DB 1 too, so DB 1 / 2 need no ConvE case:
# ConvE's smallest image (d = 60) is DB 4 and kp_conve.hip dispatches (KP_DB_DISPATCH) from that width
ATTN_MODE = {"ComplEx": "SOFTMAX_O", "DistMult": "SOFTMAX_O", "ConvE": "BCE_O"}


def ids(cases):
    return [c["id"] for c in cases]


def expand_parts(cases):
    """(case, partition) pairs as pytest params."""
    import pytest
    return [pytest.param(c, p, id=f"{c['id']}-{p}") for c in cases for p in c["parts"]]


# ----------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def graph(n_ent):
    """The 517-entity graph of the sweep, or an edge graph of ``n_ent`` entities; with its
    ordinary test subjects (8 to 40 training triples) and its hub."""
    if n_ent >= 500:
        g = synth.make_graph("small", seed=11, n_ent=n_ent, n_rel=40, n_train=6000, n_valid=200, n_test=200)
    else:
        g = synth.make_graph("tiny", seed=11, n_ent=n_ent, n_rel=6, n_train=360, n_valid=40, n_test=40)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    deg = ds.entity_to_degree
    test = [tuple(int(v) for v in t) for t in g.test]
    ordinary, seen = [], set()
    for t in test:
        if 8 <= deg.get(t[0], 0) <= 40 and t[0] not in seen:
            seen.add(t[0])
            ordinary.append(t)
    assert len(ordinary) >= 2, (n_ent, len(ordinary))
    hub = max(test, key=lambda t: deg.get(t[0], 0))
    return g, ds, ordinary, hub


@functools.lru_cache(maxsize=None)
def _weights(model, dim, n_ent, seed):
    g, ds, _, _ = graph(n_ent)
    if model == "ConvE":
        return synth.make_weights("ConvE", ds.num_entities, ds.num_relations, dim, seed=seed, conve_random_bn=True,
                                  trained_scale=0.5)
    if model == "TransE":
        # xavier rows of one common scale put every distance within a few per cent of the
        # others at d >= 100 (they concentrate like 1 / sqrt(d)), closer than the rank rule's
        # delta can separate over 517 entities; entity norms spread over 0.5 .. 4, as trained
        # tables have them, spread the distances instead
        w = synth.make_weights("TransE", ds.num_entities, ds.num_relations, dim, seed=seed)
        scale = np.exp(np.random.default_rng(1000 + seed).uniform(np.log(0.5), np.log(4.0), ds.num_entities))
        w["entity_embeddings"] = (w["entity_embeddings"] * scale[:, None]).astype(np.float32)
        return w
    return synth.make_weights(model, ds.num_entities, ds.num_relations, dim, seed=seed, trained_scale=0.3)


def make_model(case):
    """A fresh model of the case (its context is made on first use, or set by the caller)."""
    ds = graph(case["n_ent"])[1]
    w = _weights(case["model"], case["dim"], case["n_ent"], case["seed"])
    E, R = w["entity_embeddings"], w["relation_embeddings"]
    if case["model"] == "ComplEx":
        return ka.ComplEx(ds, E, R, init_scale=1e-3)
    if case["model"] == "DistMult":
        return ka.DistMult(ds, E, R, init_scale=1e-3)
    if case["model"] == "TransE":
        return ka.TransE(ds, E, R, norm=case["norm"])
    bn = {i: {"weight": w[f"bn{i}_weight"], "bias": w[f"bn{i}_bias"], "running_mean": w[f"bn{i}_mean"],
              "running_var": w[f"bn{i}_var"]} for i in (1, 2, 3)}
    return ka.ConvE(ds, E, R, w["conv_weight"].reshape(32, 3, 3), w["conv_bias"], w["fc_weight"], w["fc_bias"], bn=bn,
                    hidden_dropout_rate=0.2)


def hp_of(case):
    if case["model"] in ("ComplEx", "DistMult"):
        return dict(CX_HP, optimizer_name=case["opt"], lr=case.get("lr", 0.043), regularizer_name=case["reg"] or "N3",
                    regularizer_weight=0.05 if case["reg"] else 0)
    return dict(CV_HP) if case["model"] == "ConvE" else dict(TE_HP)


# ----------------------------------------------------------------------------- recorders
def rank_bounds(scores, target, filt, obj, minimizer=False):
    """[lo, hi] of the rank rule from one row of reference scores.  The ranked object scores
    exactly t on either side, so it is counted as the rank counts it (always by the
    minimizer, which restores it; by the maximizer unless it is filtered) and only the other
    entities are held against t -+ delta: the bounds of a target without a neighbour inside
    delta coincide."""
    s = np.asarray(scores, np.float64).copy()
    target = float(target)
    delta = TOL * max(1.0, abs(target))
    filt = np.asarray(filt, np.int64)
    own = 1 if minimizer or int(obj) not in set(filt.tolist()) else 0
    if minimizer:
        s[filt] = 1e6
        s[obj] = 2e6
        return own + int((s <= target - delta).sum()), own + int((s <= target + delta).sum())
    s[filt] = -1e6
    s[obj] = -2e6
    return own + int((s >= target + delta).sum()), own + int((s >= target - delta).sum())


class OracleRecorder:
    """The oracle-backed stand-in of a ComplEx, ConvE or TransE context that records, per
    post-trained slot in call order: score, rank, final row, the oracle's score row for
    (kelpie, p, .) and the rank rule's bounds from it."""

    def __init__(self, model):
        assert model.name in ("ComplEx", "ConvE", "TransE")
        self.inner = OracleBackedContext(model)
        self.minimizer = model.is_minimizer()
        self.slots = []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False):
        s, r, x = self.inner.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=True)
        for i in range(len(s)):
            kp = tuple(int(v) for v in pred[i])
            row = self.inner.om.all_scores([kp], kelpie_row=x[i])[0]
            assert float(row[kp[2]]) == float(s[i])
            lo, hi = rank_bounds(row, float(s[i]), filt[filt_off[i]:filt_off[i + 1]], kp[2], self.minimizer)
            self.slots.append({"score": float(s[i]), "rank": int(r[i]), "lo": lo, "hi": hi, "x": x[i].copy(),
                               "row": row, "n_rows": int(row_off[i + 1] - row_off[i])})
            if self.inner.model.name == "ConvE":
                pairs = np.unique(np.asarray(rows[row_off[i]:row_off[i + 1]], np.int64)[:, :2], axis=0)
                self.slots[-1]["max_logit"] = max(self._max_logit(pairs, v) for v in (x0[i], x[i]))
        return s, r, (x if want_x else None)

    def _max_logit(self, pairs, x):
        """The largest logit of the slot's (head, relation) pairs over [E; x], without dropout."""
        om = self.inner.om
        E = np.vstack([om.E, np.asarray(x, np.float32)[None]])
        enc, _ = om.conve_encode(E[pairs[:, 0]], om.R[pairs[:, 1]])
        return float((enc @ E.T).max())


def oracle_context(model):
    return DistMultOracleContext(model) if model.name == "DistMult" else OracleRecorder(model)


def device_context(model):
    return RecordingContext(model.ctx)


def check_slots(got, ref, rows):
    """Every slot of ``got`` against the oracle's record ``ref``: score within
    1e-4 * max(1, |ref|), rank inside the rank rule's bounds; with ``rows`` the final row
    within 1e-4 of its largest magnitude.  Returns (exact rank matches, largest row error
    relative to the row's largest magnitude): recorded by the callers, not asserted."""
    assert len(got) == len(ref) and len(ref) > 0, (len(got), len(ref))
    exact, worst = 0, 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        assert abs(a["score"] - b["score"]) <= TOL * max(1.0, abs(b["score"])), (i, a["score"], b["score"])
        assert b["lo"] <= a["rank"] <= b["hi"], (i, a["rank"], b["rank"], b["lo"], b["hi"])
        scale = float(np.abs(b["x"]).max())
        err = float(np.abs(a["x"] - b["x"]).max())
        if rows:
            assert err <= TOL * scale, (i, err, scale)
        worst = max(worst, err / scale if scale > 0 else err)
        exact += int(a["rank"] == b["rank"])
    return exact, worst


def check_vacuity(ref):
    """The rank rule must decide: every slot's bounds at most one apart, at least three
    quarters of the slots with one admissible rank, the oracle's own rank inside."""
    assert len(ref) > 0
    for i, b in enumerate(ref):
        assert b["hi"] - b["lo"] <= 1, (i, b["lo"], b["hi"])
        assert b["lo"] <= b["rank"] <= b["hi"], (i, b["rank"], b["lo"], b["hi"])
    sharp = sum(int(b["hi"] == b["lo"]) for b in ref)
    assert 4 * sharp >= 3 * len(ref), (sharp, len(ref))
    # ConvE: no logit of a training step near the saturated sigmoid.  torch's float32 sigmoid
    # (and the device's) is 1.0 from a logit of ~16.64, where the BCE gradient becomes 0; the
    # oracle's step rounds a float64 sigmoid, which is 1.0 only from ~17.33, so a logit in
    # between moves the two apart (width sweep).  The hidden dropout
    # scales the kept units by 1.25, hence the margin on the logits without dropout.
    for i, b in enumerate(ref):
        assert 1.25 * b.get("max_logit", 0.0) < SATURATION, (i, b["max_logit"])


# ----------------------------------------------------------------------------- running a case
def subjects(case):
    """[(pred, epochs, candidates)]: two ordinary subjects with two singleton candidates
    each, or (``hub``) the hub subject with one candidate in a batch of its own."""
    _, ds, ordinary, hub = graph(case["n_ent"])
    hp = hp_of(case)
    if case["hub"]:
        return [(hub, HUB_EPOCHS, 1)]
    return [(p, hp["epochs"], 2) for p in ordinary[:2]]


def hub_rows(case):
    """Rows (triples and inverses) of the hub subject's smallest slot: the one with the
    candidate removed."""
    _, ds, _, hub = graph(case["n_ent"])
    return 2 * (len(ds.entity_to_training_triples[hub[0]]) - 1)


def run_necessary(case, ctx_of):
    """The case's necessary-mode batches through ``ctx_of(model)``; the recorded slots."""
    ds = graph(case["n_ent"])[1]
    model = make_model(case)
    model._ctx = ctx_of(model)
    seed_all(42)
    for pred, epochs, n in subjects(case):
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(hp_of(case), epochs=epochs))
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        eng.compute_relevance_batch(pred, [[c] for c in cands])
    return model.ctx.slots


def query_batch(case, model):
    """The query-count edges' direct posttrain_rank arguments: ``slots`` slots whose rows are (K, r, t)
    for ``k`` distinct relations r (and their inverses, whose heads are frozen), so that a
    step launch has exactly slots * k queries."""
    n_slots, k = NQ_SPLIT[case["nq"]]
    ds = model.dataset
    K, nr, d = ds.num_entities, ds.num_relations, model.dimension
    rng = np.random.default_rng(100 + case["nq"])
    hp = dict(hp_of(case))
    if model.name == "ConvE":
        x0 = (rng.standard_normal((n_slots, d)) * 0.5).astype(np.float32)
    else:
        x0 = (rng.random((n_slots, d)) * 0.2).astype(np.float32)
    row_off, rows, pred, draws = [0], [], [], []
    seed_all(42)
    for s in range(n_slots):
        rels = rng.permutation(nr)[:k]
        tails = rng.permutation(K)[:k]
        t = np.stack([np.full(k, K), rels, tails], 1).astype(np.int64)
        inv = t[:, [2, 1, 0]].copy()
        inv[:, 1] += nr
        r = np.vstack([t, inv])
        rows.append(r)
        row_off.append(row_off[-1] + len(r))
        pred.append((K, int(rels[0]), int(rng.integers(K))))
        draws.append(np.asarray(model.posttrain_draws(r, hp, ReferenceRNG()), np.int32))
    rng_off = np.concatenate([[0], np.cumsum([len(v) for v in draws])]).astype(np.int64)
    filt_off = np.arange(n_slots + 1) * 2
    filt = rng.integers(0, K, 2 * n_slots).astype(np.int64)
    return (model.kp_hp(hp), x0, np.array(row_off), np.vstack(rows), rng_off, np.concatenate(draws).astype(np.int32),
            np.array(pred), filt_off, filt)


def run_queries(case, ctx_of):
    model = make_model(case)
    model._ctx = ctx_of(model)
    args = query_batch(case, model)
    model.ctx.posttrain_rank(*args, want_x=True)
    return model.ctx.slots, model


_REF = {}


def reference(case):
    """The oracle side of a case, computed once and shared by the runs that differ only in
    how the device partitions or contracts its attention."""
    if case["id"] not in _REF:
        run = run_queries if "nq" in case else run_necessary
        out = run(case, oracle_context)
        _REF[case["id"]] = out[0] if isinstance(out, tuple) else out
    return _REF[case["id"]]


def score_pairs(case):
    """About 16 (head, relation) pairs, one inverse relation among them."""
    ds = graph(case["n_ent"])[1]
    n = min(16, ds.num_entities)
    heads = (np.arange(n) * 31 + 5) % ds.num_entities
    rels = np.arange(n) % ds.num_relations
    rels[3] += ds.num_relations
    return heads.astype(np.int64), rels.astype(np.int64)


def reference_scores(case, model):
    """all_scores of score_pairs: the fp64 product for ComplEx and DistMult, the oracle's
    all_scores for ConvE and TransE."""
    heads, rels = score_pairs(case)
    if model.name in ("ComplEx", "DistMult"):
        E, R = model.entity_embeddings.astype(np.float64), model.relation_embeddings.astype(np.float64)
        if model.name == "DistMult":
            return (E[heads] * R[rels]) @ E.T
        d = model.real_dimension
        a, b, c, e = E[heads, :d], E[heads, d:], R[rels, :d], R[rels, d:]
        return np.concatenate([a * c - b * e, a * e + b * c], 1) @ E.T
    return np.asarray(OracleBackedContext(model).all_scores(heads, rels), np.float64)
