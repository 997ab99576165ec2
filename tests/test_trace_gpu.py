"""The post-training trace on the device (ComplEx, DistMult, TransE and ConvE; kp_posttrain_rank_trace).

1. Against the reference: every step of every post-training of tests/golden/trace_golden.json
   (the reference's own ``step_on_batch`` returns, fp32 and fp64 runs) within
   ``max(1e-4 * max(1, |l64|), 2 * |l32 - l64|)``; the second clause is counted and must
   never be needed.
2. Against the definition (trace_reference.py) at the compiled widths: one step per epoch,
   1 to 4 epochs, the k-epoch trace's last value against the restatement on the
   (k - 1)-epoch run's final row.
3. Nothing else moves: rows, scores, ranks, top-k lists and probes are bitwise those without
   the trace; the trace is bitwise the same from two fresh contexts.
4. Shape edges: the crafted batch of test_distmult_gpu.py at batch sizes that leave a last
   step of one row.
5. Errors: a wrong ``trace_off`` and a NULL ``out_loss`` are refused with the rule's message
   and the context serves the next call.

Every graph has at most 517 entities.  Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import trace_cases as tc
import trace_reference as tr
import kelpie_amd as ka
from kelpie_amd import _lib, synth

pytestmark = pytest.mark.gpu


def _hp(hp):
    """MultiClassNLLModel.kp_hp."""
    name = hp["optimizer_name"]
    return _lib.HP(optimizer=_lib.KP_OPT[name], epochs=int(hp["epochs"]), batch_size=int(hp["batch_size"]),
                   lr=float(hp["lr"]), beta1=float(hp.get("decay1", 0.9)), beta2=float(hp.get("decay2", 0.999)),
                   eps=1e-10 if name == "Adagrad" else 1e-8, reg_weight=float(hp.get("regularizer_weight", 0.0)),
                   reg_kind=_lib.KP_REG[hp.get("regularizer_name", "N3")])


def _te_hp(hp):
    """TransE.kp_hp."""
    return _lib.HP(optimizer=_lib.KP_OPT["Adam"], epochs=int(hp["epochs"]), batch_size=int(hp["batch_size"]),
                   lr=float(hp["lr"]), beta1=0.9, beta2=0.999, eps=1e-8, reg_weight=float(hp["regularizer_weight"]),
                   margin=float(hp["margin"]), neg_ratio=int(hp["negative_triples_ratio"]))


TE_HP = {"batch_size": 2048, "epochs": 4, "lr": 0.01, "margin": 5, "negative_triples_ratio": 5,
         "regularizer_weight": 1.0}
HP = {"optimizer_name": "Adagrad", "batch_size": 512, "epochs": 4, "lr": 0.043, "decay1": 0.9, "decay2": 0.999,
      "regularizer_name": "N3", "regularizer_weight": 0.05}


def _batch(slots, K, n_rel, epochs, seed=0, transe=False):
    """posttrain_rank's arrays for ``slots`` = [(kelpie-form triples, ranked triple)]: the rows
    with their inverses, one permutation per epoch and slot (``transe``: [row order | negative
    entity in [0, K] | head_or_tail] per epoch), no filter."""
    rng = np.random.default_rng(seed)
    row_off, rows, pred, perms, rng_off = [0], [], [], [], [0]
    for trip, p in slots:
        t = np.array(trip, np.int64).reshape(-1, 3)
        inv = t[:, [2, 1, 0]].copy()
        inv[:, 1] += n_rel
        rows.append(np.vstack([t, inv]))
        row_off.append(row_off[-1] + 2 * len(t))
        pred.append(p)
        R = 2 * len(t)
        if transe:
            pm = [np.concatenate([rng.permutation(R), rng.integers(0, K + 1, R), rng.integers(0, 2, R)])
                  for _ in range(epochs)]
        else:
            pm = [rng.permutation(R) for _ in range(epochs)]
        perms.append(pm)
        rng_off.append(rng_off[-1] + epochs * len(pm[0]) if epochs else rng_off[-1])
    flat = np.concatenate([np.concatenate(pm) for pm in perms if len(pm) and len(pm[0])] or [np.zeros(0)])
    n = len(slots)
    return {"row_off": np.array(row_off, np.int32), "rows": np.vstack(rows).astype(np.int32),
            "rng_off": np.array(rng_off, np.int64), "rng": flat.astype(np.int32), "pred": np.array(pred, np.int32),
            "filt_off": np.zeros(n + 1, np.int32), "filt": np.zeros(1, np.int32), "perms": perms}


def _conve_model(g, w, rates=(0.0, 0.0, 0.0)):
    """A ka.ConvE over synth.make_weights' dict with the dropout rates (input, feature map, hidden)."""
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    bn = {i: {"weight": w[f"bn{i}_weight"], "bias": w[f"bn{i}_bias"], "running_mean": w[f"bn{i}_mean"],
              "running_var": w[f"bn{i}_var"]} for i in (1, 2, 3)}
    return ka.ConvE(ds, w["entity_embeddings"], w["relation_embeddings"], w["conv_weight"].reshape(32, 3, 3),
                    w["conv_bias"], w["fc_weight"], w["fc_bias"], bn=bn, input_dropout_rate=rates[0],
                    feature_map_dropout_rate=rates[1], hidden_dropout_rate=rates[2])


CV_HP = {"batch_size": 512, "epochs": 3, "label_smoothing": 0.1, "lr": 0.0432, "decay": 0.995}


def _conve_bits(model, b, hp, seed=0):
    """Random keep bits for every slot of batch ``b`` in kp_batch.rng's ConvE layout; also the
    first step's masks of every slot as multipliers (None where a rate is 0)."""
    rng = np.random.default_rng(seed)
    segs = model.dropout_segments()
    words, off, first = [], [0], []
    for i in range(len(b["row_off"]) - 1):
        rows = b["rows"][b["row_off"][i]:b["row_off"][i + 1]]
        steps = model.er_vocab_sizes(rows, int(hp["batch_size"]), int(hp["epochs"])) if len(rows) else []
        mine, masks = [], []
        for j, n_pairs in enumerate(steps):
            for n, p in segs:
                if p == 0:
                    masks.append(None) if j == 0 else None
                    continue
                keep = (rng.random(n_pairs * n) < 1.0 - p).astype(np.uint8)
                if j == 0:
                    masks.append(keep.reshape(n_pairs, n) * float(np.float32(1.0) / np.float32(1.0 - p)))
                keep = np.concatenate([keep, np.zeros(-len(keep) % 32, np.uint8)])
                mine.append(np.packbits(keep, bitorder="little").view(np.uint32))
        first.append(masks)
        words += mine
        off.append(off[-1] + sum(len(m) for m in mine))
    flat = np.concatenate(words).view(np.int32) if words else np.zeros(1, np.int32)
    return dict(b, rng=flat, rng_off=np.array(off, np.int64)), first


def _run(ctx, hp, x0, b, **kw):
    return ctx.posttrain_rank(hp, x0, b["row_off"], b["rows"], b["rng_off"], b["rng"], b["pred"], b["filt_off"],
                              b["filt"], **kw)


# --------------------------------------------------------------------------- 1. against the reference
@functools.lru_cache(maxsize=None)
def _golden_ctx(name):
    case = next(c for c in tc.golden()["cases"] if c["name"] == name)
    if case["model"] == "ConvE":
        return _conve_model(tc.graph(), tc.conve_weights(name), case["posttrainings"][0]["rates"])
    model, E, R = tc.tables(name)
    if model == "TransE":
        norm = next(c for c in tc.golden()["cases"] if c["name"] == name)["weights"]["norm"]
        return _lib.Context(model, E, R, norm_p=norm)
    return _lib.Context(model, E, R)


_CLAUSE2 = []  # steps that needed the reference's own spread, over every case run so far


@pytest.mark.parametrize("pid,case,pt", tc.posttrainings(), ids=lambda v: v if isinstance(v, str) else "")
def test_trace_vs_reference(pid, case, pt):
    ctx = _golden_ctx(case["name"])
    w = tc.width(case)
    rows = np.asarray(pt["rows"], np.int32)
    R, E = len(rows), pt["hp"]["epochs"]
    x0 = tc.x0(case)[None, :w]
    K = pt["kelpie"]
    if case["model"] == "ConvE":  # the context's model knows the dropout rates; the draws are the keep bits
        hp, draws, ctx = ctx.kp_hp(pt["hp"]), np.asarray(pt["rng"] or [0], np.int32), ctx.ctx
    elif case["model"] == "TransE":
        hp, draws = _te_hp(pt["hp"]), np.concatenate(pt["rng"]).astype(np.int32)
    else:
        hp, draws = _hp(pt["hp"]), np.concatenate(pt["perms"]).astype(np.int32)
    assert case["model"] == "ConvE" or len(draws) % (E * R) == 0
    out = ctx.posttrain_rank(hp, x0, [0, R], rows, [0, len(draws)], draws, [[K, int(rows[0][1]), 0]], [0, 0],
                             np.zeros(1, np.int32), trace=True)
    loss = out[-1][0]
    assert len(loss) == len(pt["steps"])
    worst = 0.0
    for j, (v, s) in enumerate(zip(loss.tolist(), pt["steps"])):
        err, tol1 = abs(v - s["l64"]), tc.TOL * max(1.0, abs(s["l64"]))
        worst = max(worst, err / max(1.0, abs(s["l64"])))
        assert err <= max(tol1, 2 * abs(s["l32"] - s["l64"])), (pid, j, v, s["l32"], s["l64"])
        if err > tol1:
            _CLAUSE2.append((pid, j, v, s["l32"], s["l64"]))
    print(f"{pid}: {len(loss)} steps, worst |dev - l64| / max(1, |l64|) = {worst:.3g}")
    # a trace that leans on the reference's spread is a failure to look at, not a pass
    assert not _CLAUSE2, _CLAUSE2


# --------------------------------------------------------------------------- 2. against the definition
@functools.lru_cache(maxsize=None)
def _graph(n_ent):
    return synth.make_graph("tiny", seed=5, n_ent=n_ent)


def _subject_rows(g, lo=10, hi=40):
    """The kelpie-form training triples of a subject with lo .. hi of them."""
    deg = np.bincount(np.concatenate([g.train[:, 0], g.train[:, 2]]), minlength=g.num_entities)
    s = int(next(e for e in range(g.num_entities) if lo <= deg[e] <= hi))
    t = g.train[(g.train[:, 0] == s) | (g.train[:, 2] == s)].astype(np.int64).copy()
    K = g.num_entities
    t[:, 0][t[:, 0] == s] = K
    t[:, 2][t[:, 2] == s] = K
    return [tuple(int(v) for v in r) for r in t]


WIDTHS = [  # model, row width, entities, attention partition, regulariser
    pytest.param("ComplEx", 6, 300, None, "N3", id="complex-6-DB1"),
    pytest.param("ComplEx", 256, 300, None, "N2", id="complex-256-DB16"),
    pytest.param("ComplEx", 400, 300, None, "N3", id="complex-400-DB25"),
    pytest.param("ComplEx", 400, 513, "ranges", "N3", id="complex-400-513-ranges"),
    pytest.param("DistMult", 200, 300, None, "N3", id="distmult-200-DB13"),
]


@pytest.mark.parametrize("model,width,n_ent,part,reg", WIDTHS)
def test_trace_vs_definition_at_compiled_widths(model, width, n_ent, part, reg, monkeypatch):
    if part:
        monkeypatch.setenv("KP_ATTN_PART", part)
    g = _graph(n_ent)
    dim = width // 2 if model == "ComplEx" else width
    w = synth.make_weights(model, g.num_entities, g.num_relations, dim, seed=5, trained_scale=0.3)
    E, R = w["entity_embeddings"], w["relation_embeddings"]
    assert E.shape == (n_ent, width)
    ctx = _lib.Context(model, E, R)
    K = n_ent
    trip = _subject_rows(g)
    b = _batch([(trip, (K, trip[0][1], 1))], K, g.num_relations, 0)
    x0 = (np.random.default_rng(9).random((1, width)) * 0.5).astype(np.float32)
    hp = dict(HP, regularizer_name=reg, batch_size=2 * len(trip))  # one step per epoch
    prev_x, prev_loss = x0, []
    for k in (1, 2, 3, 4):
        s, r, x, loss = _run(ctx, _hp(dict(hp, epochs=k)), x0, b, want_x=True, trace=True)
        loss = loss[0]
        assert len(loss) == k and np.array_equal(loss[:k - 1], prev_loss)  # the same draws as a prefix
        want = tr.step_loss(model, E, R, prev_x[0], b["rows"], reg, hp["regularizer_weight"])
        print(f"{model} {width} epochs {k}: device {loss[-1]:.9g} definition {want:.12g}")
        assert tc.within(float(loss[-1]), want), (k, float(loss[-1]), want)
        prev_x, prev_loss = x, loss
    if part == "ranges":
        plan = ctx.last_attn_plan()
        assert plan["attn_parts"] >= 2, plan  # several splits per query
        assert n_ent % 32 == 1  # one entity in the last key tile
    ctx.close()


def _hub(n_ent, n_rel, copies):
    """A crafted hub: the kelpie entity linked to every entity under ``copies`` relations."""
    K = n_ent
    return [(K, r, e) if (e + r) % 2 else (e, r, K) for r in range(copies) for e in range(n_ent)]


TE_WIDTHS = [  # row width, norm, rows: the ordinary subject, or the hub (slots too long for the LDS staging)
    pytest.param(16, 2, "subject", 5, id="transe-16"),
    pytest.param(16, 1, "hub", 1, id="transe-16-L1-hub-ratio1"),  # 1,800 work items: four record chunks per step
    pytest.param(260, 2, "hub", 5, id="transe-260-VPL2-hub"),
]


@pytest.mark.parametrize("width,norm,which,ratio", TE_WIDTHS)
def test_transe_trace_vs_definition_at_compiled_widths(width, norm, which, ratio):
    g = _graph(300)
    w = synth.make_weights("TransE", g.num_entities, g.num_relations, width, seed=5)
    E, R = w["entity_embeddings"], w["relation_embeddings"]
    ctx = _lib.Context("TransE", E, R, norm_p=norm)
    K = g.num_entities
    trip = _subject_rows(g) if which == "subject" else _hub(K, g.num_relations, 3)
    n_rows = 2 * len(trip)
    assert (n_rows > 1365) == (which == "hub")  # past what the kernel stages in LDS at either workgroup size
    b = _batch([(trip, (K, trip[0][1], 1))], K, g.num_relations, 4, seed=2, transe=True)
    x0 = (np.random.default_rng(9).standard_normal((1, width)) * 0.3).astype(np.float32)
    hp = dict(TE_HP, batch_size=n_rows, negative_triples_ratio=ratio)  # one step per epoch
    prev_x, prev_loss = x0, []
    for k in (1, 2, 3, 4):
        s, r, x, loss = _run(ctx, _te_hp(dict(hp, epochs=k)), x0, b, want_x=True, trace=True)
        loss = loss[0]
        assert len(loss) == k and np.array_equal(loss[:k - 1], prev_loss)  # the same draws as a prefix
        pos, neg = tr.transe_batches(b["rows"], b["perms"][0][k - 1], hp["negative_triples_ratio"], n_rows, 0)
        want = tr.transe_step_loss(E, R, prev_x[0], pos, neg, norm, hp["margin"], hp["regularizer_weight"])
        print(f"TransE {width} L{norm} {which} epochs {k}: device {loss[-1]:.9g} definition {want:.12g}")
        assert tc.within(float(loss[-1]), want), (k, float(loss[-1]), want)
        prev_x, prev_loss = x, loss
    ctx.close()


# --------------------------------------------------------------------------- 3. nothing else moves
def _multi_slot_case(model, width, n_ent=300):
    g = _graph(n_ent)
    dim = width // 2 if model == "ComplEx" else width
    w = synth.make_weights(model, g.num_entities, g.num_relations, dim, seed=7,
                           trained_scale=None if model in ("TransE", "ConvE") else 0.3)
    K = n_ent
    trip = _subject_rows(g)
    slots = [(trip, (K, trip[0][1], trip[0][2] if trip[0][0] == K else 3)), (trip[:-2], (K, trip[1][1], K)),
             ([], (K, 2, 9)), (trip[1:], (K, trip[2][1], 5))]
    b = _batch(slots, K, g.num_relations, HP["epochs"], seed=3, transe=model == "TransE")
    x0 = (np.random.default_rng(11).random((len(slots), width)) * 0.5).astype(np.float32)
    # probes: two per slot with rows, none for the empty one
    p_off = np.array([0, 2, 4, 4, 6], np.int32)
    probes = np.array([[0, 1], [3, K], [1, 7], [2, 8], [4, 2], [5, K]], np.int32)
    pf_off = np.array([0, 1, 1, 3, 3, 3, 4], np.int32)
    pf = np.array([4, 6, 7, 9], np.int32)
    return w, b, x0, (p_off, probes, pf_off, pf)


@pytest.mark.parametrize("model,width", [("ComplEx", 16), ("DistMult", 200), ("TransE", 16), ("ConvE", 60)])
def test_trace_moves_nothing_else_and_is_deterministic(model, width):
    w, b, x0, probes = _multi_slot_case(model, width)
    # several steps per epoch, a shorter last one
    hp = _te_hp(dict(TE_HP, batch_size=7)) if model == "TransE" else _hp(dict(HP, batch_size=7))
    if model == "ConvE":  # all three dropouts
        cv = _conve_model(_graph(300), w, (0.2, 0.3, 0.1))
        hpd = dict(CV_HP, batch_size=7, epochs=HP["epochs"])
        hp, (b, _) = cv.kp_hp(hpd), _conve_bits(cv, b, hpd, seed=4)
    runs = []
    for trace in (False, True, True):
        # a fresh context
        ctx = cv._make_ctx() if model == "ConvE" else _lib.Context(model, w["entity_embeddings"], w["relation_embeddings"])
        runs.append(_run(ctx, hp, x0, b, want_x=True, topk=5, probes=probes, **({"trace": True} if trace else {})))
        ctx.close()
    plain, traced, again = runs
    assert len(plain) == 5 and len(traced) == 6
    for a, t in zip(plain, traced[:5]):
        for u, v in zip(a if isinstance(a, tuple) else (a,), t if isinstance(t, tuple) else (t,)):
            assert u.dtype == v.dtype and np.array_equal(u, v, equal_nan=True) and u.tobytes() == v.tobytes()
    steps = _lib.trace_steps(model, hp, b["row_off"], b["rows"]).tolist()
    assert [len(v) for v in traced[5]] == steps and steps[2] == 0 and min(steps[0], steps[1], steps[3]) > hp.epochs
    for u, v in zip(traced[5], again[5]):
        assert u.tobytes() == v.tobytes()
    assert all(np.isfinite(v).all() for v in traced[5])


# --------------------------------------------------------------------------- 4. shape edges
def _crafted(K, nr, epochs):
    """test_distmult_gpu._crafted's slots: a self-loop (K, r, K) and its inverse; no rows at
    all; rows repeating one relation and one frozen (h, r) pair; a ranked kelpie object."""
    slots = [
        ([(K, 3, K), (K, 3, 17), (40, 5, K)], (K, 3, 17)),
        ([], (K, 2, 9)),
        ([(K, 7, 11), (K, 7, 12), (K, 7, 11), (60, 9, K), (60, 9, K), (61, 9, K)], (K, 7, 12)),
        ([(K, 1, 5), (30, 4, K)], (K, 1, K)),
    ]
    return _batch(slots, K, nr, epochs, seed=5)


@pytest.mark.parametrize("model,width", [("ComplEx", 48), ("DistMult", 24)])
@pytest.mark.parametrize("reg", ["N3", "N2"])
def test_crafted_batch_edges(model, width, reg):
    g = _graph(300)
    dim = width // 2 if model == "ComplEx" else width
    w = synth.make_weights(model, g.num_entities, g.num_relations, dim, seed=5, trained_scale=0.3)
    E, R = w["entity_embeddings"], w["relation_embeddings"]
    ctx = _lib.Context(model, E, R)
    K, nr, epochs = g.num_entities, g.num_relations, 3
    b = _crafted(K, nr, epochs)
    x0 = (np.random.default_rng(5).random((4, width)) * 0.2).astype(np.float32)
    sizes = [6, 12, 4]  # the slots' rows
    # R = batch_size and R = batch_size + 1 (a last step of one row) for every slot with rows
    for bs in (3, 4, 5, 6, 11, 12, 13):
        hp = _hp(dict(HP, epochs=epochs, batch_size=bs, regularizer_name=reg))
        s, r, x, loss = _run(ctx, hp, x0, b, want_x=True, trace=True)
        steps = _lib.trace_steps(model, hp, b["row_off"], b["rows"]).tolist()
        assert steps == [epochs * -(-sizes[0] // bs), 0, epochs * -(-sizes[1] // bs), epochs * -(-sizes[2] // bs)]
        assert [len(v) for v in loss] == steps
        assert np.array_equal(x[1], x0[1]), "a slot without rows must only be ranked"
        for i in (0, 2, 3):
            assert np.isfinite(loss[i]).all(), (bs, i, loss[i])
            rows = b["rows"][b["row_off"][i]:b["row_off"][i + 1]]
            # the first step needs only x0: the whole slot, or the first slice of its permutation
            first = rows if len(rows) <= bs else rows[b["perms"][i][0][:bs]]
            want = tr.step_loss(model, E, R, x0[i], first, reg, hp.reg_weight)
            assert tc.within(float(loss[i][0]), want), (bs, i, float(loss[i][0]), want)
    assert any(n % bs == 1 for n in sizes for bs in (3, 5, 11))
    ctx.close()


def test_transe_crafted_batch_edges():
    g = _graph(300)
    w = synth.make_weights("TransE", g.num_entities, g.num_relations, 16, seed=5)
    E, R = w["entity_embeddings"], w["relation_embeddings"]
    K, nr, epochs = g.num_entities, g.num_relations, 3
    slots = [([(K, 3, K), (K, 3, 17), (40, 5, K)], (K, 3, 17)), ([], (K, 2, 9)),
             ([(K, 7, 11), (K, 7, 12), (K, 7, 11), (60, 9, K), (60, 9, K), (61, 9, K)], (K, 7, 12)),
             ([(K, 1, 5), (30, 4, K)], (K, 1, K))]
    b = _batch(slots, K, nr, epochs, seed=5, transe=True)
    # negatives that are the kelpie entity, in the head and in the tail
    for pm in b["perms"][0] + b["perms"][2]:
        R_ = len(pm) // 3
        pm[R_:R_ + 2] = K
    b["rng"] = np.concatenate([np.concatenate(pm) for pm in b["perms"] if len(pm[0])]).astype(np.int32)
    x0 = (np.random.default_rng(5).standard_normal((4, 16)) * 0.3).astype(np.float32)
    sizes = [6, 12, 4]
    for norm in (2, 1):
        ctx = _lib.Context("TransE", E, R, norm_p=norm)
        for bs, ratio in ((3, 5), (5, 5), (6, 2), (11, 5), (12, 7), (13, 1)):
            hpd = dict(TE_HP, epochs=epochs, batch_size=bs, negative_triples_ratio=ratio)
            hp = _te_hp(hpd)
            s, r, x, loss = _run(ctx, hp, x0, b, want_x=True, trace=True)
            steps = _lib.trace_steps("TransE", hp, b["row_off"], b["rows"]).tolist()
            assert steps == [epochs * -(-sizes[0] // bs), 0, epochs * -(-sizes[1] // bs), epochs * -(-sizes[2] // bs)]
            assert [len(v) for v in loss] == steps and np.array_equal(x[1], x0[1])
            for i in (0, 2, 3):
                assert np.isfinite(loss[i]).all(), (bs, i, loss[i])
                rows = b["rows"][b["row_off"][i]:b["row_off"][i + 1]]
                pos, neg = tr.transe_batches(rows, b["perms"][i][0], ratio, bs, 0)
                want = tr.transe_step_loss(E, R, x0[i], pos, neg, norm, hpd["margin"], hpd["regularizer_weight"])
                assert tc.within(float(loss[i][0]), want), (norm, bs, ratio, i, float(loss[i][0]), want)
        ctx.close()


@pytest.mark.parametrize("rates", [(0.0, 0.0, 0.0), (0.0, 0.0, 0.2), (0.2, 0.3, 0.1)], ids=["plain", "hidden", "all"])
def test_conve_crafted_batch_edges(rates):
    """P = batch_size and P = batch_size + 1 (a last step of one pair) for every slot with rows,
    without dropouts, with the hidden one (the frozen-head pairs' FC rows are encoded once per
    batch) and with all three (they are encoded every step)."""
    g = _graph(300)
    w = synth.make_weights("ConvE", g.num_entities, g.num_relations, 60, seed=5)
    cv = _conve_model(g, w, rates)
    ctx = cv.ctx
    K, nr, epochs = g.num_entities, g.num_relations, 3
    b0 = _crafted(K, nr, 0)
    x0 = np.random.default_rng(5).random((4, 60)).astype(np.float32)
    pairs = [tr.slot_steps("ConvE", 1, 1, b0["rows"][b0["row_off"][i]:b0["row_off"][i + 1]]) for i in range(4)]
    assert pairs == [5, 0, 6, 4]
    for bs in (3, 4, 5, 6):
        hpd = dict(CV_HP, epochs=epochs, batch_size=bs)
        hp = cv.kp_hp(hpd)
        b, first = _conve_bits(cv, b0, hpd, seed=bs)
        s, r, x, loss = _run(ctx, hp, x0, b, want_x=True, trace=True)
        steps = _lib.trace_steps("ConvE", hp, b["row_off"], b["rows"]).tolist()
        assert steps == [epochs * -(-p // bs) for p in pairs] and [len(v) for v in loss] == steps
        assert np.array_equal(x[1], x0[1]), "a slot without rows must only be ranked"
        for i in (0, 2, 3):
            assert np.isfinite(loss[i]).all(), (bs, i, loss[i])
            er = {}
            for h, rel, t in b["rows"][b["row_off"][i]:b["row_off"][i + 1]].tolist():
                er.setdefault((h, rel), []).append(t)
            want = tr.conve_step_loss(w, x0[i], list(er)[:bs], er, first[i], hpd["label_smoothing"])
            assert tc.within(float(loss[i][0]), want), (rates, bs, i, float(loss[i][0]), want)
    assert any(p % bs == 1 for p in pairs for bs in (3, 4, 5)) and any(p == bs for p in pairs for bs in (4, 5, 6))


def test_conve_row_chunks_give_the_same_bits(monkeypatch):
    """The rows of a step run in chunks of logits; forced to 2 and to 1 rows per chunk the trace
    is bitwise the one of a single chunk."""
    w, b, x0, _ = _multi_slot_case("ConvE", 60)
    cv = _conve_model(_graph(300), w, (0.2, 0.3, 0.1))
    hpd = dict(CV_HP, batch_size=7, epochs=2)
    b, _ = _conve_bits(cv, b, hpd, seed=4)
    runs = []
    for chunk in (None, "2", "1"):
        if chunk:
            monkeypatch.setenv("KP_TRACE_CHUNK", chunk)
        runs.append(np.concatenate(_run(cv.ctx, cv.kp_hp(hpd), x0, b, trace=True)[-1]))
    assert len(runs[0]) > 6 and runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()


# --------------------------------------------------------------------------- 5. errors
def test_errors_are_refused_and_the_context_lives_on():
    w, b, x0, _ = _multi_slot_case("ComplEx", 16)
    ctx = _lib.Context("ComplEx", w["entity_embeddings"], w["relation_embeddings"])
    hp = _hp(dict(HP, batch_size=7))
    n = len(b["row_off"]) - 1
    pred, filt = np.ascontiguousarray(b["pred"]), np.ascontiguousarray(b["filt"])
    out_s, out_r = np.zeros(n, np.float32), np.zeros(n, np.int64)
    batch = _lib.Batch(n, _lib._ptr(x0), _lib._ptr(b["row_off"]), _lib._ptr(b["rows"]), _lib._ptr(b["rng_off"]),
                       _lib._ptr(b["rng"]), _lib._ptr(pred), _lib._ptr(b["filt_off"]), _lib._ptr(filt), None,
                       _lib._ptr(out_s), _lib._ptr(out_r))
    steps = _lib.trace_steps("ComplEx", hp, b["row_off"], b["rows"])
    good = np.zeros(n + 1, np.int32)
    np.cumsum(steps, out=good[1:])
    loss = np.zeros(int(good[-1]), np.float32)
    L = _lib.lib()

    def call(t_off, out_loss):
        t = _lib.Trace(_lib._ptr(t_off), _lib._ptr(out_loss))
        rc = L.kp_posttrain_rank_trace(ctx.h, C.byref(hp), C.byref(batch), 0, None, None, None, C.byref(t))
        return rc, L.kp_last_error(ctx.h).decode()

    wrong = good.copy()
    wrong[2] += 1
    assert call(wrong, loss) == (-22, "ComplEx: trace: trace_off disagrees with kp_trace_steps")
    shifted = good + 1
    assert call(shifted.astype(np.int32), loss) == (-22, "ComplEx: trace: trace_off must start at 0")
    assert call(good, None) == (-22, "ComplEx: trace: missing out_loss")
    assert not loss.any() and not out_s.any()  # refused before any device work
    rc, msg = call(good, loss)
    assert rc == 0, msg
    again = _run(ctx, hp, x0, b, trace=True)
    assert np.concatenate(again[-1]).tobytes() == loss.tobytes() and np.isfinite(loss).all()
    assert again[0].tobytes() == out_s.tobytes() and again[1].tobytes() == out_r.tobytes()
    ctx.close()
