"""Epoch marks on the device (kp_posttrain_rank_marks) against the stand-in and themselves.

1. every case of marks_cases.py against the stand-in's answer by the definition (the oracle
   on the same batch with ``hp.epochs = e``): every mark's score within 1e-4 * max(1, |ref|),
   its rank inside the rank rule's bounds, its row within 1e-4 of the row's largest magnitude
   (ComplEx, DistMult; the oracle's ConvE and TransE steps have no fp64 variant to derive a
   row bound from: printed, as test_gpu_widths.py does);
2. nothing else moves: with marks, out_x, out_score, out_rank, the lists at k = 5, the probes'
   results and the trace are bitwise those without;
3. the ends: mark hp.epochs is the slot's own result, mark 0 a call with hp.epochs = 0, an
   empty slot x0's result at every mark;
4. the definition, bitwise where it must hold: every mark against the same batch run with
   hp.epochs = e (TransE always; the other families on equal steps per epoch), a mixed batch
   at the score tolerance and the rank rule;
5. KP_MARKS_CHUNK=16 with five marks: bitwise the unchunked call;
6. a fresh context gives the same marks bitwise;
7. malformed marks are host errors raised before any device work, and a call that breaks two
   rules at once reports the one checked first (batch, top-k, probes, trace, marks);
8. both sets of rank rows chunked at once (KP_PROBE_CHUNK=16 and KP_MARKS_CHUNK=16, each set
   with a partial last chunk), with the lists and the trace: bitwise the unchunked call;
9. every post-training of the reference fixture: score, rank and, in every family, the rows
   against the reference's fp64 run.

Run on an MI355X: ``python -m pytest tests -m gpu``.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import marks_cases as mc
import width_cases as wc
from kelpie_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from extras_digest import probes_of  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILY = [c for c in mc.CASES if c["id"] in ("ComplEx-d32-DB4", "DistMult-d40-DB4", "ConvE-d60-DB4",
                                              "TransE-d16-VPL1-NT1024")]
assert len(FAMILY) == 4


@functools.lru_cache(maxsize=None)
def _device(case_id):
    """One device run of a case through the engine: its captured batches and its model."""
    case = next(c for c in mc.CASES + mc.MIXED if c["id"] == case_id)
    return mc.run(case, lambda m: m.ctx)


def _call(model, batch, epochs=None, fresh=False, **kw):
    """The captured batch again, directly: with ``epochs`` as hp.epochs, on a fresh context."""
    hp = batch["args"][0] if epochs is None else mc.hp_with_epochs(batch["args"][0], epochs)
    ctx = model._make_ctx() if fresh else model.ctx._ctx  # (model.ctx is marks_cases.Capture around the device's)
    return ctx.posttrain_rank(hp, *batch["args"][1:], want_x=True, **kw)


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ----------------------------------------------------------------------------- 1. the stand-in
@pytest.mark.parametrize("case", mc.CASES + mc.MIXED, ids=mc.ids(mc.CASES + mc.MIXED))
def test_marks_vs_standin(case):
    batches, model = _device(case["id"])
    ref, spe = mc.reference(case)
    got = mc.device_marks(batches)
    assert len(got) == len(ref) > 0
    if case.get("mixed"):
        assert sorted(spe[0]) == [1, 2, 3], spe
    rows = case["model"] in ("ComplEx", "DistMult")
    exact = n = 0
    worst = 0.0
    for gb, rb in zip(got, ref):
        assert len(gb) == len(rb)
        for gs, rs in zip(gb, rb):  # a slot's marks as so many slots of check_slots
            e, w = wc.check_slots(gs, rs, rows=rows)
            exact, n, worst = exact + e, n + len(gs), max(worst, w)
    print(f"{case['id']}: marks {n}, exact ranks {exact}, row error {worst:.2e} of the row's scale; "
          f"ranks {[[m['rank'] for m in s] for b in got for s in b]}")
    # the marks move on the device as well: a feature that returned the final result everywhere fails
    assert any(len({m["rank"] for m in s}) > 1 for b in got for s in b)


# ----------------------------------------------------------------------------- 2. nothing else moves
def _own_probes(batch):
    """One probe per slot: the slot's own (p, o) with its own filter."""
    _, _, row_off, _, _, _, pred, filt_off, filt = batch["args"]
    n = len(row_off) - 1
    return (np.arange(n + 1, dtype=np.int32), np.asarray(pred)[:, 1:3].astype(np.int32),
            np.asarray(filt_off, np.int32), np.asarray(filt, np.int32))


@pytest.mark.parametrize("case", FAMILY, ids=mc.ids(FAMILY))
def test_nothing_else_moves(case):
    batches, model = _device(case["id"])
    b = batches[0]
    marks = mc.marks_of(case)
    kw = {"topk": 5, "probes": _own_probes(b), "trace": True}
    plain = _call(model, b, **kw)
    marked = _call(model, b, marks=marks, **kw)
    assert len(marked) == len(plain) + 1
    s, r, x, (ids, top), (ps, pr), losses = plain
    s2, r2, x2, (ids2, top2), (ps2, pr2), losses2 = marked[:-1]
    for a, c in ((s, s2), (r, r2), (x, x2), (ids, ids2), (top, top2), (ps, ps2), (pr, pr2)):
        assert _same(a, c)
    assert len(losses) == len(losses2) and all(_same(a, c) for a, c in zip(losses, losses2))
    assert sum(len(v) for v in losses) > 0 and (ids >= 0).any()
    # and the other requests move neither the slots nor the marks
    bare = _call(model, b, marks=marks)
    assert all(_same(a, c) for a, c in zip(bare[:3], plain[:3]))
    assert all(_same(a, c) for a, c in zip(bare[-1], marked[-1]))
    assert all(_same(a, c) for a, c in zip(bare[-1], b["out"][-1]))  # as the engine's call returned them


# ----------------------------------------------------------------------------- 3. the ends
def _with_empty_slot(batch):
    """The batch with a slot without rows (and without draws) after its first slot: that slot's
    x0, target and filter are the first slot's."""
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = batch["args"]
    f0 = np.asarray(filt[filt_off[0]:filt_off[1]])
    return (hp, np.insert(x0, 1, x0[0], axis=0), np.insert(row_off, 1, row_off[1]), rows,
            np.insert(rng_off, 1, rng_off[1]), rng, np.insert(pred, 1, pred[0], axis=0),
            np.concatenate([filt_off[:2], filt_off[1:] + len(f0)]),
            np.concatenate([filt[:filt_off[1]], f0, filt[filt_off[1]:]]))


@pytest.mark.parametrize("case", FAMILY, ids=mc.ids(FAMILY))
def test_the_ends(case):
    batches, model = _device(case["id"])
    b = {"args": _with_empty_slot(batches[0])}
    E = int(b["args"][0].epochs)
    marks = [0, 2, E]
    s, r, x, (ms, mr, mx) = _call(model, b, marks=marks)
    # mark hp.epochs is the slot's own result
    assert _same(ms[:, -1], s) and _same(mx[:, -1], x) and mr[:, -1].tolist() == r.tolist()
    # mark 0 is a call with hp.epochs = 0
    s0, r0, x0 = _call(model, b, epochs=0)
    assert _same(ms[:, 0], s0) and _same(mx[:, 0], x0) and mr[:, 0].tolist() == r0.tolist()
    assert _same(x0, np.asarray(b["args"][1], np.float32))
    # the empty slot has x0's result at every mark, and is the first slot's mark 0 (the same
    # x0, target and filter)
    for j in range(len(marks)):
        assert _same(ms[1, j], s0[1]) and _same(mx[1, j], x0[1]) and mr[1, j] == r0[1]
    assert _same(ms[1, 0], ms[0, 0]) and mr[1, 0] == mr[0, 0]
    assert not _same(mx[0, 1], mx[0, 0]) and not _same(mx[0, 1], mx[0, 2])  # a slot with rows moves


# ----------------------------------------------------------------------------- 4. the definition
@pytest.mark.parametrize("case", mc.CASES, ids=mc.ids(mc.CASES))
def test_definition_bitwise_equal_steps(case):
    """One step per epoch in every slot: the first e epochs of the call are the launches of the
    call with hp.epochs = e on the same inputs (TransE: one workgroup per slot, whatever the rest)."""
    batches, model = _device(case["id"])
    _, spe = mc.reference(case)
    for b, steps in zip(batches, spe):
        assert len(set(steps)) == 1, steps
        ms, mr, mx = b["out"][-1]
        for j, e in enumerate(mc.marks_of(case)):
            s, r, x = _call(model, b, epochs=e)
            assert _same(ms[:, j], s) and _same(mx[:, j], x) and mr[:, j].tolist() == r.tolist(), (case["id"], e)


@pytest.mark.parametrize("case", mc.MIXED, ids=mc.ids(mc.MIXED))
def test_definition_mixed_steps(case):
    """Slots of 1, 2 and 3 steps per epoch in one batch: TransE bitwise; the other families at
    the score tolerance and the rank rule (slots that finish early change the attention's
    key-range plan, and with it the last bit)."""
    batches, model = _device(case["id"])
    ref, spe = mc.reference(case)
    b = batches[0]
    assert sorted(spe[0]) == [1, 2, 3], spe
    ms, mr, mx = b["out"][-1]
    for j, e in enumerate(mc.marks_of(case)):
        s, r, x = _call(model, b, epochs=e)
        if case["model"] == "TransE":
            assert _same(ms[:, j], s) and _same(mx[:, j], x) and mr[:, j].tolist() == r.tolist(), e
            continue
        for i in range(len(s)):
            m = ref[0][i][j]
            assert abs(float(ms[i, j]) - float(s[i])) <= wc.TOL * max(1.0, abs(float(s[i]))), (e, i)
            assert m["lo"] <= int(mr[i, j]) <= m["hi"] and m["lo"] <= int(r[i]) <= m["hi"], (e, i, mr[i, j], r[i], m)


# ----------------------------------------------------------------------------- 5. chunks, 6. rerun
def _twice(args):
    """The batch twice over: its slots, then the same slots again."""
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = args
    return (hp, np.vstack([x0, x0]), np.concatenate([row_off, row_off[1:] + row_off[-1]]), np.vstack([rows, rows]),
            np.concatenate([rng_off, rng_off[1:] + rng_off[-1]]), np.concatenate([rng[:rng_off[-1]]] * 2),
            np.vstack([pred, pred]), np.concatenate([filt_off, filt_off[1:] + filt_off[-1]]),
            np.concatenate([filt[:filt_off[-1]]] * 2))


@pytest.mark.parametrize("case", FAMILY, ids=mc.ids(FAMILY))
def test_chunks_and_rerun(case, monkeypatch):
    batches, model = _device(case["id"])
    b = batches[0]
    marks = [0, 1, 2, 5, 8]  # five marks a slot: its rows straddle chunks of 16
    whole = _call(model, b, marks=marks)
    monkeypatch.setenv("KP_MARKS_CHUNK", "16")
    assert len(b["args"][2]) - 1 == 3 and 3 * len(marks) < 16
    # 15 rows fit one chunk of 16: the batch twice over makes 30 rows, slot 3's marks straddle
    twice = _twice(b["args"])
    chunked = _call(model, {"args": twice}, marks=marks)
    monkeypatch.delenv("KP_MARKS_CHUNK")
    unchunked = _call(model, {"args": twice}, marks=marks)
    for a, c in zip(chunked[:3] + chunked[-1], unchunked[:3] + unchunked[-1]):
        assert _same(a, c)
    if case["model"] == "TransE":  # one workgroup per slot: the doubled batch repeats the single one
        for a, c in zip(unchunked[-1], whole[-1]):
            assert _same(a[:3], c) and _same(a[3:], c)
    # a fresh context gives bitwise the same marks
    again = _call(model, b, marks=marks, fresh=True)
    for a, c in zip(again[:3] + again[-1], whole[:3] + whole[-1]):
        assert _same(a, c)


# ----------------------------------------------------------------------------- 7. errors
def _raw(ctx, args, epochs, nulls=(), n_override=None):
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = args
    n = len(row_off) - 1
    keep = [np.ascontiguousarray(x0, np.float32), np.ascontiguousarray(row_off, np.int32),
            np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(rng_off, np.int64),
            np.ascontiguousarray(rng, np.int32), np.ascontiguousarray(pred, np.int32),
            np.ascontiguousarray(filt_off, np.int32), np.ascontiguousarray(filt, np.int32),
            np.zeros(n, np.float32), np.zeros(n, np.int64)]
    p = [_lib._ptr(a) for a in keep]
    b = _lib.Batch(n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], None, p[8], p[9])
    ep = np.ascontiguousarray(epochs, np.int32)
    nm = max(1, len(ep))
    out = {"epochs": ep if len(ep) else np.zeros(1, np.int32), "out_score": np.zeros((n, nm), np.float32),
           "out_rank": np.zeros((n, nm), np.int64)}
    mk = _lib.Marks(len(ep) if n_override is None else n_override,
                    *[None if k in nulls else _lib._ptr(a) for k, a in out.items()], None)
    rc = _lib.lib().kp_posttrain_rank_marks(ctx.h, C.byref(hp), C.byref(b), 0, None, None, None, None, C.byref(mk))
    return rc, _lib.lib().kp_last_error(ctx.h).decode()


@pytest.mark.parametrize("case", FAMILY, ids=mc.ids(FAMILY))
def test_errors_are_host_errors(case, monkeypatch):
    batches, model = _device(case["id"])
    args = batches[0]["args"]
    E = int(args[0].epochs)
    ctx = model.ctx._ctx
    for epochs, kw, msg in (([], {}, "n must be in [1, 16]"),
                            (list(range(16)) + [16], {}, "n must be in [1, 16]"),
                            ([0, 2, 2], {}, "epochs must be strictly increasing"),
                            ([0, E + 1], {}, "epoch beyond hp->epochs"),
                            ([-1, 2], {}, "negative epoch"),
                            ([0, 2], {"nulls": ("out_rank",)}, "missing mark output"),
                            ([0, 2], {"nulls": ("epochs",)}, "missing epochs")):
        rc, err = _raw(ctx, args, epochs, **kw)
        assert rc == -22 and err.endswith("marks: " + msg), (epochs, rc, err)
    rc, _ = _raw(ctx, args, [0, 2])
    assert rc == 0  # the context stays usable
    with pytest.raises(_lib.KelpieHipError, match="marks"):
        ctx.posttrain_rank(*args, marks=[0, E + 1])
    # the fp32 diagnostic ranks have no fp64 operands to rank the marks on
    if case["model"] in ("ConvE", "TransE"):
        monkeypatch.setenv("KP_CV_RANK" if case["model"] == "ConvE" else "KP_TE_RANK", "f32")
        f32 = wc.make_model(case).ctx
        rc, err = _raw(f32, args, [0, 2])
        assert rc == -95 and "marks need the fp64 rank" in err, (rc, err)
        rc, err = _raw(f32, args, [0, 2, 2])
        assert rc == -22, (rc, err)  # malformed first


def _two_faults(ctx, args, faults, empty=False):
    """kp_posttrain_rank_marks on the batch (``empty``: with n_slots = 0) with the requests named
    in ``faults`` malformed and the others absent: "k" = 33, "probes" whose probe_off starts at 1,
    "trace" without trace_off, "marks" with n = 0; "hp": batch_size = 0."""
    hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = args
    n = len(row_off) - 1
    hp = type(hp).from_buffer_copy(hp)
    if "hp" in faults:
        hp.batch_size = 0
    keep = [np.ascontiguousarray(x0, np.float32), np.ascontiguousarray(row_off, np.int32),
            np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(rng_off, np.int64),
            np.ascontiguousarray(rng, np.int32), np.ascontiguousarray(pred, np.int32),
            np.ascontiguousarray(filt_off, np.int32), np.ascontiguousarray(filt, np.int32),
            np.zeros(n, np.float32), np.zeros(n, np.int64), np.ones(n + 1, np.int32), np.zeros(2, np.int32),
            np.zeros(1, np.float32), np.zeros(1, np.int64), np.zeros((n, 33), np.int32), np.zeros((n, 33), np.float32)]
    p = [_lib._ptr(a) for a in keep]
    b = _lib.Batch(0 if empty else n, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], None, p[8], p[9])
    pr = _lib.Probes(1, p[10], p[11], p[11], p[11], p[12], p[13]) if "probes" in faults else None
    tr = _lib.Trace(None, None) if "trace" in faults else None
    mk = _lib.Marks(0, p[11], p[12], p[13], None) if "marks" in faults else None
    ref = lambda st: C.byref(st) if st is not None else None  # noqa: E731
    k = 33 if "k" in faults else 0
    rc = _lib.lib().kp_posttrain_rank_marks(ctx.h, C.byref(hp), C.byref(b), k, p[14] if k else None,
                                            p[15] if k else None, ref(pr), ref(tr), ref(mk))
    return rc, _lib.lib().kp_last_error(ctx.h).decode()


# what the library answered to each pair of faults before the request checks were joined into
# one function (profiles/extras_refactor/two_faults_parent.txt): (faults, n_slots = 0) ->
# message, "{m}" the family's name
TWO_FAULTS = {
    (("k", "probes"), False): "{m}: top-k: k must be in [0, 32]",
    (("k", "probes"), True): "kp_posttrain_rank_topk: k must be in [0, 32]",
    (("probes", "trace"), False): "{m}: probes: probe_off must start at 0",
    (("probes", "trace"), True): "kp_posttrain_rank_probes: probes without a slot",
    (("trace", "marks"), False): "{m}: trace: missing trace_off",
    (("trace", "marks"), True): "{m}: trace: missing trace_off",
    # without a slot no family runs, and none refuses its hyper-parameters
    (("probes", "hp"), True): "kp_posttrain_rank_probes: probes without a slot",
    (("hp", "trace"), True): "{m}: trace: batch_size must be positive",
    (("hp", "marks"), True): "{m}: marks: n must be in [1, 16]",
    (("k", "hp"), True): "kp_posttrain_rank_topk: k must be in [0, 32]",
}
# ComplEx / DistMult refuse batch_size = 0 before the request, ConvE between the probes and the
# trace, TransE after the request (where the trace's own rule has already refused it)
_CX_HP = "{m}: bad batch_size/epochs"
HP_FAULTS = {
    (("probes", "hp"), False): {"ComplEx": _CX_HP, "DistMult": _CX_HP, "ConvE": "{m}: probes: probe_off must start at 0",
                                "TransE": "{m}: probes: probe_off must start at 0"},
    (("hp", "trace"), False): {"ComplEx": _CX_HP, "DistMult": _CX_HP, "ConvE": "{m}: bad hyper-parameters",
                               "TransE": "{m}: trace: batch_size must be positive"},
    (("hp", "marks"), False): {"ComplEx": _CX_HP, "DistMult": _CX_HP, "ConvE": "{m}: bad hyper-parameters",
                               "TransE": "{m}: marks: n must be in [1, 16]"},
    (("k", "hp"), False): {"ComplEx": _CX_HP, "DistMult": _CX_HP, "ConvE": "{m}: top-k: k must be in [0, 32]",
                           "TransE": "{m}: top-k: k must be in [0, 32]"},
}


@pytest.mark.parametrize("case", FAMILY, ids=mc.ids(FAMILY))
def test_two_faults_report_the_first(case):
    """A call that breaks two rules reports the one checked first: batch, top-k, probes, trace,
    marks, with each family's hyper-parameter check at its own place among them."""
    batches, model = _device(case["id"])
    args = batches[0]["args"]
    ctx = model.ctx._ctx
    m = case["model"]
    table = dict(TWO_FAULTS)
    table.update({key: msgs[m] for key, msgs in HP_FAULTS.items()})
    for (faults, empty), msg in table.items():
        rc, err = _two_faults(ctx, args, faults, empty)
        assert rc == -22 and err == msg.format(m=m), (faults, empty, rc, err)
    rc, _ = _raw(ctx, args, [0, 2])
    assert rc == 0  # the context stays usable


# ----------------------------------------------------------------------------- 8. both row sets chunked
@pytest.mark.parametrize("case", FAMILY, ids=mc.ids(FAMILY))
def test_both_row_sets_chunked(case, monkeypatch):
    """Six slots, three probes and five marks each: 18 probe rows and 30 mark rows, each more
    than one chunk of 16 and no multiple of it, the smallest shape at which the two sets, each
    with a partial last chunk, could disturb one another."""
    batches, model = _device(case["id"])
    args = _twice(batches[0]["args"])
    n = len(args[2]) - 1
    marks = [0, 1, 2, 5, 8]
    probes = probes_of(args, model.ctx.n_ent, per_slot=3)
    for rows in (len(probes[1]), n * len(marks)):
        assert rows > 16 and rows % 16 != 0
    kw = {"topk": 5, "probes": probes, "trace": True, "marks": marks}
    whole = _call(model, {"args": args}, **kw)
    monkeypatch.setenv("KP_PROBE_CHUNK", "16")
    monkeypatch.setenv("KP_MARKS_CHUNK", "16")
    chunked = _call(model, {"args": args}, **kw)
    s, r, x, lists, probed, losses, marked = whole
    s2, r2, x2, lists2, probed2, losses2, marked2 = chunked
    for a, c in zip((s, r, x) + lists + probed + marked, (s2, r2, x2) + lists2 + probed2 + marked2):
        assert _same(a, c)
    assert len(losses) == len(losses2) == n and all(_same(a, c) for a, c in zip(losses, losses2))
    assert sum(len(v) for v in losses) > 0 and (lists[0] >= 0).any() and len(probed[0]) == 18


# ----------------------------------------------------------------------------- the reference fixture
def _fixture():
    import marks_golden as mg
    return mg.posttrainings()


@pytest.mark.parametrize("pid,case,pt", _fixture(), ids=lambda v: v if isinstance(v, str) else "")
def test_marks_vs_reference(pid, case, pt):
    """Every recorded post-training: the device's marks against the values the reference gave
    inside one run of its own optimizer (tests/golden/marks_golden.json)."""
    import marks_golden as mg
    model = mg.make_model(case)
    s, r, x, (ms, mr, mx) = model.ctx.posttrain_rank(*mg.batch(model, case, pt), want_x=True, marks=mg.golden()["marks"])
    print(f"{pid}: row error {mg.row_error(pt, mx[0]):.2e} of the fp64 row's scale (every family's rows are held)")
    exact = mg.check(pid, pt, ms[0], mr[0], mx[0])
    print(f"{pid}: ranks {mr[0].tolist()}, {exact} of {len(pt['marks'])} equal the reference's fp64 rank")
    assert _same(ms[0, -1], s[0]) and _same(mx[0, -1], x[0]) and int(mr[0, -1]) == int(r[0])
