"""The post-training trace, CPU tier: the reference fixture and the fp64 restatement of the
definition (trace_reference.py), kp_trace_steps, and the host layers -- ``compute_traces``,
the engine's ``trace``, the builder / pipeline ``trace`` -- over the oracle-backed stand-in
contexts wrapped to serve traces (trace_backend.py).  The device side is test_trace_gpu.py.
"""
import inspect
import random

import numpy as np
import pytest
import torch

import kelpie_amd as ka
import trace_cases as tc
import trace_reference as tr
from engine_cases import build_product
from golden_io import seed_all
from kelpie_amd import _lib
from kelpie_amd.pipeline import build_pipeline, run_explain
from trace_backend import code, wrap


def _state():
    return (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
            random.getstate())


# ----------------------------------------------------------------------------- the reference fixture
def test_fixture_fp32_and_fp64_agree():
    """The generator's condition, asserted again on the file."""
    n = 0
    for _, case, pt in tc.posttrainings():
        R, bs = pt.get("pairs", len(pt["rows"])), pt["hp"]["batch_size"]  # ConvE steps over its pairs
        per_epoch = (R + bs - 1) // bs
        assert per_epoch >= 3 and R % bs != 0 and pt["hp"]["epochs"] <= 8  # a shorter last step
        assert len(pt["steps"]) == pt["hp"]["epochs"] * per_epoch
        for s in pt["steps"]:
            assert tc.within(s["l32"], s["l64"]), (case["name"], pt["kind"], s["l32"], s["l64"])
            n += 1
    assert n >= 100 and len(tc.posttrainings()) == 16
    conve = tc.posttrainings(("ConvE",))
    assert [c["weights"]["dim"] for _, c, _ in conve] == [60, 60, 200]
    assert [all(r > 0 for r in p["rates"]) for _, _, p in conve] == [False, True, False]
    for _, _, p in conve:  # ls 0.1, a last batch of one pair, no logit near the clamp
        assert p["hp"]["label_smoothing"] == 0.1 and p["pairs"] % p["hp"]["batch_size"] == 1
        assert p["max_logit"] < 16 / 1.25
    names = {c["name"] for c in tc.golden()["cases"]}
    assert {"complex8_adagrad", "complex8_n3", "complex8_n2", "complex8_adam", "distmult8_n3", "complex200_n3",
            "transe16_l2", "transe16_l1", "transe200_l2", "conve60", "conve60_drop", "conve200"} <= names
    for family in ("ComplEx", "TransE"):  # each family's three row sets: base, necessary, sufficient
        assert {p["kind"] for _, c, p in tc.posttrainings() if c["model"] == family} == {"base", "necessary", "sufficient"}
    # every start row is reproduced from the case's seed: the first recorded row is it
    for _, case, pt in tc.posttrainings():
        if pt["steps"][0]["row"] is not None:
            assert np.array_equal(np.asarray(pt["steps"][0]["row"])[:tc.width(case)], tc.x0(case).astype(np.float64))


def _recorded(case, pt):
    """(step, restatement, l64) of every step recorded with its row."""
    model = case["model"]
    E, R = tc.tables(case["name"])[1:] if model != "ConvE" else (None, None)
    hp = pt["hp"]
    for j, s in enumerate(pt["steps"]):
        if s["row"] is None:
            continue
        batch = tc.step_batch(case, pt, j)
        if model == "ConvE":
            got, logits = tr.conve_step_loss(tc.conve_weights(case["name"]), s["row"], batch[0], batch[1],
                                             tc.conve_masks(case, pt, j), hp["label_smoothing"], with_logits=True)
            assert np.abs(logits).max() < 16 / 1.25  # the bound the width cases keep: no clamped log
        elif model == "TransE":
            got = tr.transe_step_loss(E, R, s["row"], batch[0], batch[1], case["weights"]["norm"], hp["margin"],
                                      hp["regularizer_weight"])
        else:
            got = tr.step_loss(model, E, R, s["row"], batch, hp["regularizer_name"], hp["regularizer_weight"])
        yield j, got, s["l64"]


@pytest.mark.parametrize("pid,case,pt", [p for p in tc.posttrainings() if p[2]["steps"][0]["row"] is not None],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_restatement_equals_reference_fp64(pid, case, pt):
    """Both sides are fp64 and differ only in summation order: 1e-10 relative."""
    n = 0
    for j, got, l64 in _recorded(case, pt):
        assert abs(got - l64) <= 1e-10 * abs(l64), (pid, j, got, l64)
        n += 1
    assert n == len(pt["steps"])


def test_distmult_is_complex_on_zero_imaginary():
    """The zero-imaginary identity holds for the value."""
    case = next(c for c in tc.golden()["cases"] if c["model"] == "DistMult")
    _, E, R = tc.tables(case["name"])
    pad = lambda a: np.hstack([a, np.zeros_like(a)])  # noqa: E731
    for _, c, pt in tc.posttrainings():
        if c is not case:
            continue
        hp = pt["hp"]
        for j, s in enumerate(pt["steps"][:5]):
            row = np.asarray(s["row"])
            batch = tc.step_batch(case, pt, j)
            d = E.shape[1]
            assert np.all(row[d:] == 0)
            for reg in ("N3", "N2"):
                a = tr.step_loss("DistMult", E, R, row[:d], batch, reg, hp["regularizer_weight"])
                b = tr.step_loss("ComplEx", pad(E), pad(R), row, batch, reg, hp["regularizer_weight"])
                assert abs(a - b) <= 1e-12 * abs(b)


# ----------------------------------------------------------------------------- kp_trace_steps
def _hp(epochs, batch_size):
    hp = _lib.HP()
    hp.epochs, hp.batch_size = epochs, batch_size
    return hp


def test_trace_steps_equal_the_fixture():
    for pid, case, pt in tc.posttrainings():
        rows = np.asarray(pt["rows"], np.int32)
        hp = _hp(pt["hp"]["epochs"], pt["hp"]["batch_size"])
        # the recorded slot between an empty slot and a copy of itself
        off = np.array([0, 0, len(rows), len(rows), 2 * len(rows)], np.int32)
        got = _lib.trace_steps(case["model"], hp, off, np.vstack([rows, rows]))
        n = len(pt["steps"])
        assert got.tolist() == [0, n, 0, n], (pid, got)
        assert tr.slot_steps(case["model"], hp.epochs, hp.batch_size, rows) == n


def test_trace_steps_rule():
    K = 50
    rows = np.array([[K, 0, 1], [K, 0, 2], [K, 1, 1], [3, 2, K], [3, 2, K], [4, 2, K], [K, 0, K]], np.int32)
    off = np.array([0, 7, 7, 10], np.int32)
    both = np.vstack([rows, rows[:3]])
    for model in ("ComplEx", "DistMult", "TransE"):
        assert _lib.trace_steps(model, _hp(3, 2), off, both).tolist() == [12, 0, 6]
        assert _lib.trace_steps(model, _hp(3, 7), off, both).tolist() == [3, 0, 3]
        assert _lib.trace_steps(model, _hp(3, 6), off, both).tolist() == [6, 0, 3]
        assert _lib.trace_steps(model, _hp(0, 6), off, both).tolist() == [0, 0, 0]
    # ConvE: the distinct (head, relation) pairs: (K,0) (K,1) (3,2) (4,2) -> 4; then (K,0) (K,1) -> 2
    assert _lib.trace_steps("ConvE", _hp(3, 2), off, both).tolist() == [6, 0, 3]
    assert _lib.trace_steps("ConvE", _hp(3, 3), off, both).tolist() == [6, 0, 3]
    assert _lib.trace_steps("ConvE", _hp(5, 4), off, both).tolist() == [5, 0, 5]
    for model in ("ComplEx", "ConvE"):
        for bad_hp in (_hp(1, 0), _hp(-1, 4)):
            with pytest.raises(_lib.KelpieHipError, match="kp_trace_steps"):
                _lib.trace_steps(model, bad_hp, off, both)
        with pytest.raises(_lib.KelpieHipError, match="row_off"):
            _lib.trace_steps(model, _hp(1, 4), np.array([0, 7, 5, 10], np.int32), both)


def test_symbols_declared_and_bound():
    assert {"kp_trace_steps", "kp_posttrain_rank_trace"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.kp_posttrain_rank_trace(None, None, None, 0, None, None, None, None) != 0  # null context: refused
    assert inspect.signature(_lib.Context.posttrain_rank).parameters["trace"].default is False
    for f in (ka.StochasticBuilder.__init__, build_pipeline, run_explain):
        assert inspect.signature(f).parameters["trace"].default is False


# ----------------------------------------------------------------------------- host protocol
def _necessary(name, traced=True):
    rec, ds, model = build_product(name, "cpu")
    ctx = wrap(model) if traced else model._ctx
    block = rec["necessary"][0]
    pred = tuple(block["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in block["calls"]]
    return rec, ds, model, ctx, pred, rules


def _slot_of(ctx, side):
    """The traced slot whose result this side reports: found by its coded trace."""
    assert side["loss"], side
    v = side["loss"][0]
    slot = next(s for s in ctx.slots if s["loss"] and s["loss"][0] == v)
    assert side["loss"] == slot["loss"] and side["score"] == slot["score"] and side["rank"] == slot["rank"], (side, slot)
    assert slot["loss"] == [code(slot["call"], slot["slot"], j) for j in range(len(slot["loss"]))]
    return slot


@pytest.mark.parametrize("name", ["complex_tiny", "transe_tiny", "conve60_tiny"])
def test_traces_equal_relevance_batch(name):
    """Same relevances, same generator state afterwards, same batches; every slot's trace on
    its own rule and side, with the length of its own rows."""
    rec, ds, model, ctx, pred, rules = _necessary(name)
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    plain = eng.compute_relevance_batch(pred, rules)
    after_plain = _state()
    plain_results = [(dict(pt), dict(base)) for pt, base in eng.last_results]
    calls = list(ctx.calls)
    assert ctx.trace_calls and not any(ctx.trace_calls)
    assert all("loss" not in pt and "loss" not in base for pt, base in plain_results)

    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    n0 = len(ctx.trace_calls)
    out = eng.compute_traces(pred, rules)
    assert _state() == after_plain
    assert [o["relevance"] for o in out] == plain
    assert ctx.calls[len(calls):] == calls and all(ctx.trace_calls[n0:])
    assert eng.trace is False
    n_base = len(eng._get_kelpie_dataset(pred[0]).base_rows)
    seen = set()
    for o, rule, (ppt, pbase) in zip(out, rules, plain_results):
        assert set(o) == {"relevance", "base", "post"}
        for side, ref in ((o["base"], pbase), (o["post"], ppt)):
            assert set(side) == {"score", "rank", "loss"}
            assert side["score"] == ref["target_score"] and side["rank"] == ref["target_rank"]
        base, post = _slot_of(ctx, o["base"]), _slot_of(ctx, o["post"])
        # the base slot trains every row of the subject, the post slot the rule's triples fewer
        assert base["rows"] == n_base and post["rows"] == n_base - 2 * len(rule), (base, post, rule)
        assert (post["call"], post["slot"]) not in seen
        seen.add((post["call"], post["slot"]))
    assert len({(o["base"]["loss"][0]) for o in out}) == 1  # one base post-training serves every rule


@pytest.mark.parametrize("name", ["complex_tiny", "transe_tiny", "conve60_tiny"])
def test_sufficient_traces(name):
    rec, ds, model = build_product(name, "cpu")
    ctx = wrap(model)
    block = rec["sufficient"][0]
    pred = tuple(block["pred"])
    rules = [[tuple(t) for t in c["rule"]] for c in block["calls"]]

    def engine():
        seed_all(rec["seed"])
        eng = ka.SufficientPostTrainingEngine(model, ds, rec["hp"])
        eng.select_entities_to_convert(pred, block["k"], block["degree_cap"])
        return eng

    eng = engine()
    plain = eng.compute_relevance_batch(pred, rules)
    after = _state()
    eng = engine()
    out = eng.compute_traces(pred, rules)
    assert _state() == after and [o["relevance"] for o in out] == plain
    for o, rule in zip(out, rules):
        assert set(o) == {"relevance", "conversions"}
        assert [c["entity"] for c in o["conversions"]] == list(eng.entities_to_convert)
        for c in o["conversions"]:
            assert set(c) == {"entity", "base", "post"}
            base, post = _slot_of(ctx, c["base"]), _slot_of(ctx, c["post"])
            n_base = len(eng._get_kelpie_dataset(c["entity"]).base_rows)
            assert base["rows"] == n_base and post["rows"] == n_base + 2 * len(rule)
    # every conversion entity has a base of its own
    assert len({c["base"]["loss"][0] for c in out[0]["conversions"]}) == len(eng.entities_to_convert)


def test_trace_property_and_cached_base():
    rec, ds, model, ctx, pred, rules = _necessary("complex_tiny")
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    assert eng.trace is False
    eng.compute_relevance_batch(pred, rules[:1])  # caches the base result, without a trace
    slots_before = sum(ctx.calls)
    out = eng.compute_traces(pred, rules[1:])
    assert sum(ctx.calls) - slots_before == len(rules) - 1  # the post-trainings only: no base run again
    for o in out:
        assert o["base"]["loss"] is None and o["base"]["rank"] >= 1
        assert len(o["post"]["loss"]) > 0
    # under engine.trace every result has "loss": None on a base cached without one
    eng.trace = True
    eng.compute_relevance_batch(pred, rules[1:2])
    pt, base = eng.last_results[0]
    assert "loss" in base and base["loss"] is None and pt["loss"]
    eng.trace = False
    eng.set_cache()
    eng.trace = True
    eng.compute_relevance_batch(pred, rules[:1])
    pt, base = eng.last_results[0]
    assert pt["loss"] and base["loss"] and all(isinstance(v, float) for v in pt["loss"])
    for bad in (1, 0, "yes", None):
        with pytest.raises(TypeError):
            eng.trace = bad
    assert eng.trace is True


def test_no_trace_passes_no_new_keyword():
    rec, ds, model, ctx, pred, rules = _necessary("complex_tiny", traced=False)
    assert "trace" not in inspect.signature(ctx.posttrain_rank).parameters
    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    eng.compute_relevance_batch(pred, rules)
    eng.set_cache()
    with pytest.raises(TypeError, match="trace"):
        eng.compute_traces(pred, rules)


def test_sharding_refused_before_any_draw():
    rec, ds, model, ctx, pred, rules = _necessary("complex_tiny")

    class Sharding:
        world, rank = 2, 0

        def __getattr__(self, name):
            raise AssertionError(f"sharding used: {name}")

    seed_all(rec["seed"])
    eng = ka.NecessaryPostTrainingEngine(model, ds, rec["hp"])
    eng.sharding = Sharding()
    before = _state()
    with pytest.raises(NotImplementedError):
        eng.compute_traces(pred, rules)
    eng.trace = True
    with pytest.raises(NotImplementedError):
        eng.compute_relevance_batch(pred, rules)
    assert _state() == before and ctx.trace_calls == []


@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
def test_builder_record(mode):
    rec, ds, model = build_product("complex_tiny", "cpu")
    wrap(model)
    block = rec[mode][0]
    pred = tuple(block["pred"])
    cands = [tuple(c["rule"][0]) for c in block["calls"] if len(c["rule"]) == 1][:3]

    def build(**kw):
        seed_all(rec["seed"])
        cls = ka.NecessaryPostTrainingEngine if mode == "necessary" else ka.SufficientPostTrainingEngine
        eng = cls(model, ds, rec["hp"])
        if mode == "sufficient":
            eng.select_entities_to_convert(pred, block["k"], block["degree_cap"])
        return eng, ka.StochasticBuilder(1e9, eng, max_explanation_length=1, **kw).build_explanations(pred, cands)

    _, plain = build()
    eng, res = build(trace=True)
    assert eng.trace is True and "traces" not in plain and set(res) == set(plain) | {"traces"}
    assert res["rule_to_relevance"] == plain["rule_to_relevance"] and res["#relevances"] == plain["#relevances"]
    assert len(res["traces"]) == len(res["rule_to_relevance"]) >= 1
    for t in res["traces"]:
        for side in ([t] if mode == "necessary" else t):
            assert set(side) == {"base", "post"} | ({"entity"} if mode == "sufficient" else set())
            assert side["post"] and side["base"] and side["post"] != side["base"]
