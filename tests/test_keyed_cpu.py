"""Keyed draws on the CPU: the restatement's statistics, the key derivation, and the engines in
keyed mode on the oracle-backed stand-in (keyed_backend.KeyedStandIn in front of the stand-ins
of width_cases, used as they are).

The statistical thresholds are 5 standard errors of each statistic, derived here from the
sample size; none is a tuned number.  The engine tests use the 517-entity graph of
width_cases with 3 epochs: order independence is a property of the host layer and of the
draws' definition, not of the epoch count."""
import itertools
import math
import random

import numpy as np
import pytest
import torch

import kelpie_amd as ka
import keyed_reference as kr
import width_cases as wc
from keyed_backend import KeyedStandIn
from kelpie_amd import keyed

CASES = {"ComplEx": wc._case("ComplEx", 20, seed=4), "DistMult": wc._case("DistMult", 40, seed=4),
         "TransE": wc._case("TransE", 50, seed=4)}
ENGINES = {"necessary": ka.NecessaryPostTrainingEngine, "sufficient": ka.SufficientPostTrainingEngine}
EPOCHS = 3


# ----------------------------------------------------------------------------- the streams
def test_every_permutation_is_a_permutation():
    for R, e in itertools.product((1, 2, 3, 64, 65, 1000), (0, 1, 5)):
        p = kr.permutation(0xABCDEF0123456789 + R, e, R)
        assert sorted(p.tolist()) == list(range(R)), (R, e)
    # ties keep the row order: equal key words are broken by row index (the argsort is stable)
    w = kr.words(5, kr.PERM, 0, 200000)
    p = np.argsort(w, kind="stable")
    same = w[p][1:] == w[p][:-1]
    assert same.any()  # 2 * 10^5 words of 32 bits: about 4.7 equal pairs are expected
    assert (p[1:][same] > p[:-1][same]).all()


def test_permutation_orders_are_uniform():
    n = 6000
    orders = {o: 0 for o in itertools.permutations(range(3))}
    pos0 = np.zeros(64, np.int64)
    for k in range(n):
        key = keyed.slot_key(k, (1, 2, 3), 1, "necessary", [(1, 2, 3)])
        orders[tuple(kr.permutation(key, 0, 3).tolist())] += 1
        pos0[int(np.nonzero(kr.permutation(key, 1, 64) == 0)[0][0])] += 1
    for cells, counts in ((6, np.array(list(orders.values()))), (64, pos0)):
        p = 1.0 / cells
        se = math.sqrt(n * p * (1 - p))  # binomial standard error of one cell's count
        assert np.abs(counts - n * p).max() <= 5 * se, (cells, counts)


def test_negatives_and_head_or_tail_are_uniform():
    n = 40000
    neg = kr.negatives(0x1234, 0, n, 5)
    assert neg.min() == 0 and neg.max() == 4
    se = math.sqrt(n * 0.2 * 0.8)
    assert np.abs(np.bincount(neg, minlength=5) - n * 0.2).max() <= 5 * se
    hot = kr.head_or_tail(0x1234, 0, n)
    assert set(hot.tolist()) == {0, 1}
    assert abs(int(hot.sum()) - n / 2) <= 5 * math.sqrt(n * 0.25)


def test_normal_rows_have_mean_zero_and_variance_std2():
    n, std = 40000, float(np.float32(math.sqrt(2.0 / 51.0)))
    x = kr.x0_normal(0x77, n, std).astype(np.float64)
    assert abs(x.mean()) <= 5 * std / math.sqrt(n)  # the mean's standard error
    # the sample variance of a normal has standard error std^2 * sqrt(2 / (n - 1))
    assert abs(x.var(ddof=1) - std * std) <= 5 * std * std * math.sqrt(2.0 / (n - 1))
    u = kr.x0_uniform(0x77, n, 1.0).astype(np.float64)
    assert 0.0 <= u.min() and u.max() < 1.0
    assert abs(u.mean() - 0.5) <= 5 * math.sqrt(1.0 / 12.0 / n)


# ----------------------------------------------------------------------------- the keys
def test_key_derivation():
    pred, rule = (5, 2, 9), [(5, 1, 7), (3, 0, 5), (5, 4, 11)]
    k = keyed.slot_key(1, pred, 1, "necessary", rule)
    assert 0 <= k < 2 ** 64 and 0 <= keyed.init_key(1, pred) < 2 ** 64
    for perm in itertools.permutations(rule):  # a rule's triple order does not matter
        assert keyed.slot_key(1, pred, 1, "necessary", list(perm)) == k
    others = [keyed.slot_key(2, pred, 1, "necessary", rule), keyed.slot_key(1, (5, 2, 8), 1, "necessary", rule),
              keyed.slot_key(1, pred, 0, "necessary", rule), keyed.slot_key(1, pred, 1, "sufficient", rule),
              keyed.slot_key(1, pred, 1, "necessary", rule[:2]),
              keyed.slot_key(1, pred, 1, "necessary", [(5, 1, 7), (3, 0, 5), (5, 4, 12)])]
    assert len(set(others + [k])) == len(others) + 1
    # init_key: the seed and the prediction, nothing else
    assert keyed.init_key(1, pred) != keyed.init_key(2, pred) and keyed.init_key(1, pred) != keyed.init_key(1, (5, 2, 8))
    assert keyed.init_key(1, pred) != k
    # the encoding itself, pinned: blake2b-8 of the documented bytes
    import hashlib
    import struct
    data = b"kelpie-keyed/slot\0" + struct.pack("<qiii", 1, 5, 2, 9) + struct.pack("<BBI", 1, 0, 3)
    for t in sorted(rule):
        data += struct.pack("<iii", *t)
    assert k == int.from_bytes(hashlib.blake2b(data, digest_size=8).digest(), "little")
    with pytest.raises(ValueError):
        keyed.slot_key(1, pred, 2, "necessary")


# ----------------------------------------------------------------------------- the engines
def make_engine(model_name, mode, draws="keyed", seed=7):
    case = CASES[model_name]
    ds = wc.graph(case["n_ent"])[1]
    model = wc.make_model(case)
    model._ctx = KeyedStandIn(wc.oracle_context(model), model)
    eng = ENGINES[mode](model, ds, dict(wc.hp_of(case), epochs=EPOCHS))
    eng.draws, eng.seed = draws, seed
    return eng, ds


def inputs(ds, mode="necessary"):
    """Necessary mode: two predictions, three rules of the first and one rule of the second."""
    p1, p2 = wc.graph(517)[2][:2]
    a, b, c = sorted(ds.entity_to_training_triples[p1[0]])[:3]
    other = [sorted(ds.entity_to_training_triples[p2[0]])[0]]
    return p1, p2, [[a], [b, c], [c]], [other]


def run_batch(eng, mode, pred, rules, ents=None):
    if mode == "sufficient":
        eng.entities_to_convert = list(ents)
    return eng.compute_relevance_batch(pred, rules)


def sufficient_inputs(ds):
    """Sufficient mode: the first prediction's facts as rules to add, two conversion entities."""
    p1, p2 = wc.graph(517)[2][:2]
    facts = sorted(ds.entity_to_training_triples[p1[0]])[:3]
    rules = [[facts[0]], [facts[1], facts[2]], [facts[2]]]
    ents = [e for e in range(40, 60) if e not in (p1[0], p2[0]) and 4 <= ds.entity_to_degree.get(e, 0) <= 40][:2]
    assert len(ents) == 2
    return p1, p2, rules, ents


@pytest.mark.parametrize("mode", ["necessary", "sufficient"])
@pytest.mark.parametrize("model_name", ["ComplEx", "DistMult", "TransE"])
def test_order_independence_on_the_stand_in(model_name, mode):
    eng, ds = make_engine(model_name, mode)
    if mode == "necessary":
        p1, p2, rules, other = inputs(ds, mode)
        ents = None
        multi_items = [(p2, other), (p1, rules)]
    else:
        p1, p2, rules, ents = sufficient_inputs(ds)
        multi_items = [(p2, [[sorted(ds.entity_to_training_triples[p2[0]])[0]]], ents), (p1, rules, ents)]
    t_state, n_state = torch.get_rng_state().clone(), np.random.get_state()
    together = run_batch(eng, mode, p1, rules, ents)
    assert eng.model.ctx.keyed_calls == 1
    # each rule alone, in reverse order, each on a fresh engine
    alone = []
    for r in reversed(rules):
        fresh, _ = make_engine(model_name, mode)
        alone.append(run_batch(fresh, mode, p1, [r], ents)[0])
    assert alone[::-1] == together, (alone[::-1], together)
    # a rule's triple order does not matter
    fresh, _ = make_engine(model_name, mode)
    assert run_batch(fresh, mode, p1, [rules[1][::-1]], ents)[0] == together[1]
    # beside another prediction in one device batch
    fresh, _ = make_engine(model_name, mode)
    if mode == "sufficient":
        fresh.entities_to_convert = list(ents)
    assert fresh.compute_relevance_multi(multi_items)[1] == together
    # another seed gives other numbers (the keys are read)
    fresh, _ = make_engine(model_name, mode, seed=8)
    assert run_batch(fresh, mode, p1, rules, ents) != together
    # no generator was read or advanced
    assert torch.equal(torch.get_rng_state(), t_state)
    now = np.random.get_state()
    assert now[0] == n_state[0] and np.array_equal(now[1], n_state[1]) and now[2:] == n_state[2:]


@pytest.mark.parametrize("model_name", ["ComplEx", "TransE"])
def test_reference_mode_is_order_dependent(model_name):
    """The same comparison in reference mode does not hold: there a relevance depends on what
    was drawn before it."""
    from golden_io import seed_all
    eng, ds = make_engine(model_name, "necessary", draws="reference")
    p1, _, rules, _ = inputs(ds, "necessary")
    seed_all(42)
    together = eng.compute_relevance_batch(p1, rules)
    alone = []
    seed_all(42)
    for r in reversed(rules):
        fresh, _ = make_engine(model_name, "necessary", draws="reference")
        alone.append(fresh.compute_relevance_batch(p1, [r])[0])
    assert alone[::-1] != together
    assert eng.model.ctx.keyed_calls == 0


def test_base_and_edited_slots_share_x0():
    eng, ds = make_engine("ComplEx", "necessary")
    p1, _, rules, _ = inputs(ds, "necessary")
    eng.compute_relevance_batch(p1, rules)
    x0, rng_off, _ = eng.model.ctx.fed[0]
    assert len(x0) == 4 and all(np.array_equal(x0[0], x) for x in x0[1:])  # the base slot and the three edited ones
    assert rng_off[-1] == 0  # no slot with R > batch_size: no words, as complex_epochs' rule


def test_builder_default_path_and_checkpoints():
    """The builder's default path in keyed mode: its windows' checkpoints are accepted, and the
    explanation is the same with another speculative window (nothing depends on the order)."""
    outs = []
    for window in (4, 32):
        eng, ds = make_engine("ComplEx", "necessary")
        p1 = wc.graph(517)[2][0]
        cands = sorted(ds.entity_to_training_triples[p1[0]])[:5]
        random.seed(3)
        b = ka.StochasticBuilder(1e9, eng, window=window, max_explanation_length=2, draws="keyed", seed=11)
        assert eng.draws == "keyed" and eng.seed == 11
        t_state = torch.get_rng_state().clone()
        out = b.build_explanations(p1, cands)
        assert torch.equal(torch.get_rng_state(), t_state)
        outs.append(out["rule_to_relevance"])
    assert outs[0] == outs[1]
    cps = []
    eng, ds = make_engine("ComplEx", "necessary")
    p1, _, rules, _ = inputs(ds, "necessary")
    a = eng.compute_relevance_batch(p1, rules, checkpoints=cps)
    assert len(cps) == len(rules)
    cps[0].restore()
    assert eng.compute_relevance_batch(p1, rules) == a


@pytest.mark.parametrize("api", ["compute_counterfactuals", "compute_side_effects", "compute_traces",
                                 "compute_curves"])
def test_extras_in_keyed_mode_on_the_stand_in(api):
    """The four reports take the keyed path: one armed call each, the relevances those of
    compute_relevance_batch, a rule's report the same alone on a fresh engine."""
    import marks_backend
    import probe_backend
    import topk_backend
    import trace_backend

    def engine():
        case = CASES["ComplEx"]
        ds = wc.graph(case["n_ent"])[1]
        model = wc.make_model(case)
        model._ctx = wc.oracle_context(model).inner if api == "compute_curves" else wc.oracle_context(model)
        if api == "compute_curves":
            model._ctx = marks_backend.MarksContext(model._ctx, model.name)
        else:
            {"compute_counterfactuals": topk_backend, "compute_side_effects": probe_backend,
             "compute_traces": trace_backend}[api].wrap(model)
        model._ctx = KeyedStandIn(model._ctx, model)
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(wc.hp_of(case), epochs=EPOCHS))
        eng.draws, eng.seed = "keyed", 7
        return eng, ds

    extra = {"compute_counterfactuals": (3,), "compute_curves": ([0, 1, 3],)}.get(api, ())
    eng, ds = engine()
    p1, _, rules, _ = inputs(ds, "necessary")
    t_state = torch.get_rng_state().clone()
    together = getattr(eng, api)(p1, rules, *extra)
    assert eng.model.ctx.keyed_calls == 1
    plain, _ = make_engine("ComplEx", "necessary")
    assert [r["relevance"] for r in together] == plain.compute_relevance_batch(p1, rules)
    if api != "compute_traces":  # the trace stand-in's values encode the call and the slot, not a loss
        alone = getattr(engine()[0], api)(p1, [rules[2]], *extra)
        assert alone[0] == together[2]
    assert torch.equal(torch.get_rng_state(), t_state)


# ----------------------------------------------------------------------------- refusals
def states():
    return torch.get_rng_state().clone(), np.random.get_state()[1].copy()


def test_refusals_before_any_draw():
    t0, n0 = states()
    eng, ds = make_engine("ComplEx", "necessary")
    p1, _, rules, _ = inputs(ds, "necessary")
    eng.precision = "fp64"
    with pytest.raises(NotImplementedError, match="fp64"):
        eng.compute_relevance_batch(p1, rules)
    eng.precision = "fp32"
    with pytest.raises(NotImplementedError, match="compute_relevance_pipeline"):
        eng.compute_relevance_pipeline([[(p1, rules)]])
    with pytest.raises(NotImplementedError, match="submit_batch"):
        eng.submit_batch(p1, rules)
    with pytest.raises(NotImplementedError, match="pipelined"):
        ka.StochasticBuilder(5, eng, pipelined=True)

    class OneRank:  # a slot sharding that takes the sharded path
        world, rank, force_collective = 2, 0, False
    eng.sharding = OneRank()
    with pytest.raises(NotImplementedError, match="sharding"):
        eng.compute_relevance_batch(p1, rules)
    eng.sharding = None
    assert eng.model.ctx.keyed_calls == 0 and eng.model.ctx.armed is None
    # ConvE: its masks are not keyed
    case = wc._case("ConvE", 100)
    cv = ka.NecessaryPostTrainingEngine(wc.make_model(case), wc.graph(517)[1], wc.hp_of(case))
    cv.draws = "keyed"
    with pytest.raises(NotImplementedError, match="ConvE"):
        cv.compute_relevance_batch(p1, rules)
    with pytest.raises(ValueError):
        eng.draws = "philox"
    with pytest.raises(TypeError):
        eng.seed = 1.5
    with pytest.raises(ValueError):
        eng.seed = 2 ** 63
    t1, n1 = states()
    assert torch.equal(t0, t1) and np.array_equal(n0, n1)
    # the engine still works afterwards
    assert len(eng.compute_relevance_batch(p1, rules)) == 3


def test_default_is_reference_mode():
    eng, _ = make_engine("ComplEx", "necessary", draws="reference")
    fresh = ka.NecessaryPostTrainingEngine(eng.model, eng.dataset, wc.hp_of(CASES["ComplEx"]))
    assert fresh.draws == "reference" and fresh.seed == 0
