"""Attributions, CPU tier.  The device side is test_attrib_gpu.py, the host check and the row map
test_attrib_check.py.

1. The restatement (attrib_reference.py) pinned independently of its hand-derived gradients: with
   every row gradient taken by torch autograd of the reference-shaped loss (CrossEntropy over
   [E; x] plus the regulariser, one row at a time) it gives the same ``fit`` and ``reg``.
2. Completeness of its float64 mode on every case of attrib_cases.py.
3. The conditions that let the GPU tests decide: the two modes agree per row within 1e-5 S, every
   case has rows of both signs, a multi-step duplicate row pair has unequal values and a
   single-step one equal values.
4. ``compute_attributions``, ``rank_facts``, ``engine.attributions``, the builder's and the
   pipeline's ``attributions=`` over the oracle-backed stand-ins wrapped to answer attributions by
   the restatement (attrib_backend.py), necessary and sufficient, ComplEx and DistMult; every
   refusal by its message with the generators left alone.
5. ``R_C``, the device's completeness bound, from the float32-emulating mode.

Bounds from measurements (each 8 x the value measured here, the factor f64_cases.TOL_F64 takes;
DESIGN.md section 3 records them):
    MEASURED_AUTOGRAD = 1.1e-16   largest |restated - autograd| over the rows of the toy, / S
    MEASURED_COMPLETE = 2.2e-16   largest |sum_i (fit_i + reg_i) - delta| / S, float64 mode
"""
import inspect
import random

import numpy as np
import pytest
import torch

import attrib_cases as ac
import attrib_reference as ar
import kelpie_amd as ka
import width_cases as wc
from attrib_backend import AttribStandIn
from golden_io import seed_all
from keyed_backend import KeyedStandIn
from kelpie_amd import _lib
from kelpie_amd.pipeline import build_pipeline, run_explain
from marks_cases import Capture

MEASURED_AUTOGRAD = 1.1e-16
TOL_AUTOGRAD = 8 * MEASURED_AUTOGRAD
MEASURED_COMPLETE = 2.2e-16
TOL_COMPLETE = 8 * MEASURED_COMPLETE
EPOCHS = 3  # the host layers do not depend on the epoch count
MODES = ("necessary", "sufficient")
ALL = ac.ids(ac.CASES) + ["crafted-ComplEx", "crafted-DistMult"]


def _state():
    return (torch.get_rng_state().numpy().tobytes(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
            random.getstate())


def _batches(case_id):
    return ac.crafted(case_id.split("-")[1])[0] if case_id.startswith("crafted-") else ac.batches(case_id)[0]


# ----------------------------------------------------------------------------- 1. autograd
class _HP:
    def __init__(self, opt, reg):
        self.optimizer = _lib.KP_OPT[opt]
        self.epochs, self.batch_size = 4, 5
        self.lr, self.eps = (0.1, 1e-10) if opt == "Adagrad" else (0.5, 0.0)
        self.reg_weight = 0.0 if reg is None else 0.05
        self.reg_kind = 1 if reg == "N2" else 0


def _toy(prod):
    """57 entities, 6 relations, rows of width 8: kelpie-head rows, frozen-head rows, a self-loop,
    duplicate rows; 12 rows at a batch size of 5: three minibatches per epoch."""
    rng = np.random.default_rng(0)
    N, NR, d = 57, 6, 8
    E, R = rng.normal(size=(N, d)) * 0.3, rng.normal(size=(NR, d)) * 0.3
    K = N
    facts = [(K, 0, 3), (K, 0, 7), (5, 1, K), (K, 2, 9), (K, 0, 3), (K, 1, K)]
    rows = np.array(facts + [(t, (r + NR // 2) % NR, h) for h, r, t in facts])
    x0 = (rng.random(d) * 0.3).astype(np.float32)
    perms = np.concatenate([np.random.default_rng(1 + e).permutation(len(rows)) for e in range(4)])
    return E.astype(np.float32), R.astype(np.float32), rows, x0, perms, (K, 2, 11)


def _autograd(prod, E, R, hp):
    """grad_fn by torch autograd, float64: CrossEntropy of the row's scores over [E; x] against its
    target, and the regulariser's factors of the kelpie entity (N3: sum |f|^3, N2: ||f||^3)."""
    Et, Rt = torch.tensor(E, dtype=torch.float64), torch.tensor(R, dtype=torch.float64)
    K, w, n2 = len(E), hp.reg_weight, hp.reg_kind == 1

    def product(lhs, rel):
        if prod == "DistMult":
            return lhs * rel
        h = lhs.shape[-1] // 2
        a, b, c, e = lhs[:h], lhs[h:], rel[:h], rel[h:]
        return torch.cat([a * c - b * e, a * e + b * c])

    def factor(x):
        if prod == "DistMult":
            return torch.sqrt(x * x)
        h = x.shape[-1] // 2
        return torch.sqrt(x[:h] ** 2 + x[h:] ** 2)

    def grad_fn(x, row):
        h, r, t = (int(v) for v in row)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        Eall = torch.cat([Et, xt[None]])
        scores = Eall @ product(Eall[h], Rt[r])
        loss = torch.nn.functional.cross_entropy(scores[None], torch.tensor([t]))
        gamma, = torch.autograd.grad(loss, xt)
        rho = torch.zeros_like(xt)
        if w:
            xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            f = factor(xr)
            one = torch.linalg.vector_norm(f, 2) ** 3 if n2 else (f ** 3).sum()
            rho, = torch.autograd.grad(w * ar.occurrences(row, K) * one, xr)
        return gamma.numpy(), rho.numpy()

    return grad_fn


@pytest.mark.parametrize("reg", [None, "N3", "N2"])
@pytest.mark.parametrize("opt", ["Adagrad", "SGD"])
@pytest.mark.parametrize("prod", ["ComplEx", "DistMult"])
def test_restatement_against_autograd(prod, opt, reg):
    E, R, rows, x0, perms, pred = _toy(prod)
    hp = _HP(opt, reg)
    mine = ar.attributions(prod, E, R, hp, x0, rows, perms, pred, mode="f64")
    auto = ar.attributions(prod, E, R, hp, x0, rows, perms, pred, mode="f64", grad_fn=_autograd(prod, E, R, hp))
    S = float(np.abs(auto["fit"]).sum() + np.abs(auto["reg"]).sum())
    worst = max(float(np.abs(mine[k] - auto[k]).max()) for k in ("fit", "reg")) / S
    print(f"{prod} {opt} {reg}: |restated - autograd| / S = {worst:.2e}; S = {S:.3e}")
    assert S > 0 and (reg is None) == (not np.abs(auto["reg"]).any())
    assert worst <= TOL_AUTOGRAD
    assert abs(mine["delta"] - auto["delta"]) <= TOL_AUTOGRAD * S
    # rows 0 and 4 are one triple twice and part in the three minibatches
    assert mine["fit"][0] != mine["fit"][4]


# ----------------------------------------------------------------------------- 2. completeness
@pytest.mark.parametrize("case_id", ALL)
def test_f64_mode_is_complete(case_id):
    worst = 0.0
    for out, args in zip(ac.reference(case_id, "f64"), _batches(case_id)):
        for resid, S in ac.residuals(out, args):
            if S > 0:
                worst = max(worst, resid / S)
            else:
                assert resid == 0.0
    print(f"{case_id}: largest float64 completeness residual / S = {worst:.2e}")
    assert worst <= TOL_COMPLETE


# ----------------------------------------------------------------------------- 3. conditions
@pytest.mark.parametrize("case_id", ALL)
def test_inputs_can_decide(case_id):
    worst = 0.0
    for o32, o64, args in zip(ac.reference(case_id, "f32"), ac.reference(case_id, "f64"), _batches(case_id)):
        ro = args[2]
        for s in range(len(ro) - 1):
            a, z = int(ro[s]), int(ro[s + 1])
            if a == z:
                continue
            S = ac.slot_scale(o32[0], o32[1], ro, s)
            for k in (0, 1):
                worst = max(worst, float(np.abs(o32[k][a:z] - o64[k][a:z]).max()) / S)
            tot = o32[0][a:z] + o32[1][a:z]
            assert (tot > 0).any() and (tot < 0).any(), (case_id, s)
    print(f"{case_id}: largest |f32 mode - f64 mode| per row / S = {worst:.2e}")
    assert worst <= ac.MODE_TOL


@pytest.mark.parametrize("prod", ["ComplEx", "DistMult"])
def test_duplicate_rows(prod):
    """Rows 0 and 5 of the crafted slot are one triple twice: equal values in one step per epoch,
    unequal ones where the permutations part them."""
    single, multi, alone = ac.reference(f"crafted-{prod}", "f32")
    assert single[0][0] == single[0][5] and single[1][0] == single[1][5]
    assert alone[0][0] == alone[0][5]
    assert multi[0][0] != multi[0][5]
    # the frozen pair's two rows as well
    assert single[0][3] == single[0][6] and multi[0][3] != multi[0][6]


# ----------------------------------------------------------------------------- 5. R_C
def test_completeness_bound_of_the_device():
    worst = 0.0
    for case_id in ALL:
        for out, args in zip(ac.reference(case_id, "f32"), _batches(case_id)):
            for resid, S in ac.residuals(out, args):
                if S > 0:
                    worst = max(worst, resid / S)
    print(f"largest float32-emulating completeness residual / S = {worst:.3e}; R_C = {ac.R_C:.3e}")
    assert worst <= ac.MEASURED_RC and ac.R_C == 8 * ac.MEASURED_RC
    assert ac.MEASURED_RC <= 2 * worst  # the recorded figure is the measured one, rounded up


# ----------------------------------------------------------------------------- 4. the host layers
HOST = {"ComplEx": wc._case("ComplEx", 32, seed=4), "DistMult": wc._case("DistMult", 40, seed=4)}


def standin(model):
    return AttribStandIn(wc.oracle_context(model))


def _engine(name, mode, reg=None, keyed=False, opt="Adagrad"):
    case = dict(HOST[name], opt=opt, regname=reg)
    ds, ordinary = wc.graph(517)[1:3]
    model = wc.make_model(case)
    model._ctx = cap = Capture(standin(model))
    if keyed:
        model._ctx = KeyedStandIn(cap, model)
    hp = dict(ac.hp_of(case), epochs=EPOCHS)
    cls = ka.NecessaryPostTrainingEngine if mode == "necessary" else ka.SufficientPostTrainingEngine
    eng = cls(model, ds, hp)
    if mode == "sufficient":
        eng.entities_to_convert = [int(p[0]) for p in ordinary if p[0] != ordinary[0][0]][:2]
    if keyed:
        eng.draws, eng.seed = "keyed", 7
    return eng, ds, cap


def _pred_rules(ds):
    pred = wc.graph(517)[2][0]
    return pred, [[c] for c in sorted(ds.entity_to_training_triples[pred[0]])[:2]]


def _sides(out, mode):
    for o in out:
        if mode == "necessary":
            yield None, o["base"], o["post"]
        else:
            for c in o["conversions"]:
                yield c["entity"], c["base"], c["post"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["ComplEx", "DistMult"])
def test_engine_reports(name, mode):
    eng, ds, cap = _engine(name, mode, reg="N3")
    pred, rules = _pred_rules(ds)
    seed_all(42)
    out = eng.compute_attributions(pred, rules)
    assert eng.attributions is False and cap._ctx.attrib_calls == [True]
    plain, _, _ = _engine(name, mode, reg="N3")
    seed_all(42)
    assert [o["relevance"] for o in out] == plain.compute_relevance_batch(pred, rules)
    assert plain.model.ctx._ctx.attrib_calls == [False]
    # the raw rows of the one batch, slot by slot in the engine's order: base, post, (base,) post ...
    args, raw = cap.batches[0]["args"], cap.batches[0]["out"][-1]
    row_off, rows = args[2], args[3]
    K = ds.num_entities
    sides = []
    for ent, base, post in _sides(out, mode):
        for side in (base, post):
            if not any(side == s for _, s in sides):
                sides.append((pred[0] if ent is None else ent, side))
    # every slot of the batch is one side of the report (a base is shared by its rules)
    assert len(sides) == len(row_off) - 1
    by_delta = {float(raw[2][i]): i for i in range(len(row_off) - 1)}
    for ent, side in sides:
        i = by_delta[side["delta"]]
        a, z = int(row_off[i]), int(row_off[i + 1])
        F = (z - a) // 2
        assert len(side["facts"]) == F > 0
        for f, fact in enumerate(side["facts"]):
            kt = tuple(int(v) for v in rows[a + f])
            assert fact["triple"] == tuple(ent if v == K and k != 1 else v for k, v in enumerate(kt))
            assert fact["triple"] in ds.entity_to_training_triples[ent] or mode == "sufficient"
            # rows f and f + F are one fact
            assert fact["fit"] == raw[0][a + f] + raw[0][a + F + f] and fact["reg"] == raw[1][a + f] + raw[1][a + F + f]
            assert tuple(int(v) for v in rows[a + F + f]) == (kt[2], kt[1] + ds.num_relations, kt[0])
        assert side["score0"] + side["delta"] == side["score"]
        S = sum(abs(f["fit"]) + abs(f["reg"]) for f in side["facts"])
        assert abs(sum(f["fit"] + f["reg"] for f in side["facts"]) - side["delta"]) <= ac.R_C * S
        assert any(f["reg"] != 0 for f in side["facts"])


def test_cached_base_without_attributions_gives_none():
    eng, ds, cap = _engine("ComplEx", "necessary")
    pred, rules = _pred_rules(ds)
    seed_all(42)
    eng.compute_relevance_batch(pred, rules[:1])  # caches the base result, no attributions
    out = eng.compute_attributions(pred, rules[1:])[0]
    assert out["base"]["facts"] is None and out["base"]["delta"] is None and out["base"]["score0"] is None
    assert out["post"]["facts"] and cap._ctx.attrib_calls == [False, True]


@pytest.mark.parametrize("keyed", [False, True], ids=["reference", "keyed"])
def test_rank_facts(keyed):
    eng, ds, cap = _engine("ComplEx", "necessary", keyed=keyed)
    pred, rules = _pred_rules(ds)
    seed_all(42)
    before = _state()
    ranked = eng.rank_facts(pred)
    # reference draws: the generators are back where a compute_relevance_batch(pred, []) leaves
    # them, which draws nothing; keyed draws: nothing was asked of them
    assert _state() == before
    assert eng.compute_relevance_batch(pred, []) == [] and _state() == before
    assert len(cap.batches) == 1 and len(cap.batches[0]["args"][2]) == 2  # the base slot alone
    facts = sorted(ds.entity_to_training_triples[pred[0]])
    assert sorted(f["triple"] for f in ranked) == facts
    fits = [f["fit"] for f in ranked]
    assert fits == sorted(fits, reverse=True) and fits[0] > 0 > fits[-1]
    assert eng.rank_facts(pred, k=3) == ranked[:3] and eng.rank_facts(pred, k=0) == []
    assert eng.attributions is False and pred not in eng.base_pt_results
    with pytest.raises(ValueError, match="k must be"):
        eng.rank_facts(pred, k=-1)
    if keyed:
        # the base of every keyed relevance of pred: compute_attributions reports the same facts
        base = eng.compute_attributions(pred, rules[:1])[0]["base"]
        assert sorted(base["facts"], key=lambda f: (-f["fit"], f["triple"])) == \
            sorted(ranked, key=lambda f: (-f["fit"], f["triple"]))
        # ... and a cached base with attributions is reused: no further call
        n = len(cap.batches)
        assert eng.rank_facts(pred) == ranked and len(cap.batches) == n
        assert _state() == before


REFUSALS = {
    "TransE": "not linear in the kelpie row", "ConvE": "not linear in the kelpie row",
    "Adam": "optimizer_name='Adam'", "fp64": "precision='fp64'", "sharding": "slot sharding",
    "pipeline": "compute_relevance_pipeline", "submit_batch": "submit_batch",
    "pipelined builder": "pipelined builder", "self-loop": "<s, p, s>", "sufficient self-loop": "<s, p, s>",
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_leave_the_generators_alone(what):
    ds = wc.graph(517)[1]
    mode = "sufficient" if what.startswith("sufficient") else "necessary"
    if what in ("TransE", "ConvE"):
        import margins_cases as gc
        case = next(c for c in gc.FAMILY if c["model"] == what)
        model = wc.make_model(case)
        model._ctx = cap = Capture(wc.oracle_context(model))
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(wc.hp_of(case), epochs=EPOCHS))
    else:
        eng, ds, cap = _engine("ComplEx", mode, opt="Adam" if what == "Adam" else "Adagrad")
    pred, rules = _pred_rules(ds)
    seed_all(42)

    class Sharding:
        world, rank = 2, 0

        def __getattr__(self, name):
            raise AssertionError(f"sharding used: {name}")

    if what == "fp64":
        eng.precision = "fp64"
    elif what == "sharding":
        eng.sharding = Sharding()
    elif what == "self-loop":
        pred = (pred[0], pred[1], pred[0])
    elif what == "sufficient self-loop":
        eng.entities_to_convert = [eng.entities_to_convert[0], pred[2]]
    before = _state()
    with pytest.raises(NotImplementedError, match="attributions") as err:
        if what == "pipeline":
            eng.attributions = True
            eng.compute_relevance_pipeline([[(pred, rules)]])
        elif what == "submit_batch":
            eng.attributions = True
            eng.submit_batch(pred, rules)
        elif what == "pipelined builder":
            ka.StochasticBuilder(5, eng, pipelined=True, attributions=True)
        else:
            eng.compute_attributions(pred, rules)
    assert REFUSALS[what] in str(err.value)
    assert _state() == before and cap.batches == []
    if what not in ("pipeline", "submit_batch", "pipelined builder"):
        assert eng.attributions is False
        eng.attributions = True  # through the attribute as well
        with pytest.raises(NotImplementedError, match="attributions"):
            eng.compute_relevance_batch(pred, rules)
        if mode == "necessary":
            eng.attributions = False
            with pytest.raises(NotImplementedError, match="attributions"):
                eng.rank_facts(pred)
        assert _state() == before and cap.batches == []


def test_attributions_is_a_bool():
    eng, ds, cap = _engine("ComplEx", "necessary")
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="attributions"):
            eng.attributions = bad
    for f in (ka.StochasticBuilder.__init__, build_pipeline, run_explain):
        assert inspect.signature(f).parameters["attributions"].default is False
    assert inspect.signature(_lib.Context.posttrain_rank).parameters["attrib"].default is False


@pytest.mark.parametrize("mode", MODES)
def test_pipeline_records(mode):
    case = dict(HOST["ComplEx"], opt="Adagrad", regname=None)
    ds, ordinary = wc.graph(517)[1:3]
    pred = ordinary[0]
    recs = {}
    for on in (False, True):
        model = wc.make_model(case)
        model._ctx = standin(model)
        seed_all(42)
        pipe = build_pipeline(model, ds, dict(ac.hp_of(case), epochs=EPOCHS), mode, xsi=1e9,
                              **({"attributions": True} if on else {}))
        pipe.builder.length_cap = 1
        recs[on] = pipe.explain(pred, prefilter_k=3, to_convert_k=2) if mode == "sufficient" else \
            pipe.explain(pred, prefilter_k=3)
    plain, rec = recs[False], recs[True]
    assert "attributions" not in plain and set(rec) == set(plain) | {"attributions"}
    assert rec["rule_to_relevance"] == plain["rule_to_relevance"] and rec["#relevances"] == plain["#relevances"]
    assert len(rec["attributions"]) == len(rec["rule_to_relevance"]) > 0
    for (_, rel), a in zip(rec["rule_to_relevance"], rec["attributions"]):
        assert a["relevance"] == rel
        if mode == "necessary":
            assert set(a) == {"relevance", "base", "post"}
            sides = [a["base"], a["post"]]
        else:
            assert set(a) == {"relevance", "conversions"}
            assert [c["entity"] for c in a["conversions"]] == rec["entities_to_convert"]
            sides = [c[k] for c in a["conversions"] for k in ("base", "post")]
        for side in sides:
            assert set(side) == {"score", "rank", "score0", "delta", "facts"}
            assert side["score0"] + side["delta"] == side["score"]
            assert all(isinstance(v, str) for f in side["facts"] for v in f["triple"])
    assert pipe.engine.attributions is True and pipe.builder.attributions is True


def test_library_symbol_and_split():
    assert "kp_posttrain_rank_attrib" in _lib.EXPORTS
    out = (1, 2, 3, "top", "margins", "attrib")
    res = _lib.split_rank_result(out, topk=4, margins=0.5, attrib=True)
    assert res.top == "top" and res.margins == "margins" and res.attrib == "attrib" and res.marks is None
    with pytest.raises(ValueError):
        _lib.split_rank_result(out[:5], topk=4, margins=0.0, attrib=True)
    assert _lib.split_rank_result(out[:5], topk=4, margins=0.0).attrib is None
