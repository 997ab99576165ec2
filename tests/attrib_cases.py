"""The attributions' cases (TEST INFRASTRUCTURE), read by test_attrib_gpu.py and by its CPU
companion test_attrib_cpu.py.

Every case is on width_cases.py's 517-entity graph (17 key tiles, 5 entities in the last) with 8
epochs and holds three engine batches, captured from the necessary engine as it packs them: two
ordinary subjects with the base post-training and two singleton candidates each (one step per
epoch), and the graph's hub subject (817 facts, 1,634 rows) with its base and two candidates at a
batch size of half the candidates' rows: the candidates take two steps per epoch and the base,
two rows longer, three, so the plans are per (epoch, step) and the slots end at different steps.

``crafted`` gives hand-written batches at a row width of 24 (DB 2): a self-loop row, an empty
slot, a repeated relation and pair, a duplicate row; and the full slot alone, a one-slot launch.

``R_C`` is the completeness bound of the device: 8 x the largest completeness residual, relative
to S = sum_i (|fit_i| + |reg_i|), of attrib_reference.py's float32-emulating mode over every slot
of every case here (test_attrib_cpu.py recomputes it and holds this constant against it).  The
factor 8 is the margin for the device's other grouping of the gradient's float32 sum (four wave
partials of four chains), as for f64_cases.TOL_F64.
"""
from __future__ import annotations

import functools

import numpy as np

import kelpie_amd as ka
import width_cases as wc
from golden_io import seed_all
from marks_cases import Capture

EPOCHS = 8
MEASURED_RC = 5.6e-8  # the largest residual / S of the float32-emulating mode (test_attrib_cpu.py)
R_C = 8 * MEASURED_RC
ROW_TOL = 1e-4        # per row, relative to S: the project's row rule (test_gpu_widths.py)
MODE_TOL = 1e-5       # the two modes of the restatement agree within this, relative to S


def _case(model, dim, opt="Adagrad", reg=None, seed=4):
    c = wc._case(model, dim, seed=seed, opt=opt)
    c["regname"] = reg
    c["id"] = f"{model}-d{dim}-DB{c['db']}-{opt}-{reg or 'none'}"
    return c


# (product, d, DB): ComplEx 32 / 4, ComplEx 200 / 25, DistMult 40 / 4, DistMult 200 / 13;
# Adagrad with none / N3 / N2, and SGD.  Every case has single-step and multi-step batches.
# ``seed`` (of the weights) is chosen per case so that the case is well conditioned: the two modes
# of the restatement agree within MODE_TOL per row (test_attrib_cpu.py asserts it; DistMult d = 200
# at seed 3 is not: 1.9e-4 S, Adagrad's first step divides a gradient by its own magnitude)
CASES = [
    _case("ComplEx", 32),
    _case("ComplEx", 32, reg="N3"),
    _case("ComplEx", 32, opt="SGD", reg="N2"),
    _case("ComplEx", 200, reg="N2", seed=6),
    _case("DistMult", 40, reg="N3"),
    _case("DistMult", 40, opt="SGD"),
    _case("DistMult", 200, seed=6),
]


def ids(cases):
    return [c["id"] for c in cases]


def hp_of(case, batch_size=512):
    return dict(wc.CX_HP, optimizer_name=case["opt"], epochs=EPOCHS, batch_size=batch_size,
                lr=0.043 if case["opt"] == "Adagrad" else 0.5,
                regularizer_name=case["regname"] or "N3", regularizer_weight=0.05 if case["regname"] else 0)


class NullContext:
    """A context that post-trains nothing: it lets the engine pack its batches (Capture keeps
    them) where no result is needed."""

    def __init__(self, model):
        self.n_ent, self.dim = model.dataset.num_entities, model.dimension

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False, **kw):
        assert not kw
        n = len(row_off) - 1
        return np.zeros(n, np.float32), np.ones(n, np.int64), np.zeros((n, self.dim), np.float32)

    def last_timing(self):
        return {"device_s": 0.0, "hot_s": 0.0, "hot_launches": 0}


def hub_batch_size(case):
    """Half the rows of the hub's candidate slots: those take two steps per epoch, the base three."""
    return (wc.hub_rows(case)) // 2


def plan(case):
    """[(pred, candidates, batch_size)]: the batches of a case."""
    _, ds, ordinary, hub = wc.graph(case["n_ent"])
    return [(p, 2, 512) for p in ordinary[:2]] + [(hub, 2, hub_batch_size(case))]


@functools.lru_cache(maxsize=None)
def batches(case_id):
    """The case's batches as posttrain_rank arguments (hp, x0, row_off, rows, rng_off, rng, pred,
    filt_off, filt), packed by the necessary engine from seed 42, and a fresh model."""
    case = next(c for c in CASES if c["id"] == case_id)
    ds = wc.graph(case["n_ent"])[1]
    model = wc.make_model(case)
    model._ctx = cap = Capture(NullContext(model))
    seed_all(42)
    for pred, n, bs in plan(case):
        eng = ka.NecessaryPostTrainingEngine(model, ds, hp_of(case, bs))
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        eng.compute_relevance_batch(pred, [[c] for c in cands])
    model._ctx = None
    return [b["args"] for b in cap.batches], model


def crafted(prod):
    """(args, model) of the hand-written batch at a row width of 24: ComplEx d = 12 or DistMult
    d = 24, Adagrad with N3.  The rows of a full slot: a repeated relation (rows 0, 2, 4 and 5
    share relation 1; rows 0 and 5 are one triple twice: a duplicate row), a repeated frozen pair
    (rows 3, 6), a self-loop (row 4).  Three batches: ``[0]`` the full slot, an empty slot and the
    full slot again under another init and pred, one step per epoch (batch size 16); ``[1]`` the
    full slot at batch size 3, three steps per epoch from its own permutations, so the duplicate
    rows part; ``[2]`` the full slot alone in one step per epoch: a one-slot launch."""
    dim = 12 if prod == "ComplEx" else 24
    case = wc._case(prod, dim, seed=4)
    model = wc.make_model(case)
    K, nr = model.dataset.num_entities, model.dataset.num_relations
    r1, r2 = 1, 2
    rows0 = np.array([[K, r1, 3], [K, r2, 5], [K, r1, 4], [6, r1 + nr, K], [K, r1, K], [K, r1, 3], [6, r1 + nr, K],
                      [7, r2 + nr, K]], np.int64)
    rng = np.random.default_rng(24)
    x0 = (rng.random((3, model.dimension)) * 0.2).astype(np.float32)
    pred = np.array([[K, r1, 9], [K, r2, 11], [K, r1, 12]], np.int64)
    filt = np.array([3, 5, 4], np.int64)

    def args(hp, slots):
        """``slots``: [(rows, draws, which init / pred / filter)]"""
        ro = np.concatenate([[0], np.cumsum([len(r) for r, _, _ in slots])]).astype(np.int32)
        go = np.concatenate([[0], np.cumsum([len(d) for _, d, _ in slots])]).astype(np.int64)
        dr = np.concatenate([d for _, d, _ in slots]).astype(np.int32)
        at = [i for _, _, i in slots]
        return (model.kp_hp(hp), x0[at], ro, np.vstack([r for r, _, _ in slots]), go,
                dr if len(dr) else np.zeros(1, np.int32), pred[at], np.arange(len(slots) + 1, dtype=np.int32), filt[at])

    empty, none = np.zeros((0, 3), np.int64), np.zeros(0, np.int32)
    perms = np.concatenate([np.random.default_rng(100 + e).permutation(len(rows0)) for e in range(EPOCHS)])
    reg = {"opt": "Adagrad", "regname": "N3"}
    return [args(hp_of(reg, 16), [(rows0, none, 0), (empty, none, 1), (rows0, none, 2)]),
            args(hp_of(reg, 3), [(rows0, perms, 0)]),
            args(hp_of(reg, 16), [(rows0, none, 0)])], model


@functools.lru_cache(maxsize=None)
def reference(case_id, mode="f32"):
    """attrib_reference.batch of every batch of a case (or of ``crafted-<product>``), computed once
    and shared: [(fit, reg, delta, x)]."""
    import attrib_reference as ar
    bs, model = crafted(case_id.split("-")[1]) if case_id.startswith("crafted-") else batches(case_id)
    E, R = model.entity_embeddings, model.relation_embeddings
    out = [ar.batch(product_of(model), E, R, *b[:7], mode=mode) for b in bs]
    for o in out:
        for a in o:
            a.setflags(write=False)
    return out


def residuals(out, args):
    """Per slot of one batch (|sum_i (fit_i + reg_i) - delta|, S)."""
    fit, reg, delta = out[:3]
    ro = args[2]
    return [(abs(float((fit[ro[s]:ro[s + 1]] + reg[ro[s]:ro[s + 1]]).sum()) - float(delta[s])), slot_scale(fit, reg, ro, s))
            for s in range(len(ro) - 1)]


def slot_scale(fit, reg, row_off, s):
    """S = sum_i (|fit_i| + |reg_i|) of slot s."""
    a, z = int(row_off[s]), int(row_off[s + 1])
    return float(np.abs(fit[a:z]).sum() + np.abs(reg[a:z]).sum())


def product_of(model):
    return "DistMult" if model.name == "DistMult" else "ComplEx"
