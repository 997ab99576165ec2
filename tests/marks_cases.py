"""The epoch marks' cases (TEST INFRASTRUCTURE), read by test_marks_gpu.py and by its CPU
companion in test_marks_cpu.py.

The batches are width_cases.py's: on the 517-entity graph, two ordinary subjects with the base
post-training and two singleton candidates each, 8 epochs, marks after epochs 0, 1, 3 and 8
(the TransE hub subject: one candidate, 3 epochs, marks 0, 1, 3).  Every slot takes one step
per epoch there.  ``MIXED`` cases run one subject with a batch size that gives its base
post-training 3 steps per epoch, its first rule 2 and its second rule 1 (ConvE steps over
(head, relation) pairs: the largest batch size that gives its three slots three different counts).

The reference of every mark is the stand-in's answer by the definition (marks_backend.py): the
oracle on the same batch with ``hp.epochs = e``, recorded with the rank rule's bounds from the
oracle's own score row (width_cases.rank_bounds).
"""
from __future__ import annotations

import numpy as np

import kelpie_amd as ka
import width_cases as wc
from golden_io import seed_all
from marks_backend import MarksContext, hp_with_epochs  # noqa: F401 (re-exported)

MARKS = [0, 1, 3, 8]
HUB_MARKS = [0, 1, 3]
# ComplEx / DistMult kelpie rows start as init * INIT_SCALE: at width_cases' 1e-3 every score of
# mark 0 lies within the rank rule's delta of the target and the rule decides nothing there
INIT_SCALE = 0.5

# ``seed`` (of the weights) per case, as width_cases chooses it: the stand-in alone meets
# check_marks_vacuity (test_marks_cpu.py asserts it)
CASES = [
    wc._case("ComplEx", 8, seed=4),      # row 16
    wc._case("ComplEx", 32, seed=4),     # row 64
    wc._case("ComplEx", 200, seed=3),    # row 400
    wc._case("DistMult", 40, seed=4),
    wc._case("DistMult", 200, seed=3),
    wc._case("ConvE", 60, seed=3),
    wc._case("ConvE", 200, seed=4),
    wc._case("TransE", 16, seed=10),
    wc._case("TransE", 200, seed=3),
    wc._case("TransE", 260, seed=7),
    wc._case("TransE", 260, tag="hub", hub=True, seed=5),
]
MIXED = [dict(wc._case(m, d, tag="mixed", seed=s), mixed=True)
         for m, d, s in (("ComplEx", 32, 4), ("DistMult", 40, 4), ("ConvE", 60, 4), ("TransE", 16, 3))]


def ids(cases):
    return [c["id"] for c in cases]


def marks_of(case):
    return HUB_MARKS if case["hub"] else MARKS


class Capture:
    """Wraps a context: runs every posttrain_rank call with ``want_x`` and keeps its arguments
    (copied: the native TransE path hands out views of reused arenas) and everything it returned."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.batches = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def posttrain_rank(self, hp, *arrays, want_x=False, **kw):
        args = (type(hp).from_buffer_copy(hp),) + tuple(np.array(a, copy=True) for a in arrays)
        out = self._ctx.posttrain_rank(hp, *arrays, want_x=True, **kw)
        self.batches.append({"args": args, "kw": dict(kw), "out": out})
        return out[:2] + (out[2] if want_x else None,) + tuple(out[3:])


def _pairs_steps(rows_h_r, bs):
    return -(-len(set(rows_h_r)) // bs)


def mixed_plan(case):
    """(pred, rules, batch_size) of a MIXED case: the first ordinary subject, a rule of one
    triple and a rule of more than half of its triples."""
    _, ds, ordinary, _ = wc.graph(case["n_ent"])
    pred = ordinary[0]
    mine = sorted(ds.entity_to_training_triples[pred[0]])
    n = len(mine)
    rules = [mine[:1], mine[:(n + 2) // 2]]
    if case["model"] != "ConvE":
        return pred, rules, n - 1  # 2n rows: 3 steps; 2n - 2: 2 steps; at most n - 1: 1 step

    def pairs(triples):  # the (head, relation) pairs of the triples and their inverses
        nr = ds.num_relations
        return [(h, r) for h, r, t in triples] + [(t, r + nr) for h, r, t in triples]

    slots = [mine, mine[1:], mine[len(rules[1]):]]
    best = max(range(2, 2 * n), key=lambda bs: (len({_pairs_steps(pairs(s), bs) for s in slots}), bs))
    return pred, rules, best


def run(case, ctx_of):
    """The case's engine batches with marks through ``ctx_of(model)`` wrapped in Capture; the
    captured batches and the model."""
    ds = wc.graph(case["n_ent"])[1]
    model = wc.make_model(case)
    if hasattr(model, "init_scale"):
        model.init_scale = INIT_SCALE
    model._ctx = cap = Capture(ctx_of(model))
    seed_all(42)
    if case.get("mixed"):
        pred, rules, bs = mixed_plan(case)
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(wc.hp_of(case), batch_size=bs))
        eng.marks = marks_of(case)
        eng.compute_relevance_batch(pred, [[tuple(t) for t in r] for r in rules])
        return cap.batches, model
    for pred, epochs, n in wc.subjects(case):
        eng = ka.NecessaryPostTrainingEngine(model, ds, dict(wc.hp_of(case), epochs=epochs))
        eng.marks = marks_of(case)
        cands = sorted(ds.entity_to_training_triples[pred[0]])[:n]
        eng.compute_relevance_batch(pred, [[c] for c in cands])
    return cap.batches, model


def standin_context(model):
    return MarksContext(wc.oracle_context(model), model.name)


_REF = {}


def reference(case):
    """The stand-in side of a case, computed once: per batch, per slot, per mark the record
    {"score", "rank", "lo", "hi", "x"}; and per batch the slots' steps per epoch."""
    if case["id"] not in _REF:
        batches, model = run(case, standin_context)
        _REF[case["id"]] = ([rec for rec in model._ctx._ctx.mark_slots], [steps_per_epoch(model, b) for b in batches])
    return _REF[case["id"]]


def steps_per_epoch(model, batch):
    """Steps per epoch of every slot of a captured batch: rows, ConvE (head, relation) pairs."""
    hp, _, row_off, rows = batch["args"][:4]
    out = []
    for i in range(len(row_off) - 1):
        r = np.asarray(rows[row_off[i]:row_off[i + 1]]).reshape(-1, 3)
        n = len({(int(h), int(p)) for h, p, _ in r}) if model.name == "ConvE" else len(r)
        out.append(-(-n // int(hp.batch_size)))
    return out


def device_marks(batches):
    """Per batch, per slot, per mark {"score", "rank", "x"} of a device run's captured batches."""
    out = []
    for b in batches:
        m_s, m_r, m_x = b["out"][-1]
        out.append([[{"score": float(m_s[i, j]), "rank": int(m_r[i, j]), "x": m_x[i, j].copy()}
                     for j in range(m_s.shape[1])] for i in range(m_s.shape[0])])
    return out


def check_marks_vacuity(ref):
    """The rank rule decides the marks (width_cases.check_vacuity's conditions over every mark of
    a case) and the marks move: some slot has two marks of different rank."""
    flat = [m for batch in ref for slot in batch for m in slot]
    for m in flat:
        assert m["hi"] - m["lo"] <= 1 and m["lo"] <= m["rank"] <= m["hi"], (m["rank"], m["lo"], m["hi"])
    sharp = sum(int(m["hi"] == m["lo"]) for m in flat)
    assert 4 * sharp >= 3 * len(flat), (sharp, len(flat))
    assert any(len({m["rank"] for m in slot}) > 1 for batch in ref for slot in batch)
    for m in flat:
        assert 1.25 * m.get("max_logit", 0.0) < wc.SATURATION, m["max_logit"]
