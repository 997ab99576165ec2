"""The probe cases of the device (TEST INFRASTRUCTURE), shared by test_probes_gpu.py and
its CPU companion in test_probes_cpu.py.

A case is one batch: two subjects x (base + two singleton candidates) = six slots, two
epochs, through the necessary engine; ``ProbeInjector`` adds ``COUNTS[i]`` probes to slot i
of the batch it passes on and records the call.  The probes of a slot, in order:

  0   the slot's own (p, o) with the slot's own filter (consequence 1 of the probes'
      definition: the slot's score bit for bit, its rank exactly);
  1   the kelpie entity as object (o = n_ent), any relation;
  2   an object that its own filter names (a maximizer leaves it out of its own count, the
      minimizer restores it);
  3+  any relation (inverse ones included), any object, a filter of 0 .. 5 columns, the
      kelpie column sometimes among them.

Shapes: entity tables of 255, 256 and 257 rows (the count kernel's 256-column blocks: one
block short of full, one full block plus the kelpie column in a second, two blocks) and 31
(n_ent + 1 a multiple of 32: the filter bitmap's last word is full); probe counts of 0, 1,
15, 16 and 17 per slot (the count kernel ranks 16 rows per workgroup row), the empty slot
between full ones; 65 probes, so five chunks of KP_PROBE_CHUNK=16 rows.

The reference of a probe is a float64 numpy restatement of the model's score row on the
slot's returned final row (``rows64``), held to the project's rank rule (width_cases.py).
The weight seeds are chosen so that the oracle alone shows the rule to decide
(test_probes_cpu.py::test_rank_rule_decides).
"""
from __future__ import annotations

import functools

import numpy as np

import kelpie_amd as ka
import width_cases as wc
from golden_io import seed_all
from kelpie_amd import synth

COUNTS = (16, 0, 17, 1, 15, 16)
EPOCHS = 2


def _case(family, dim, n_ent, seed=3):
    model = family.split("-")[0]
    return {"id": f"{family}-d{dim}-n{n_ent}", "family": family, "model": model, "dim": dim, "n_ent": n_ent,
            "norm": 1 if family.endswith("L1") else 2, "seed": seed}


# every family at 257 entities; the other table sizes on one maximizer and the minimizer.
# ``seed`` (of the weights): 3 unless the oracle's bounds were two apart there
CASES = ([_case(f, d, 257, seed) for f, d, seed in (("ComplEx", 32, 3), ("DistMult", 40, 3), ("ConvE", 60, 3),
                                                     ("TransE-L2", 50, 3), ("TransE-L1", 50, 4))]
         + [_case("ComplEx", 32, n, 4 if n == 256 else 3) for n in (255, 256, 31)]
         + [_case("TransE-L2", 50, n, 5 if n == 255 else 3) for n in (255, 256, 31)]
         + [_case("ConvE", 60, 31)])


def ids(cases=CASES):
    return [c["id"] for c in cases]


@functools.lru_cache(maxsize=None)
def graph(n_ent):
    """(dataset, two test predictions whose subjects have 6 to 40 training triples)."""
    if n_ent < 100:
        _, ds, ordinary, _ = wc.graph(n_ent)
        return ds, ordinary[:2]
    g = synth.make_graph("tiny", seed=11, n_ent=n_ent, n_rel=6, n_train=1500, n_valid=60, n_test=60)
    ds = ka.Dataset(g.num_entities, g.num_relations, g.train, g.valid, g.test)
    deg = ds.entity_to_degree
    preds, seen = [], set()
    for t in (tuple(int(v) for v in t) for t in g.test):
        if 6 <= deg.get(t[0], 0) <= 40 and t[0] not in seen:
            seen.add(t[0])
            preds.append(t)
    assert len(preds) >= 2, (n_ent, len(preds))
    return ds, preds[:2]


def make_model(case):
    ds, _ = graph(case["n_ent"])
    m, d, seed = case["model"], case["dim"], case["seed"]
    if m == "ConvE":
        w = synth.make_weights("ConvE", ds.num_entities, ds.num_relations, d, seed=seed, conve_random_bn=True,
                               trained_scale=0.5)
        bn = {i: {"weight": w[f"bn{i}_weight"], "bias": w[f"bn{i}_bias"], "running_mean": w[f"bn{i}_mean"],
                  "running_var": w[f"bn{i}_var"]} for i in (1, 2, 3)}
        return ka.ConvE(ds, w["entity_embeddings"], w["relation_embeddings"], w["conv_weight"].reshape(32, 3, 3),
                        w["conv_bias"], w["fc_weight"], w["fc_bias"], bn=bn, hidden_dropout_rate=0.2)
    if m == "TransE":
        w = synth.make_weights("TransE", ds.num_entities, ds.num_relations, d, seed=seed)
        scale = np.exp(np.random.default_rng(1000 + seed).uniform(np.log(0.5), np.log(4.0), ds.num_entities))
        return ka.TransE(ds, (w["entity_embeddings"] * scale[:, None]).astype(np.float32), w["relation_embeddings"],
                         norm=case["norm"])
    # unit-scale tables: after two epochs the kelpie row is still small, and the scores of
    # (kelpie, p, .) must spread wider than the rank rule's delta over the table
    w = synth.make_weights(m, ds.num_entities, ds.num_relations, d, seed=seed, trained_scale=1.0)
    cls = ka.ComplEx if m == "ComplEx" else ka.DistMult
    return cls(ds, w["entity_embeddings"], w["relation_embeddings"], init_scale=1e-3)


def hp_of(case):
    base = {"ComplEx": wc.CX_HP, "DistMult": wc.CX_HP, "ConvE": wc.CV_HP, "TransE": wc.TE_HP}[case["model"]]
    return dict(base, epochs=EPOCHS)


def plan_probes(case, n_ent, n_rel2, pred, filt_off, filt):
    """(probe_off, probes [n][2], filt_off, filt) of the batch's slots (module docstring)."""
    rng = np.random.default_rng(1 + case["seed"] + n_ent)
    p_off, tr, f_off, fl = [0], [], [0], []
    for i in range(len(pred)):
        own = [int(e) for e in filt[filt_off[i]:filt_off[i + 1]]]
        for j in range(COUNTS[i % len(COUNTS)]):
            p, o = int(rng.integers(n_rel2)), int(rng.integers(n_ent + 1))
            f = [int(e) for e in rng.integers(0, n_ent + 1, int(rng.integers(0, 6)))]
            if j == 0:
                p, o, f = int(pred[i][1]), int(pred[i][2]), own
            elif j == 1:
                o = n_ent
            elif j == 2:
                f = f + [o]
            tr.append((p, o))
            fl += f
            f_off.append(len(fl))
        p_off.append(len(tr))
    return (np.array(p_off, np.int32), np.array(tr, np.int32).reshape(-1, 2), np.array(f_off, np.int32),
            np.array(fl or [0], np.int32))


class ProbeInjector:
    """Wraps a context that serves ``probes`` (and ``topk``): adds the planned probes to
    every batch it passes on and records the call's arguments, probes and results."""

    def __init__(self, ctx, case, n_rel2, topk=0, with_probes=True):
        self._ctx, self._case, self._n_rel2, self._topk, self._with = ctx, case, n_rel2, topk, with_probes
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def posttrain_rank(self, hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=False):
        n_ent = int(pred[0][0])
        probes = plan_probes(self._case, n_ent, self._n_rel2, pred, filt_off, filt)
        kw = {"topk": self._topk} if self._topk else {}
        if self._with:
            kw["probes"] = probes
        out = self._ctx.posttrain_rank(hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt, want_x=True, **kw)
        self.calls.append({"pred": np.array(pred), "filt_off": np.array(filt_off), "filt": np.array(filt),
                           "probes": probes, "out": out})
        return out[0], out[1], (out[2] if want_x else None)


def run(case, ctx_of, topk=0, with_probes=True):
    """The case's batch through ``ctx_of(model)`` (a context that serves probes); the
    recorded call and the model."""
    ds, preds = graph(case["n_ent"])
    model = make_model(case)
    model._ctx = ProbeInjector(ctx_of(model), case, 2 * ds.num_relations, topk, with_probes)
    seed_all(42)
    eng = ka.NecessaryPostTrainingEngine(model, ds, hp_of(case))
    eng.compute_relevance_multi([(p, [[c] for c in sorted(ds.entity_to_training_triples[p[0]])[:2]]) for p in preds])
    assert len(model.ctx.calls) == 1 and len(model.ctx.calls[0]["pred"]) == 6
    return model.ctx.calls[0], model


def oracle_ctx(model):
    """The family's oracle-backed stand-in, wrapped to serve probes (and lists)."""
    from probe_backend import ProbeContext
    from topk_backend import TopkContext
    return ProbeContext(TopkContext(wc.oracle_context(model), model.is_minimizer()), model.is_minimizer())


# ----------------------------------------------------------------------------- the float64 restatement
def rows64(model, ref_ctx, p, x):
    """float64 scores of (kelpie, p, .) over [E; x] for the final row ``x``: the model's
    score function restated in numpy (ConvE: the oracle's encoder, then float64 logits)."""
    E = np.vstack([model.entity_embeddings, np.asarray(x, np.float32)[None]]).astype(np.float64)
    r = model.relation_embeddings[p].astype(np.float64)
    x = np.asarray(x, np.float64)
    if model.name == "ComplEx":
        h = len(x) // 2
        q = np.concatenate([x[:h] * r[:h] - x[h:] * r[h:], x[:h] * r[h:] + x[h:] * r[:h]])
        return E @ q
    if model.name == "DistMult":
        return E @ (x * r)
    if model.name == "TransE":
        diff = (x + r)[None] - E
        return np.abs(diff).sum(1) if model.norm == 1 else np.sqrt((diff ** 2).sum(1))
    om = ref_ctx.inner.om
    enc, _ = om.conve_encode(np.asarray(x, np.float32)[None], om.R[[p]])
    return 1.0 / (1.0 + np.exp(-(E @ enc[0].astype(np.float64))))


def check_probes(call, model, ref_ctx):
    """Every probe of the recorded call against ``rows64`` on its slot's returned final
    row: score within TOL * max(1, |ref|), rank inside the rank rule's bounds.  Returns
    (probes, exact rank matches, sharp probes, widest bounds): the callers print or hold them."""
    from probe_backend import triple_results
    minimizer = model.is_minimizer()
    p_off, tr, f_off, fl = call["probes"]
    x = call["out"][2]
    ps, prk = call["out"][-1]
    n = exact = sharp = widest = 0
    for i in range(len(p_off) - 1):
        rows = {}
        for j in range(p_off[i], p_off[i + 1]):
            p, o = int(tr[j, 0]), int(tr[j, 1])
            if p not in rows:
                rows[p] = rows64(model, ref_ctx, p, x[i])
            f = fl[f_off[j]:f_off[j + 1]]
            t, rank = triple_results(rows[p], f, o, minimizer)
            lo, hi = wc.rank_bounds(rows[p], t, f, o, minimizer)
            assert abs(float(ps[j]) - t) <= wc.TOL * max(1.0, abs(t)), (i, j, p, o, float(ps[j]), t)
            assert lo <= int(prk[j]) <= hi, (i, j, p, o, int(prk[j]), rank, lo, hi)
            n += 1
            exact += int(int(prk[j]) == rank)
            sharp += int(lo == hi)
            widest = max(widest, hi - lo)
    return n, exact, sharp, widest


def check_own_target(call):
    """Consequence 1: probe 0 of every slot with probes is the slot's own target."""
    p_off = call["probes"][0]
    s, r = call["out"][0], call["out"][1]
    ps, prk = call["out"][-1]
    hit = 0
    for i in range(len(p_off) - 1):
        if p_off[i + 1] > p_off[i]:
            j = p_off[i]
            assert np.float32(ps[j]).tobytes() == np.float32(s[i]).tobytes(), (i, float(ps[j]), float(s[i]))
            assert int(prk[j]) == int(r[i]), (i, int(prk[j]), int(r[i]))
            hit += 1
    return hit
