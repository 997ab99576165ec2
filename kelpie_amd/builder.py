"""Stochastic explanation builder driving the batched engine.

Same algorithm, output and RNG use as the reference
``src/explanation_builders/stochastic_builder.py:13-192`` (without
summarisation), restructured for a batched engine:

* all singleton rules of a prediction are evaluated in ONE engine batch
  (the reference's hot loop A, ``:110-124``);
* compound rules are evaluated in speculative windows of rules in prescore
  order (hot loop B, ``:126-175``).  The accept / early-return /
  ``random.random()`` termination logic is then replayed sequentially over the
  window's relevances; if the search stops inside the window, the torch /
  numpy generators are rewound to the state right after the last rule the
  reference would have evaluated, so every later draw is unchanged.

With ``pipelined`` the next window is scheduled while the current one runs on the device
(its draws follow the current window's, on this thread; its slots are packed on its batch
thread), but it is held: its device work starts only once the replay of the current
window has gone through without a stop (``engine.submit_batch(hold=True)``,
``release_batch``).  A stop inside the current window cancels it with no device work and
rewinds the generators past both, so only host work is ever thrown away.  Off by default:
the look-ahead's size is chosen before the current window's relevances are known, so its
windows run past more stops (273 against 245 evaluations for the same 224 relevances), and
that costs more device time than overlapping the host schedule saves (the schedule is 11 %
of the builder's time, the library call 85 %): headline builder leg, alternating on one
box, 439.8 / 456.9 relevances/s held look-ahead against 485.1 / 480.8 sequential
(profiles/r06/r06y/r06y7_*).  A first form started the look-ahead at once on the second
context: 392.5 / 394.7 against 452.3 / 453.1 (profiles/r06/r06i/).

Window sizes: a fixed ``window``, or ``window="auto"``: the rules before index 10
of a length (the sliding window's size: no stochastic stop can happen there, only
the early exit on ``xsi``) go as one window, and after that each window holds about
as many rules as the search is expected to run before it stops, from the stop
probability the replay has reached (1 - average / best of the sliding window),
between ``AUTO_MIN`` and ``AUTO_MAX`` rules.  Either way the results, the draws and
``#relevances`` are those of the sequential reference; only the device work spent
past a stop (``stats["wasted"]``) and the number of engine batches change.

With ``top_k`` > 0 the engine also reports, for every post-training, the k tails the
post-trained row would predict (``engine.top_k``), and each record gains
``"counterfactuals"``, aligned with ``rule_to_relevance``: per rule the ``base`` and
``post`` lists of [label, score] pairs (the sufficient engine: one such pair of lists per
conversion entity, with its label); the kelpie entity is printed as ``kelpie:`` plus the
label of the entity it clones.  The lists come with the batches the search runs anyway.

With ``side_effects`` = cap > 0 every post-training also ranks the subject's other held-out
facts (``engine.side_effects``: its validation then test triples without the prediction,
the first ``cap``), and each record gains ``"side_effects"``, aligned with
``rule_to_relevance``: per rule the probe count ``"probes"``, ``"base"`` and ``"post"`` =
{"mrr", "h1"} over the probes (compute_metrics' formulas and rounding) and ``"ranks"`` =
[labelled triple, base rank, post rank] per probe (the sufficient engine: one such record
per conversion entity, with its label).  A base result cached without probes gives None
for the base figures.

With ``trace`` = True every post-training also reports the optimizer's loss of each of its
steps (``engine.trace``), and each record gains ``"traces"``, aligned with
``rule_to_relevance``: per rule ``{"base", "post"}``, each the list of losses in step order
(the sufficient engine: one such record per conversion entity, with its label).  A base
result cached without a trace gives None.

With ``margins`` = a tolerance in [0, 1] every post-training also reports how far its rank is
from changing (``engine.margin_tol``), and each record gains ``"margins"``, aligned with
``rule_to_relevance``: per rule ``engine.compute_margins``' report of it -- ``"relevance_lo"``
/ ``"relevance_hi"`` and ``"base"`` / ``"post"`` with the rank bands, the ties and the nearest
competitors (the sufficient engine: ``"conversions"``, one such pair per conversion entity,
with its label).  A base result cached without margins gives None for its figures and for the
band.  Not offered with a pipelined builder.

With ``attributions`` = True every post-training also splits its score change over its facts
(``engine.attributions``; ComplEx and DistMult under Adagrad or SGD), and each record gains
``"attributions"``, aligned with ``rule_to_relevance``: per rule
``engine.compute_attributions``' report of it -- ``"base"`` / ``"post"`` with ``"score0"``,
``"delta"`` and the slot's labelled facts with their ``"fit"`` and ``"reg"`` (the sufficient
engine: ``"conversions"``, one such pair per conversion entity, with its label).  A base result
cached without attributions gives None.  Not offered with a pipelined builder.
"""
from __future__ import annotations

import itertools
import random
import time


class StochasticBuilder:
    AUTO_MIN, AUTO_MAX = 4, 32

    def __init__(self, xsi, engine, summarization: str = None, max_explanation_length: int = 4, window=32,
                 pipelined=False, top_k=0, side_effects=0, trace=False, draws=None, seed=None, margins=None,
                 attributions=False):
        if summarization is not None:
            raise NotImplementedError("summarisation (simulation / bisimulation) is out of scope")
        # the source of the post-training draws (PostTrainingEngine.draws / .seed; None: as the
        # engine has it).  Keyed draws have nothing to rewind: the windows' checkpoints are
        # taken and restored as ever and change nothing; the pipelined builder is not offered
        if seed is not None:
            engine.seed = seed
        if draws is not None:
            engine.draws = draws
        if pipelined and getattr(engine, "draws", "reference") == "keyed":
            raise NotImplementedError("draws='keyed' with a pipelined builder: keyed batches run one at a time")
        self.xsi = xsi
        self.engine = engine
        self.dataset = engine.dataset
        self.length_cap = max_explanation_length
        self.window_size = 10  # the reference's sliding window (stochastic_builder.py:24)
        self.auto = window == "auto"
        self.pipelined = bool(pipelined) and hasattr(engine, "submit_batch")
        self.spec_window = self.AUTO_MAX if self.auto else max(1, int(window))
        self.summarization = None
        self.top_k = int(top_k)
        if self.top_k:
            engine.top_k = self.top_k  # validates the range
        self.side_effects = int(side_effects)
        if self.side_effects:
            engine.side_effects = self.side_effects  # validates the range
        self.trace = bool(trace)
        if self.trace:
            engine.trace = True
        self.margins = margins
        if margins is not None:
            engine.margin_tol = margins  # validates the type and the range
            self.margins = engine.margin_tol
            if pipelined:
                raise NotImplementedError("margins with a pipelined builder: batches with margins run one at a time")
        self.attributions = bool(attributions)
        if self.attributions:
            if pipelined:
                raise NotImplementedError("attributions with a pipelined builder: batches with attributions run "
                                          "one at a time")
            engine.attributions = True
        self._details = {}  # rule -> the engine's (post-trained, base) results of its evaluation
        self.stats = {"batches": 0, "evaluated": 0, "wasted": 0, "batch_s": 0.0, "schedule_s": 0.0, "pack_s": 0.0,
                      "lib_s": 0.0}

    def _account(self, t0):
        """Wall time of one engine batch and the engine's host / library split of it."""
        self.stats["batch_s"] += time.perf_counter() - t0
        bs = getattr(self.engine, "last_batch_stats", None)
        if isinstance(bs, dict):
            for k in ("schedule_s", "pack_s", "lib_s"):
                self.stats[k] += float(bs.get(k, 0.0) or 0.0)

    def build_explanations(self, pred, candidate_triples: list, k: int = 10):
        start = time.time()
        candidate_triples = [tuple(int(v) for v in t) for t in candidate_triples]
        self._details = {}
        triple_to_rel = self.explore_singleton_rules(pred, candidate_triples)
        srt = sorted(triple_to_rel.items(), key=lambda x: x[1], reverse=True)
        rule_to_rel = [((t,), rel) for (t, rel) in srt]
        triples_number = len(triple_to_rel)
        rels_num = triples_number
        _, best = rule_to_rel[0]
        if not best > self.xsi:
            for rule_length in range(2, min(triples_number, self.length_cap) + 1):
                cur, cur_n = self.explore_compound_rules(pred, candidate_triples, rule_length, triple_to_rel)
                rels_num += cur_n
                cur = sorted(cur.items(), key=lambda x: x[1], reverse=True)
                rule_to_rel += cur
                _, current_best = cur[0]
                if current_best > best:
                    best = current_best
                if best > self.xsi:
                    break
        rule_to_rel = sorted(rule_to_rel, key=lambda x: (x[1], 1 / len(x[0])), reverse=True)[:k]
        mapped = [(self.dataset.labels_triples(rule), rel) for rule, rel in rule_to_rel]
        out = {"triple": self.dataset.labels_triple(tuple(pred)), "rule_to_relevance": mapped,
               "#relevances": rels_num, "execution_time": time.time() - start}
        if self.top_k:
            out["counterfactuals"] = [self._counterfactual(pred, self._details[rule]) for rule, _ in rule_to_rel]
        if self.side_effects:
            out["side_effects"] = [self._side_effect(self._details[rule]) for rule, _ in rule_to_rel]
        if self.trace:
            out["traces"] = [self._trace_of(self._details[rule]) for rule, _ in rule_to_rel]
        if self.margins is not None:
            out["margins"] = [self._margins_of(rel, self._details[rule]) for rule, rel in rule_to_rel]
        if self.attributions:
            out["attributions"] = [self._attributions_of(pred, rel, self._details[rule]) for rule, rel in rule_to_rel]
        return out

    def _keep_details(self, rules, n):
        """The engine's per-rule results of its last batch, for the first ``n`` of ``rules``."""
        if self.top_k or self.side_effects or self.trace or self.margins is not None or self.attributions:
            for rule, det in zip(rules[:n], self.engine.last_results):
                self._details[tuple(rule)] = det

    def _labelled(self, res, cloned):
        """A result's list as [label, score] pairs; None when it was cached without one."""
        if res.get("top_ids") is None:
            return None
        ds, k = self.dataset, self.top_k
        return [["kelpie:" + ds.id_to_entity[cloned] if e == ds.num_entities else ds.id_to_entity[e], float(v)]
                for e, v in zip(res["top_ids"][:k], res["top_scores"][:k])]

    def _counterfactual(self, pred, det):
        if isinstance(det, tuple):  # necessary: (post-trained, base) of the prediction's subject
            pt, base = det
            s = int(pred[0])
            return {"base": self._labelled(base, s), "post": self._labelled(pt, s)}
        # sufficient: one pair per conversion entity
        return [{"entity": self.dataset.id_to_entity[e], "base": self._labelled(base, e), "post": self._labelled(pt, e)}
                for e, (pt, base) in zip(self.engine.entities_to_convert, det)]

    def _margins_of(self, rel, det):
        """engine.compute_margins' report of one rule, a conversion entity by its label."""
        out = self.engine._mg_rule(rel, det, self.margins)
        for c in out.get("conversions", ()):
            c["entity"] = self.dataset.id_to_entity[c["entity"]]
        return out

    def _attributions_of(self, pred, rel, det):
        """engine.compute_attributions' report of one rule, entities and facts by their labels."""
        out = self.engine._at_rule(pred, rel, det)
        sides = [out] if "base" in out else out["conversions"]
        for c in sides:
            if "entity" in c:
                c["entity"] = self.dataset.id_to_entity[c["entity"]]
            for side in (c["base"], c["post"]):
                for f in side["facts"] or ():
                    f["triple"] = self.dataset.labels_triple(f["triple"])
        return out

    def _trace_of(self, det):
        if isinstance(det, tuple):  # necessary: (post-trained, base) of the prediction's subject
            pt, base = det
            return {"base": base.get("loss"), "post": pt.get("loss")}
        # sufficient: one pair per conversion entity
        return [{"entity": self.dataset.id_to_entity[e], "base": base.get("loss"), "post": pt.get("loss")}
                for e, (pt, base) in zip(self.engine.entities_to_convert, det)]

    @staticmethod
    def _probe_metrics(ranks):
        """MRR and H@1 of a list of ranks (compute_metrics' formulas and rounding,
        kelpie_amd/verification.py); None for no ranks.  A maximizer's filtered object does
        not count itself (get_triple_results), so a held-out fact the model answers first
        has rank 0: it enters both figures as rank 1."""
        if not ranks:
            return None
        ranks = [max(1, int(r)) for r in ranks]
        acc = 0.0
        for r in ranks:
            acc += 1.0 / float(r)
        return {"mrr": round(acc / float(len(ranks)), 3),
                "h1": round(sum(1.0 for r in ranks if r <= 1) / float(len(ranks)), 3)}

    def _side_effect_pair(self, pt, base):
        post = pt.get("probes") or []
        before = base.get("probes")
        ranks = [[list(self.dataset.labels_triple(p["triple"])), None if before is None else before[i]["rank"], p["rank"]]
                 for i, p in enumerate(post)]
        return {"probes": len(post),
                "base": None if before is None else self._probe_metrics([p["rank"] for p in before]),
                "post": self._probe_metrics([p["rank"] for p in post]), "ranks": ranks}

    def _side_effect(self, det):
        if isinstance(det, tuple):  # necessary: (post-trained, base) of the prediction's subject
            return self._side_effect_pair(*det)
        # sufficient: one pair per conversion entity
        return [dict(self._side_effect_pair(pt, base), entity=self.dataset.id_to_entity[e])
                for e, (pt, base) in zip(self.engine.entities_to_convert, det)]

    def explore_singleton_rules(self, pred, triples: list):
        # one engine batch for every singleton; a duplicated candidate is evaluated
        # once per occurrence and the last value wins, like the dict of :113-123
        t0 = time.perf_counter()
        rels = self.engine.compute_relevance_batch(pred, [[t] for t in triples])
        self._account(t0)
        self._keep_details([(t,) for t in triples], len(triples))
        self.stats["batches"] += 1
        self.stats["evaluated"] += len(triples)
        out = {}
        for t, r in zip(triples, rels):
            out[t] = r
        return out

    def explore_compound_rules(self, pred, triples, length, triple_to_relevance):
        rules = itertools.combinations(triples, length)
        rules = [(r, sum(triple_to_relevance[t] for t in r)) for r in rules]
        rules = sorted(rules, key=lambda x: x[1], reverse=True)
        terminate = False
        best = -1e6
        window = [None] * self.window_size
        rule_to_relevance = {}
        computed = 0
        i = 0
        eng = self.engine
        ahead = None  # the next window, scheduled and started speculatively: (rules, checkpoints, batch)

        def submit(at, hold=False):
            chunk = [r for r, _ in rules[at:at + self._window(at, window, best)]]
            cps = []
            if self.pipelined:
                return chunk, cps, eng.submit_batch(pred, [list(r) for r in chunk], checkpoints=cps, hold=hold)
            return chunk, cps, None

        prev_cps = None
        while i < len(rules) and not terminate:
            if ahead is not None:
                chunk, cps, batch = ahead
                ahead = None
                if len(chunk) > self._window(i, window, best):
                    # sized before the previous window's relevances were known and larger than
                    # the window the sequential search now takes here: cancel it (no device
                    # work), rewind to its start and schedule the sequential one
                    eng.finish_batch(batch, discard=True)
                    self.stats["lookahead_resized"] = self.stats.get("lookahead_resized", 0) + 1
                    prev_cps[-1].restore()
                    chunk, cps, batch = submit(i)
                else:
                    eng.release_batch(batch)  # the previous window ran through: start its device work
            else:
                chunk, cps, batch = submit(i)
            prev_cps = cps
            if self.pipelined:
                t0 = time.perf_counter()
                if i + len(chunk) < len(rules):
                    # scheduled and packed while `batch` runs on the device, held until the
                    # replay below has gone through `batch` without a stop
                    ahead = submit(i + len(chunk), hold=True)
                try:
                    rels = eng.finish_batch(batch)
                except BaseException:
                    if ahead is not None:
                        eng.finish_batch(ahead[2], discard=True)  # cancelled: no device work
                    raise
                self._account(t0)
            else:
                t0 = time.perf_counter()
                rels = eng.compute_relevance_batch(pred, [list(r) for r in chunk], checkpoints=cps)
                self._account(t0)
            self._keep_details(chunk, len(rels))
            self.stats["batches"] += 1
            self.stats["evaluated"] += len(chunk)
            stop_at = None
            for j, rel in enumerate(rels):
                ii = i + j
                rule = chunk[j]
                rule_to_relevance[rule] = rel
                computed += 1
                window[ii % self.window_size] = rel
                if rel > self.xsi:
                    stop_at, terminate = j, True
                    break
                elif rel >= best:
                    best = rel
                elif ii >= self.window_size:
                    avg = sum(window) / self.window_size
                    thr = avg / best
                    if random.random() > thr:
                        stop_at, terminate = j, True
                        break
            if stop_at is not None:
                if ahead is not None:
                    # the held next window: cancelled before any device work (its host
                    # schedule is all that is lost); rewind past it and this window's later rules
                    eng.finish_batch(ahead[2], discard=True)
                    self.stats["lookahead_cancelled"] = self.stats.get("lookahead_cancelled", 0) + 1
                    ahead = None
                    cps[stop_at].restore()
                elif stop_at + 1 < len(chunk):
                    cps[stop_at].restore()  # rewind the speculative draws
                self.stats["wasted"] += len(chunk) - stop_at - 1
            i += len(chunk)
        return rule_to_relevance, computed

    def _window(self, i, window, best):
        """Rules in the next speculative window (see the module docstring)."""
        if not self.auto:
            return self.spec_window
        if i < self.window_size:
            return self.window_size - i
        if any(v is None for v in window) or best == 0:
            # a window scheduled before the replay has filled the sliding window (the
            # pipelined builder's look-ahead), or a best of zero: no estimate
            return 2 * self.AUTO_MIN
        if best == 0:
            return self.AUTO_MIN
        thr = (sum(window) / self.window_size) / best
        p_stop = min(1.0, max(0.0, 1.0 - thr))  # P(random.random() > thr) per rule below the best
        if p_stop <= 1.0 / self.AUTO_MAX:
            return self.AUTO_MAX
        return int(min(self.AUTO_MAX, max(self.AUTO_MIN, round(1.0 / p_stop))))
