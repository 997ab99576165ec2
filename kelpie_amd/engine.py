"""MI355X-native post-training relevance engines.

Drop-in for the reference's ``src/relevance_engines/post_training_engine.py``:
same class names, constructor ``(model, dataset, hp)``, ``set_cache()``,
``compute_relevance(pred, triples) -> float``, ``select_entities_to_convert``
and the same errors.  Underneath, every ``compute_relevance`` call becomes one
or more *slots* of a batched HIP launch (``kp_posttrain_rank``), and
``compute_relevance_batch(pred, rules)`` evaluates many candidates in one
launch while consuming the reference's random draws in the reference's order
(``kelpie_amd.rng``), so a batch returns exactly what the sequential calls
would.
"""
from __future__ import annotations

import math
import os
import random
import time
from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from . import keyed as _keyed
from .hparams import optimizer_hp
from .data import MANY_TO_ONE, ONE_TO_ONE, Dataset, KelpieView
from .models import FrozenModel
from .rng import ReferenceRNG, StateCheckpoint


def _sigmoid(x):
    # post_training_engine.py:19-20 (math.exp overflows below -709 like the reference)
    return 1 / (1 + math.exp(-x))


@dataclass(slots=True)
class _Slot:
    x0: np.ndarray
    rows: np.ndarray
    rng: np.ndarray
    pred: tuple
    filt: list
    result: dict = field(default=None)
    # False: another rank post-trains this slot (kelpie_amd.distributed); only the
    # generators were advanced past its draws, and x0 / rows / rng / filt may be None
    own: bool = True
    # the rank that post-trains it (sharded batches; every rank records every owner, so
    # each knows every rank's record count in the gather)
    owner: int = 0
    # rows and filter held by the library's host scheduler instead of rows / filt:
    # (SchedBatch, its slot index, row count, filter length) (kelpie_amd/_lib.py)
    native: tuple = None
    # probes ranked on this slot's post-trained row (compute_side_effects): a list of
    # (triple in original ids, (p, o) in kelpie form, filter); None: no probes asked for
    probes: list = None
    # keyed draws (engine.draws = "keyed"): (init_key, slot_key) of the slot; x0 and rng are
    # then None and the device generates both (kelpie_amd/keyed.py, Context.arm_keyed)
    keys: tuple = None


def _contiguous_draws(slots, total, ctx=None):
    """The slots' draws as one int32 array.  When they lie back to back in one pooled
    page-locked arena (rng.ReferenceRNG._take with a GPU present), that span itself: the
    library reads it by DMA, no copy.  Otherwise a copy: handing the library a view of a
    pageable arena measured slower end to end (its upload from pages first touched by
    the RNG worker threads took 10-20 ms per TransE batch against 3 ms after a copy into
    a reused buffer, profiles/r02zd_transe_draws_upload.txt).  The copy goes into a
    buffer kept with the device context ``ctx`` (no fresh pages per batch; the context's
    previous batch is done with it) and runs in the library without the interpreter lock,
    so the next batch's scheduling thread is not held up."""
    if total == 0:
        return np.zeros(1, np.int32)
    arrays = [s.rng.reshape(-1) for s in slots]
    live = [a for a in arrays if a.size]
    lease = _lib.arena_of(live[0]) if live else None
    if lease is not None:
        # the draws were written back to back into one page-locked arena in slot order
        # (the usual case): hand the library that span (a view of the lease, which keeps
        # the arena busy while the library reads it), uploaded by DMA
        start = live[0].__array_interface__["data"][0]
        pos = start
        for a in live:
            if _lib.arena_of(a) is not lease or a.__array_interface__["data"][0] != pos or a.dtype.itemsize != 4:
                break
            pos += 4 * a.size
        else:
            off = (start - lease.__array_interface__["data"][0]) // 4
            return lease[off:off + total]
    if ctx is None or any(a.dtype.itemsize != 4 for a in arrays):
        return np.concatenate(arrays).astype(np.int32, copy=False)
    buf = getattr(ctx, "_draw_buf", None)
    if buf is None or buf.size < total:
        buf = np.empty(int(total * 1.25) + 1024, np.int32)
        ctx._draw_buf = buf
    return _lib.gather_i32([np.ascontiguousarray(a) for a in arrays], buf)


class RelevanceEngine:
    """engine.py:13-20 + select_entities_to_convert (engine.py:22-126)."""

    def __init__(self, model: FrozenModel, dataset: Dataset):
        self.model = model
        self.dataset = dataset
        self._o_to_training = None
        # kelpie_amd.distributed.SlotSharding: every rank schedules every batch and
        # post-trains its share of the slots; None = this process does all of them
        self.sharding = None

    @property
    def o_to_training_triples(self):
        if self._o_to_training is None:
            d = {}
            for h, r, t in self.dataset.training_triples.tolist():
                d.setdefault(t, []).append((h, r, t))
            self._o_to_training = d
        return self._o_to_training

    def select_entities_to_convert(self, pred, k: int, degree_cap=None, criage=False):
        ds = self.dataset
        s, p, o = (int(v) for v in pred)
        ents = []
        for e in range(ds.num_entities):
            if e == s:
                continue
            deg = ds.entity_to_degree.get(e, 0)
            if deg < 1:
                continue
            if degree_cap and deg > degree_cap:
                continue
            if criage and e not in self.o_to_training_triples:
                continue
            if (e, p) in ds.to_filter:
                if ds.relation_to_type[p] in (ONE_TO_ONE, MANY_TO_ONE):
                    continue
                if o in ds.to_filter[(e, p)]:
                    continue
            ents.append(e)
        if not ents:
            # the reference returns here WITHOUT resetting entities_to_convert
            # (engine.py:90-91): a sufficient pipeline then reuses the previous
            # prediction's conversion entities
            return []
        fo, fl = [0], []
        for e in ents:
            F = ds.to_filter.get((e, p), [])
            fl.extend(F)
            fo.append(len(fl))
        sh = self.sharding
        if sh is not None and (sh.world > 1 or getattr(sh, "force_collective", False)):
            # entity-range shard of the conversion test, keep mask all-gathered
            lo, hi = len(ents) * sh.rank // sh.world, len(ents) * (sh.rank + 1) // sh.world
            part = np.zeros(0, bool)
            if hi > lo:
                part = self.model.ctx.convertible(np.array(ents[lo:hi]), p, o, np.array(fo[lo:hi + 1]) - fo[lo],
                                                  np.array(fl[fo[lo]:fo[hi]], dtype=np.int64))
            keep = sh.gather_mask(lo, hi, part, len(ents))
        else:
            keep = self.model.ctx.convertible(np.array(ents), p, o, np.array(fo), np.array(fl, dtype=np.int64))
        overall = [e for e, kflag in zip(ents, keep) if kflag]
        chosen = random.sample(overall, k=min(k, len(overall)))  # engine.py:125 (python RNG)
        self.entities_to_convert = chosen
        return chosen


class PostTrainingEngine(RelevanceEngine):
    """post_training_engine.py:17-125."""

    def __init__(self, model: FrozenModel, dataset: Dataset, hp: dict, rng: ReferenceRNG | None = None):
        RelevanceEngine.__init__(self, model=model, dataset=dataset)
        # the reference's optimizer hp class (post_training_engine.py:71): a missing or
        # mistyped field raises pydantic.ValidationError here, before any device work
        self.hp = optimizer_hp(model.name, hp)
        self.rng = rng or ReferenceRNG()
        self._fused = []  # TransE calls whose edits and draws _flush_fused makes in two library calls
        self._sched = None
        self._kp_hp = model.kp_hp(hp)
        self._kp_hp64 = model.kp_hp64(hp) if hasattr(model, "kp_hp64") else None  # the double form (fp64)
        if getattr(model, "is_kelpie", False):
            raise Exception("Already a post-trainable KelpieModel.")
        self.set_cache()
        self.last_batch_stats = {}
        self._top_k = 0
        self._side_effects = 0
        self._probe_req = None
        self._cur_probes = None
        self._trace = False
        self._marks = None
        self._precision = "fp32"
        self._draws = "reference"
        self._seed = 0

    DRAWS = ("reference", "keyed")

    @property
    def draws(self):
        """``"reference"`` (the default: every post-training's kelpie init, epoch shuffles and
        negatives come from the process-global torch / numpy generators in the reference's call
        order, bit for bit) or ``"keyed"``: every slot's random numbers are a pure function of
        ``(seed, prediction, rule)``, generated on the device by a counter-based generator
        (include/kelpie_hip.h, "Keyed draws"; the keys: kelpie_amd/keyed.py).  A relevance is
        then a function of its arguments: the same in any batch, beside any other prediction, in
        any order, on a fresh engine.  A prediction's base and edited post-trainings start from
        the same row.  No keyed call reads or advances the torch or numpy generators;
        ``checkpoints`` lists are accepted and get nothing to rewind.  Python's ``random`` keeps
        its role (the builder's termination, the conversion entities).  TransE, ComplEx and
        DistMult.  Not offered for ConvE, with ``precision = "fp64"``, a slot sharding,
        ``compute_relevance_pipeline`` or ``submit_batch`` (NotImplementedError before any
        work).  Setting it clears the cached base results."""
        return self._draws

    @draws.setter
    def draws(self, value):
        if value not in self.DRAWS:
            raise ValueError(f"draws must be one of {self.DRAWS}, got {value!r}")
        if value != self._draws:
            self.set_cache()
        self._draws = value

    @property
    def seed(self):
        """The seed of the keyed draws (an integer of at most 64 bits, signed; default 0).
        Not read in reference mode.  Setting it clears the cached base results."""
        return self._seed

    @seed.setter
    def seed(self, value):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
            raise TypeError(f"seed must be an integer, got {type(value).__name__}")
        if not -2 ** 63 <= int(value) < 2 ** 63:
            raise ValueError("seed must fit a signed 64-bit integer")
        if int(value) != self._seed:
            self.set_cache()
        self._seed = int(value)

    def _keyed(self):
        return self._draws == "keyed"

    def _refuse_keyed(self, what=None):
        """Keyed mode's refusals, before any work."""
        if not self._keyed():
            return
        if what is not None:
            raise NotImplementedError(f"draws='keyed' on {what}: keyed batches run one at a time")
        if not hasattr(self.model, "keyed_params"):
            raise NotImplementedError(f"draws='keyed': {self.model.name} has no keyed draws "
                                      "(TransE, ComplEx and DistMult only)")
        if self._fp64():
            raise NotImplementedError("draws='keyed' with precision='fp64': kp_posttrain_rank_f64 takes no keys")
        if self._sharded():
            raise NotImplementedError("draws='keyed' with a slot sharding: the keyed results are not gathered "
                                      "across ranks")

    PRECISIONS = ("fp32", "fp64")
    _precision = "fp32"

    @property
    def precision(self):
        """``"fp32"`` (the default: every call goes where it always went) or ``"fp64"``: every
        post-training and rank of ``compute_relevance``, ``compute_relevance_batch`` and
        ``compute_relevance_multi`` runs in double precision on the device
        (``kp_posttrain_rank_f64``; include/kelpie_hip.h, "fp64"), as the reference runs with
        every tensor in float64: the float32 draw upcast and scaled in float64, the Python
        doubles as hyper-parameters, ``target_score`` the double, the relevance formulas in
        float64.  The draws are those of fp32, so the generators end in the same state.
        ComplEx and DistMult only.  Not offered with ``top_k``, probes, ``trace``, ``marks``,
        a slot sharding or ``compute_relevance_pipeline`` (NotImplementedError before any
        draw).  The cached base results are kept per precision."""
        return self._precision

    @precision.setter
    def precision(self, value):
        if value not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {self.PRECISIONS}, got {value!r}")
        if value == "fp64" and not hasattr(self.model, "kelpie_init64"):
            raise NotImplementedError(f"precision='fp64': {self.model.name} has no fp64 post-training "
                                      "(ComplEx and DistMult only)")
        self._precision = value

    def _fp64(self):
        return self._precision == "fp64"

    def _refuse_fp64(self):
        """fp64's refusals, before any draw."""
        if not self._fp64():
            return
        for on, what in ((self._top_k, "top_k"), (self._side_effects or self._probe_req is not None, "probes"),
                         (self._trace, "trace"), (self._marks is not None, "marks")):
            if on:
                raise NotImplementedError(f"precision='fp64' with {what}: kp_posttrain_rank_f64 does not offer it")
        if self._sharded():
            raise NotImplementedError("precision='fp64' with a slot sharding: the fp64 results are not gathered "
                                      "across ranks")

    @property
    def base_pt_results(self):
        """The cached base post-training results of the current precision."""
        return self._base_pt[self._precision]

    @base_pt_results.setter
    def base_pt_results(self, value):
        self._base_pt[self._precision] = value

    _trace = False
    _marks = None  # the epochs after which every post-training is also ranked (marks), int32 array or None
    TOP_K_MAX = 32  # kp_posttrain_rank_topk's largest k
    _top_k = 0
    PROBES_MAX = 64  # probes per slot
    _side_effects = 0    # default probes per prediction (side_effects)
    _probe_req = None    # compute_side_effects' explicit probes: (subject, [triples])
    _cur_probes = None   # the probes of the prediction being scheduled: (subject, [triples]) or None

    @property
    def side_effects(self):
        """How many of the subject's other held-out facts every post-training also ranks (0:
        none, the default; at most ``PROBES_MAX``): the subject's validation then test triples
        without the prediction, the first ``side_effects`` of them, each ranked on the slot's
        post-trained row as ``get_triple_results`` ranks the prediction
        (post_training_engine.py:101-125).  Every slot's result gains ``"probes"``:
        [{"triple", "score", "rank"}].  The relevances, the draws and the batches are those of
        ``side_effects`` = 0."""
        return self._side_effects

    @side_effects.setter
    def side_effects(self, cap):
        if isinstance(cap, bool) or int(cap) != cap:
            raise TypeError(f"side_effects must be an integer, got {cap!r}")
        if not 0 <= int(cap) <= self.PROBES_MAX:
            raise ValueError(f"side_effects must be in [0, {self.PROBES_MAX}], got {cap}")
        self._side_effects = int(cap)

    def default_probes(self, pred, cap):
        """The subject's validation then test triples without the prediction, the first ``cap``."""
        ds = self.dataset
        pred = tuple(int(v) for v in pred)
        held = list(ds.entity_to_validation_triples.get(pred[0], [])) + list(ds.entity_to_testing_triples.get(pred[0], []))
        return [t for t in (tuple(int(v) for v in x) for x in held) if t != pred][:int(cap)]

    def _probes_of(self, pred):
        """(subject, probes) of a prediction about to be scheduled, or None."""
        s = int(pred[0])
        if self._probe_req is not None:
            return self._probe_req
        if self._side_effects:
            return (s, self.default_probes(pred, self._side_effects))
        return None

    def _slot_probes(self, view, delta):
        """The probes of one slot of ``view`` whose edit's filter delta is ``delta`` (None: the
        base slot): each of the prediction's probes moved to the view's entity as the
        prediction is, in kelpie form -- the view's entity as tail gives the inverse relation's
        (p + |R|, head) -- with to_filter[(kelpie, p)] after the edit."""
        if self._cur_probes is None:
            return None
        s, probes = self._cur_probes
        e, k, R = view.original_entity, view.kelpie_entity, self.dataset.num_relations
        out = []
        for t in probes:
            t = Dataset.replace_entity_in_triple(t, s, e)
            a, p, b = view.as_kelpie_triple(t)
            if a != k:
                p, b = p + R, a
            out.append((t, (int(p), int(b)), list(view.filter_for(p, delta.get(p) if delta else None))))
        return out

    @property
    def trace(self):
        """Whether every post-training also reports the optimizer's loss of each of its steps
        (False: the default): the ``l`` the reference's ``step_on_batch`` returns and shows on
        its progress bar (multiclass_nll_optimizer.py:147-164,
        pairwise_ranking_optimizer.py:165-203, bce_optimizer.py:167-208).  Every slot's result
        gains ``"loss"``: [float, ...], one per step.  The relevances, the draws and the batches
        are those of ``trace`` = False."""
        return self._trace

    @trace.setter
    def trace(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"trace must be a bool, got {on!r}")
        self._trace = bool(on)

    @property
    def marks(self):
        """The epochs after which every post-training is also scored and ranked (None: the
        default): one strictly increasing list of 1 to 16 epochs in [0, the hp's epochs].
        Mark ``e`` of a post-training is what the device returns for it on the same batch with
        ``epochs = e``: the kelpie row after ``e`` epochs, ranked as ``get_triple_results``
        ranks the final row (post_training_engine.py:101-125; ConvE in eval mode) -- a shorter
        run reads a prefix of the same draws.  It is not the reference started with
        ``epochs = e`` from the same seed: that run draws fewer numbers per post-training, so
        every post-training after the first starts elsewhere in the random stream.  Every
        slot's result gains ``"marks"``: [{"epoch", "score", "rank"}].  The relevances, the
        draws and the batches are those of ``marks`` = None."""
        return None if self._marks is None else [int(e) for e in self._marks]

    @marks.setter
    def marks(self, epochs):
        self._marks = None if epochs is None else _lib.check_marks(epochs, int(self._kp_hp.epochs))

    _margin_tol = None  # the tolerance of the rank margins every post-training also reports (None: off)

    @property
    def margin_tol(self):
        """The tolerance of the rank margins every post-training also reports (None: none, the
        default; else a real number in [0, 1]): how far the slot's rank is from changing
        (include/kelpie_hip.h, "Rank margins").  With ``delta = margin_tol * max(1, |score|)``
        every slot's result gains ``"margins"``: ``rank_lo`` / ``rank_hi`` (the rank were every
        other column's compared value held against the target's moved by ``delta`` against /
        for the target: ``rank_lo <= rank <= rank_hi``, all equal at 0), ``ties`` (other
        columns equal to the target exactly), ``id_better`` / ``gap_better`` and ``id_worse`` /
        ``gap_worse`` (the nearest strictly better / worse unmasked column and its distance in
        score units; -1 / inf without one; ``num_entities``: the kelpie entity), and ``tol``.
        The relevances, the draws and the batches are those of ``margin_tol`` = None.  Not
        offered with ``precision="fp64"``, a slot sharding, ``compute_relevance_pipeline`` or
        ``submit_batch`` (NotImplementedError before any draw)."""
        return self._margin_tol

    @margin_tol.setter
    def margin_tol(self, tol):
        self._margin_tol = None if tol is None else _lib.check_margin_tol(tol)

    def _refuse_margins(self, what=None):
        """The margins' refusals, before any work."""
        if self._margin_tol is None:
            return
        if what is not None:
            raise NotImplementedError(f"margins on {what}: batches with margins run one at a time")
        if self._fp64():
            raise NotImplementedError("margins with precision='fp64': kp_posttrain_rank_f64 does not offer them")
        if self._sharded():
            raise NotImplementedError("margins with a slot sharding: their results are not gathered across ranks")

    _attrib = False  # whether every post-training also reports its attributions

    @property
    def attributions(self):
        """Whether every post-training also splits its score change over its facts (False: the
        default; include/kelpie_hip.h, "Attributions").  ComplEx and DistMult score the target
        linearly in the kelpie row and Adagrad / SGD apply a diagonal to a sum of per-row
        gradients, so ``score - score0`` splits exactly into one number per training row plus the
        regulariser's share.  Every slot's result gains ``"attrib"``: ``{"facts", "fit", "reg",
        "delta"}`` -- the slot's facts in kelpie form (rows ``f`` and ``f + F``, a fact and its
        inverse, fold to fact ``f``), what fitting each fact contributed, the regulariser's share
        booked to it, and ``delta = <c, x_T - x_0>``; ``sum(fit) + sum(reg) = delta`` up to the
        float32 rounding of the updates.  The relevances, the draws and the batches are those of
        ``attributions`` = False.  Not offered for TransE and ConvE, with an Adam
        ``optimizer_name``, ``precision="fp64"``, a slot sharding, ``compute_relevance_pipeline``,
        ``submit_batch`` or a prediction ``<s, p, s>`` (NotImplementedError before any draw)."""
        return self._attrib

    @attributions.setter
    def attributions(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"attributions must be a bool, got {on!r}")
        self._attrib = bool(on)

    def _refuse_attrib(self, what=None, items=()):
        """The attributions' refusals, before any work.  ``items``: the batch's (pred, rules[,
        entities to convert])."""
        if not self._attrib:
            return
        if what is not None:
            raise NotImplementedError(f"attributions on {what}: batches with attributions run one at a time")
        if self.model.name not in ("ComplEx", "DistMult"):
            raise NotImplementedError(f"attributions: {self.model.name}'s score is not linear in the kelpie row "
                                      "(ComplEx and DistMult only)")
        if int(self._kp_hp.optimizer) == _lib.KP_OPT["Adam"]:
            raise NotImplementedError("attributions with optimizer_name='Adam': its momentum would need one vector "
                                      "per training row (Adagrad and SGD only)")
        if self._fp64():
            raise NotImplementedError("attributions with precision='fp64': kp_posttrain_rank_f64 does not offer them")
        if self._sharded():
            raise NotImplementedError("attributions with a slot sharding: their results are not gathered across "
                                      "ranks")
        for item in items:
            pred = tuple(int(v) for v in item[0])
            heads = [pred[0]] if len(item) < 3 else [int(e) for e in item[2]]
            if pred[2] in heads:
                raise NotImplementedError(f"attributions of a prediction <s, p, s> ({(pred[2], pred[1], pred[2])}): "
                                          "its score is quadratic in the kelpie row")

    @property
    def top_k(self):
        """How many of each post-training's best tails the device also reports (0: none, the
        default; at most ``TOP_K_MAX``).  With ``top_k`` > 0 every slot's result gains
        ``top_ids`` / ``top_scores``: what the post-trained row would predict for
        (kelpie, p, .), best first, filtered entities left out as the rank leaves them out;
        id ``num_entities`` is the kelpie entity itself.  The relevances, the draws and the
        batches are those of ``top_k`` = 0."""
        return self._top_k

    @top_k.setter
    def top_k(self, k):
        if isinstance(k, bool) or int(k) != k:
            raise TypeError(f"top_k must be an integer, got {k!r}")
        if not 0 <= int(k) <= self.TOP_K_MAX:
            raise ValueError(f"top_k must be in [0, {self.TOP_K_MAX}], got {k}")
        self._top_k = int(k)

    def set_cache(self):
        self._base_pt = {p: {} for p in self.PRECISIONS}  # keyed by precision (base_pt_results)
        self.kelpie_dataset_cache_size = 20
        self.kelpie_dataset_cache = OrderedDict()

    def _get_kelpie_dataset(self, original_entity: int) -> KelpieView:
        e = int(original_entity)
        if e not in self.kelpie_dataset_cache:
            self.kelpie_dataset_cache[e] = KelpieView(self.dataset, e)
            self.kelpie_dataset_cache.move_to_end(e)
            if len(self.kelpie_dataset_cache) > self.kelpie_dataset_cache_size:
                self.kelpie_dataset_cache.popitem(last=False)
        return self.kelpie_dataset_cache[e]

    # ------------------------------------------------------------------ slot assembly
    def _slot(self, x0, rows, kelpie_pred, filt):
        draws = self.model.posttrain_draws(rows, self.hp, self.rng)
        return _Slot(x0=x0, rows=rows, rng=draws, pred=tuple(int(v) for v in kelpie_pred), filt=list(filt))

    def _sharded(self):
        sh = self.sharding
        # a one-rank sharding with force_collective takes the sharded path too (its
        # gathers then run through the process group: the RCCL test on one GPU)
        return sh is not None and (sh.world > 1 or getattr(sh, "force_collective", False))

    def _skip_slot(self, kp, rows=None, n_rows=0):
        """A slot another rank post-trains: advance the generators past its draws only."""
        self.model.posttrain_skip(rows, n_rows, self.hp, self.rng)
        return _Slot(x0=None, rows=None, rng=None, pred=tuple(int(v) for v in kp), filt=None, own=False)

    def _schedule(self, pred, triples, mode, slots, pending_base):
        """Consume the draws of one reference compute_relevance call (post_training_engine.py:46-62)
        and append its slots.  Returns (pt_slot, base_key)."""
        pred = tuple(int(v) for v in pred)
        view = self._get_kelpie_dataset(pred[0])
        if self._keyed():
            return self._schedule_keyed(pred, view, triples, mode, slots, pending_base)
        if getattr(self.model, "fused_call_draws", False):
            return self._schedule_fused(pred, view, triples, mode, slots, pending_base)
        if self._sharded():
            return self._schedule_sharded(pred, view, triples, mode, slots, pending_base)
        init = self.rng.rand_init(self.model.dimension)
        kelpie_init = self.model.kelpie_init64 if self._fp64() else self.model.kelpie_init
        x_base = kelpie_init(init, self.rng)  # base KelpieModel is built every call (A-Q6)
        kp = view.as_kelpie_triple(pred)
        if pred not in self.base_pt_results and pred not in pending_base:
            pending_base[pred] = len(slots)
            slots.append(self._slot(x_base, view.base_rows, kp, view.filter_for(kp[1])))
            slots[-1].probes = self._slot_probes(view, None)
        x_pt = kelpie_init(init, self.rng)
        rows, delta = view.removed(triples) if mode == "necessary" else view.added(triples)
        filt = view.filter_for(kp[1], delta.get(kp[1]))
        slots.append(self._slot(x_pt, rows, kp, filt))
        slots[-1].probes = self._slot_probes(view, delta)
        return len(slots) - 1, pred

    def _schedule_keyed(self, pred, view, triples, mode, slots, pending_base):
        """_schedule in keyed mode: the same slots, each with its two keys instead of draws.  No
        generator is asked for anything; the plain path for every family."""
        kp = view.as_kelpie_triple(pred)
        ik = _keyed.init_key(self._seed, pred)
        if pred not in self.base_pt_results and pred not in pending_base:
            pending_base[pred] = len(slots)
            slots.append(_Slot(x0=None, rows=view.base_rows, rng=None, pred=tuple(int(v) for v in kp),
                               filt=list(view.filter_for(kp[1])),
                               keys=(ik, _keyed.slot_key(self._seed, pred, _keyed.ROLE_BASE, mode))))
            slots[-1].probes = self._slot_probes(view, None)
        # the rule in its canonical (sorted) order: an addition appends its rows in the rule's
        # order, and a row's draws go by its position
        triples = sorted(tuple(int(v) for v in t) for t in triples)
        rows, delta = view.removed(triples) if mode == "necessary" else view.added(triples)
        slots.append(_Slot(x0=None, rows=rows, rng=None, pred=tuple(int(v) for v in kp),
                           filt=list(view.filter_for(kp[1], delta.get(kp[1]))),
                           keys=(ik, _keyed.slot_key(self._seed, pred, _keyed.ROLE_EDITED, mode, triples))))
        slots[-1].probes = self._slot_probes(view, delta)
        return len(slots) - 1, pred

    def _schedule_sharded(self, pred, view, triples, mode, slots, pending_base):
        """_schedule when the batch is sharded over ranks (kelpie_amd.distributed): every
        rank walks the same draws in the same order, but only the slots this rank claims
        get their kelpie init, rows, filter and draw values; for the others the
        generators are only advanced (one deferred torch discard for a run of them), so a
        rank's host work is its share of the slots plus the generator walk."""
        m, rng, sh = self.model, self.rng, self.sharding
        kp = view.as_kelpie_triple(pred)
        need_base = pred not in self.base_pt_results and pred not in pending_base
        base_owner = sh.claim_owner(max(1, len(view.base_rows))) if need_base else -1
        own_base = base_owner == sh.rank
        edit = view.removed if mode == "necessary" else view.added
        try:
            n_pt, _ = edit(triples, rows=False)  # the reference raises after the draws below
            err = None
        except Exception as e:  # noqa: BLE001 -- re-raised at the reference's point
            err, n_pt = e, 0
        pt_owner = sh.claim_owner(max(1, n_pt)) if err is None else -1
        own_pt = pt_owner == sh.rank
        if own_base or own_pt:
            init = rng.rand_init(m.dimension)
        else:
            init = None
            rng.skip_rand_init(m.dimension)
        # the base KelpieModel is built every call (A-Q6), then (uncached) post-trained
        x_base = m.kelpie_init(init, rng) if own_base else m.kelpie_skip(rng)
        if need_base:
            pending_base[pred] = len(slots)
            if own_base:
                slots.append(self._slot(x_base, view.base_rows, kp, view.filter_for(kp[1])))
            else:
                slots.append(self._skip_slot(kp, view.base_rows, len(view.base_rows)))
            slots[-1].owner = base_owner
        x_pt = m.kelpie_init(init, rng) if own_pt else m.kelpie_skip(rng)
        if err is not None:
            raise err
        if own_pt or m.skip_needs_rows:
            rows, delta = edit(triples)
        if own_pt:
            slots.append(self._slot(x_pt, rows, kp, view.filter_for(kp[1], delta.get(kp[1]))))
        else:
            slots.append(self._skip_slot(kp, rows if m.skip_needs_rows else None, n_pt))
        slots[-1].owner = pt_owner
        return len(slots) - 1, pred

    def _schedule_fused(self, pred, view, triples, mode, slots, pending_base):
        """_schedule for TransE: the call's slots are appended now and the call is queued;
        :meth:`_flush_fused` then makes the edits and rank filters of every queued call in
        one library call (kp_sched_add_calls, csrc/kp_sched.cpp) and their draws in another
        (ReferenceRNG.transe_calls), in order.  The edit draws nothing; if it fails, the
        flush makes the draws the reference makes before raising (everything but the
        post-trained model's epochs), drops the calls after it, and raises its error."""
        kp = view.as_kelpie_triple(pred)
        need_base = pred not in self.base_pt_results and pred not in pending_base
        sharded = self._sharded()
        nb = view.n_base_rows
        base_owner = pt_owner = 0
        if sharded and need_base:
            base_owner = self.sharding.claim_owner(max(1, nb))
        own_base = need_base and (not sharded or base_owner == self.sharding.rank)
        if sharded:
            # owners from row counts known before the edit: the base rows +- the rule's
            # rows (kelpie_amd.distributed); every rank still runs every edit's checks
            est = nb + 2 * len(triples) if mode == "sufficient" else nb - 2 * len(triples)
            pt_owner = self.sharding.claim_owner(max(1, est))
            own_pt = pt_owner == self.sharding.rank
        else:
            own_pt = True
        sb = self._sched_batch()
        base = None
        if need_base:
            pending_base[pred] = len(slots)
            base = _Slot(None, None, None, kp, None, None, own_base, base_owner, (sb, sb.n_slots))
            sb.n_slots += 1
            slots.append(base)
        pt = _Slot(None, None, None, kp, None, None, own_pt, pt_owner, (sb, sb.n_slots))
        sb.n_slots += 1
        slots.append(pt)
        self._fused_probes(view, triples, mode, base, pt)
        # a queued call: (view, kelpie triple, rule triples, flags, base slot, pt slot)
        self._fused.append((view, kp, [(int(a), int(b), int(c)) for a, b, c in triples],
                            (1 if need_base else 0) | (2 if own_base else 0) | (4 if own_pt else 0)
                            | (8 if mode == "sufficient" else 0), base, pt))
        if len(self._fused) >= (self._FUSED_FLUSH if self._sched is not None else self._FUSED_FIRST):
            # hand the draws to the library's workers early: their numpy shuffles then run
            # while this thread queues the next calls (the batch's first flush sooner, so
            # the sequential numpy chain starts right away)
            self._flush_fused()
        return len(slots) - 1, pred

    def _fused_probes(self, view, triples, mode, base, pt):
        """The probes of a queued TransE call's slots: the library's scheduler makes the edit
        and the rank filter; the probes' filters need the edit's delta here as well."""
        if self._cur_probes is None:
            return
        if base is not None:
            base.probes = self._slot_probes(view, None)
        conv = [Dataset.replace_entity_in_triple(tuple(t), view.original_entity, view.kelpie_entity) for t in triples]
        pt.probes = self._slot_probes(view, view._delta(conv, -1 if mode == "necessary" else +1))

    def _schedule_fused_pred(self, pred, rules, mode, slots, pending_base):
        """:meth:`_schedule_fused` for every rule of one prediction (no checkpoints, no
        empty rule): the same slots, claims and queued calls in the same order, with the
        prediction's view, kelpie triple and row count looked up once.  Returns the
        prediction's [(pt slot index, base key)]."""
        pred = tuple(int(v) for v in pred)
        view = self._get_kelpie_dataset(pred[0])
        kp = view.as_kelpie_triple(pred)
        sharded = self._sharded()
        sh = self.sharding
        nb = view.n_base_rows
        sufficient = mode == "sufficient"
        first = self._sched is None
        sb = self._sched_batch()
        fused, flush_at = self._fused, self._FUSED_FIRST if first else self._FUSED_FLUSH
        out = []
        suf = 8 if sufficient else 0
        append = slots.append
        for rule in rules:
            triples = [(int(a), int(b), int(c)) for a, b, c in rule]
            need_base = pred not in self.base_pt_results and pred not in pending_base
            base_owner = pt_owner = 0
            if sharded and need_base:
                base_owner = sh.claim_owner(max(1, nb))
            own_base = need_base and (not sharded or base_owner == sh.rank)
            if sharded:
                est = nb + 2 * len(triples) if sufficient else nb - 2 * len(triples)
                pt_owner = sh.claim_owner(max(1, est))
                own_pt = pt_owner == sh.rank
            else:
                own_pt = True
            base = None
            j = sb.n_slots
            if need_base:
                pending_base[pred] = len(slots)
                base = _Slot(None, None, None, kp, None, None, own_base, base_owner, (sb, j))
                append(base)
                j += 1
            pt = _Slot(None, None, None, kp, None, None, own_pt, pt_owner, (sb, j))
            append(pt)
            sb.n_slots = j + 1
            if self._cur_probes is not None:
                self._fused_probes(view, triples, mode, base, pt)
            fused.append((view, kp, triples, (1 if need_base else 0) | (2 if own_base else 0) | (4 if own_pt else 0)
                          | suf, base, pt))
            out.append((len(slots) - 1, pred))
            if len(fused) >= flush_at:
                self._flush_fused()
                fused, flush_at = self._fused, self._FUSED_FLUSH
        return out

    def _sched_batch(self):
        """This batch's native scheduler batch (created on its first TransE call)."""
        if self._sched is None:
            self._sched = _lib.SchedBatch()
            self._sched.dim = self.model.dimension
        return self._sched

    # queued TransE calls per library call (KELPIE_TE_FLUSH: A/B of the per-flush overhead
    # against how early the draws reach the workers).  Alternating on two boxes, 30 steps
    # (profiles/r05/r05aj/, r05ak/): 64 averaged 57.9k cand/s over seven runs, 24 50.9k, 48
    # 55.6k over four
    _FUSED_FLUSH = int(os.environ.get("KELPIE_TE_FLUSH", "64"))
    _FUSED_FIRST = 4  # ... for a batch's first one

    @staticmethod
    def _edit_error(call, code, k):
        """The exception KelpieView.removed / added raise (kelpie_dataset.py:92-158)."""
        if code == 1:
            return AssertionError()
        if code == 2:
            v = call[0]
            o, kel = v.original_entity, v.kelpie_entity
            t = call[2][k]
            return KeyError((kel if t[0] == o else t[0], t[1], kel if t[2] == o else t[2]))
        return ValueError("list.remove(x): x not in list")

    def _flush_fused(self):
        """Make the queued TransE calls' edits, rank filters (kp_sched_add_calls) and draws
        (kp_rng_transe_calls, asynchronous) and record them with the scheduler batch: one
        record per flush, whose arrays the pack reads by slot (:meth:`_pack_native`), so no
        per-call Python work is left here beyond building the call arrays."""
        calls, self._fused = self._fused, []
        if not calls:
            return
        m, hp = self.model, self.hp
        sb = self._sched_batch()
        nviews = [c[0].native for c in calls]
        sb.views.extend(nviews)  # its C++ slots point into these views: they live as long as the batch
        off = np.zeros(len(calls) + 1, np.int32)
        np.cumsum([len(c[2]) for c in calls], out=off[1:])
        flags = np.fromiter((c[3] for c in calls), np.int32, len(calls))
        idx, rows, nf, (fc, code, k) = sb.add_calls([v.h for v in nviews], [c[1][1] for c in calls], flags, off,
                                                   [t for c in calls for t in c[2]])
        n = len(calls) if fc < 0 else fc + 1  # the reference stops at the failing call
        has_base = (flags[:n] & 1) != 0
        r_base = np.where(has_base, rows[:n, 0], -1)
        r_pt = rows[:n, 1].copy()
        if fc >= 0:
            r_pt[fc] = -1
        want = ((flags[:n] >> 1) & 3) if self._sharded() else None
        xb, xp, out, sz = self.rng.transe_calls(m.dimension, m.dimension, r_base, r_pt, int(hp["epochs"]),
                                                int(hp["negative_triples_ratio"]), m.dataset.num_entities + 1,
                                                want=want, raw=True)
        # the flush's slots in creation order: per call its base slot (if any), then its pt slot
        first = calls[0][4] if calls[0][4] is not None else calls[0][5]
        present = np.empty((n, 2), bool)
        present[:, 0] = has_base
        present[:, 1] = True
        if fc >= 0:
            present[fc, 1] = False
        sb.recs.append({"j0": first.native[1], "present": present.ravel(), "idx": idx[:n].ravel(),
                        "rows": rows[:n].ravel(), "nf": nf[:n].ravel(), "sz": sz.ravel(), "xb": xb, "xp": xp,
                        "out": out})
        sb.packed = None
        if fc >= 0:
            raise self._edit_error(calls[fc], code, k)

    def _plan_costs(self, items):
        """The claim cost of every slot the batch will schedule, in schedule order, without
        drawing anything: a base slot (first call of an uncached prediction) costs its
        base rows, a post-trained slot its rows after the edit (the costs _schedule_sharded
        claims with); the list stops where the schedule stops (an edit that raises)."""
        costs, pending = [], set()
        for pred, triples, mode in self._calls(items):
            pred = tuple(int(v) for v in pred)
            view = self._get_kelpie_dataset(pred[0])
            if pred not in self.base_pt_results and pred not in pending:
                pending.add(pred)
                costs.append(max(1, len(view.base_rows)))
            edit = view.removed if mode == "necessary" else view.added
            try:
                n_pt, _ = edit(triples, rows=False)
            except Exception:  # noqa: BLE001 -- the schedule raises there too
                break
            costs.append(max(1, n_pt))
        return costs

    def _schedule_all(self, items, checkpoints):
        """_schedule_multi, with every queued TransE call's draws made before it returns or raises."""
        self._refuse_keyed()  # before any work
        self._refuse_margins()  # before any draw
        self._refuse_attrib(items=items)  # before any draw
        self._refuse_fp64()  # before any draw
        if self._top_k and self._sharded():
            # before any draw: the gather's records hold a score and a rank per slot
            raise NotImplementedError("top_k > 0 with a slot sharding: the lists are not gathered across ranks")
        if (self._side_effects or self._probe_req is not None) and self._sharded():
            # before any draw, as the lists
            raise NotImplementedError("probes with a slot sharding: their results are not gathered across ranks")
        if self._trace and self._sharded():
            # before any draw, as the lists and the probes
            raise NotImplementedError("trace with a slot sharding: the losses are not gathered across ranks")
        if self._marks is not None and self._sharded():
            # before any draw, as the lists, the probes and the trace
            raise NotImplementedError("marks with a slot sharding: their results are not gathered across ranks")
        self._sched = None  # this batch's natively assembled slots (TransE), made on first use
        if self._sharded():
            # ComplEx / ConvE: every rank owns one contiguous run of the batch's slots, so it
            # skips the others' draws in two long runs (before and after its own), each one
            # MT19937 jump-ahead instead of a walk (kp_mt19937_discard); TransE's fused calls
            # keep the online greedy claims (its numpy stream cannot be jumped)
            fused = getattr(self.model, "fused_call_draws", False)
            self.sharding.begin_batch(None if fused else self._plan_costs(items))
        try:
            return self._schedule_multi(items, checkpoints)
        finally:
            self._flush_fused()

    def _run(self, slots, ctx=None, gate=None):
        """Post-train and rank ``slots`` on the device.  With ``self.sharding`` only this
        rank's share runs; ``_collect`` then gathers every rank's results.  ``gate``: called
        (blocking) before the library call, after the batch is packed; False cancels the
        batch (no device work, None returned) -- a held look-ahead window (submit_batch)."""
        if not slots:
            return {}
        if self._sharded():
            if gate is not None and not gate():
                return None
            # the slots this rank claimed while scheduling; a failure is reported to the
            # other ranks through the gather (_collect) instead of leaving them waiting in it
            mine = [i for i, s in enumerate(slots) if s.own]
            stats = {"slots": 0, "rows": 0, "pack_s": 0.0, "lib_s": 0.0}
            score, rank, err = [], [], None
            if any(slots[i].owner != self.sharding.rank for i in mine):
                # an owned slot must carry this rank as its owner (the record counts of the
                # gather come from the owners): report it through the gather, never before it
                err, mine = RuntimeError("slot sharding: an owned slot records another rank as its owner"), []
            if mine:
                try:
                    stats = self._run_slots([slots[i] for i in mine], ctx, fill=False)
                    score, rank = stats.pop("_score"), stats.pop("_rank")
                except Exception as e:  # noqa: BLE001 -- raised on every rank by _collect
                    err, mine = e, []
            counts = np.bincount([s.owner for s in slots], minlength=self.sharding.world)
            stats["_local"] = (mine, score, rank, len(slots), err, counts)
            self.last_batch_stats = stats
            return stats
        return self._run_slots(slots, ctx, fill=True, gate=gate)

    def _collect(self, slots, stats):
        """All-gather the ranks' slot results of a sharded batch (in batch order on every rank)."""
        local = stats.pop("_local", None) if stats else None
        if local is None:
            return
        mine, score, rank, n, err, counts = local
        t0 = time.perf_counter()
        try:
            all_s, all_r = self.sharding.gather_slots(mine, score, rank, n, failed=err is not None, counts=counts)
        except Exception:
            if err is not None:
                raise err
            raise
        for i, s in enumerate(slots):
            s.result = {"target_score": float(all_s[i]), "target_rank": int(all_r[i])}
        stats["gather_s"] = time.perf_counter() - t0

    def _pack(self, slots, ctx=None):
        """The library call's batch arrays (x0, row_off, rows, rng_off, rng, pred, filt_off, filt)."""
        n = len(slots)
        if slots and slots[0].native is not None:
            return self._pack_native(slots, ctx)
        # keyed draws: no x0, no rng_off, no rng (the armed context generates them)
        keyed = bool(slots) and slots[0].keys is not None
        x0 = None if keyed else np.stack([s.x0 for s in slots]).astype(np.float64 if self._fp64() else np.float32)
        row_off = np.zeros(n + 1, np.int32)
        row_off[1:] = np.cumsum([len(s.rows) for s in slots])
        rows = np.concatenate([s.rows.reshape(-1, 3) for s in slots]).astype(np.int32) if row_off[-1] \
            else np.zeros((0, 3), np.int32)
        rng_off = rng = None
        if not keyed:
            rng_off = np.zeros(n + 1, np.int64)
            rng_off[1:] = np.cumsum([s.rng.size for s in slots])
            rng = _contiguous_draws(slots, int(rng_off[-1]), ctx)
        pred = np.array([s.pred for s in slots], np.int32)
        filt_off = np.zeros(n + 1, np.int32)
        filt_off[1:] = np.cumsum([len(s.filt) for s in slots])
        filt = np.concatenate([np.asarray(s.filt, np.int32) for s in slots]) if filt_off[-1] \
            else np.zeros(1, np.int32)
        assert keyed or x0.shape == (n, self.model.dimension)
        return x0, row_off, rows, rng_off, rng, pred, filt_off, filt

    @staticmethod
    def _pack_probes(slots):
        """The library call's probe arrays (probe_off, probes [n][2], filt_off, filt)."""
        per = [s.probes or [] for s in slots]
        p_off = np.zeros(len(slots) + 1, np.int32)
        p_off[1:] = np.cumsum([len(p) for p in per])
        flat = [pr for p in per for pr in p]
        tr = np.array([po for _, po, _ in flat], np.int32).reshape(-1, 2)
        f_off = np.zeros(len(flat) + 1, np.int32)
        f_off[1:] = np.cumsum([len(f) for _, _, f in flat])
        filt = np.array([e for _, _, f in flat for e in f] or [0], np.int32)
        return p_off, tr, f_off, filt

    @staticmethod
    def _native_arrays(sb):
        """The scheduler batch's flush records as per-slot arrays (indexed by the slot's
        creation number j): scheduler slot index, row and filter counts, draw count and
        offset, and the kelpie init row.  Read after the batch's draws are complete."""
        if sb.packed is not None and sb.packed[0] == len(sb.recs):
            return sb.packed[1]
        N = sb.n_slots
        idx = np.full(N, -1, np.int32)
        nrow = np.zeros(N, np.int32)
        nfl = np.zeros(N, np.int32)
        nsz = np.zeros(N, np.int64)
        x0 = np.zeros((N, sb.dim), np.float32)
        outs, spans = [], []
        for r in sb.recs:
            pres = r["present"]
            m = int(pres.sum())
            js = r["j0"] + np.arange(m)
            idx[js] = r["idx"][pres]
            nrow[js] = r["rows"][pres]
            nfl[js] = r["nf"][pres]
            nsz[js] = r["sz"][pres]
            n = len(pres) // 2
            both = np.empty((n, 2, sb.dim), np.float32)
            both[:, 0] = r["xb"][:n]
            both[:, 1] = r["xp"][:n]
            x0[js] = both.reshape(2 * n, sb.dim)[pres]
            outs.append(r["out"])
            spans.append((int(js[0]) if m else r["j0"], m))
        # draw offsets per slot within the batch's concatenated draws (records in order)
        doff = np.zeros(N + 1, np.int64)
        np.cumsum(nsz, out=doff[1:])
        arrays = {"idx": idx, "nrow": nrow, "nfl": nfl, "nsz": nsz, "doff": doff, "x0": x0, "outs": outs}
        sb.packed = (len(sb.recs), arrays)
        return arrays

    def _pack_native(self, slots, ctx=None):
        """_pack for the TransE fast path: rows and filters written by the library's
        scheduler (kp_sched_pack), kelpie init rows and draws taken from the flush
        records by slot number."""
        n = len(slots)
        nat = [s.native for s in slots]
        sb = nat[0][0]
        assert all(t[0] is sb for t in nat), "one scheduler batch per device batch"
        a = self._native_arrays(sb)
        js = np.fromiter((t[1] for t in nat), np.int64, n)
        full = n == sb.n_slots and bool(np.all(js == np.arange(n)))
        row_off = np.zeros(n + 1, np.int32)
        np.cumsum(a["nrow"][js], out=row_off[1:])
        filt_off = np.zeros(n + 1, np.int32)
        np.cumsum(a["nfl"][js], out=filt_off[1:])
        rows = np.empty((int(row_off[-1]), 3), np.int32)
        filt = np.empty(max(1, int(filt_off[-1])), np.int32)
        sb.pack(a["idx"][js], rows, filt)
        rng_off = np.zeros(n + 1, np.int64)
        np.cumsum(a["nsz"][js], out=rng_off[1:])
        rng = self._native_draws(a, js, full, int(rng_off[-1]), ctx)
        x0 = a["x0"] if full else a["x0"][js]
        pred = np.array([s.pred for s in slots], np.int32)
        return x0, row_off, rows, rng_off, rng, pred, filt_off, filt

    @staticmethod
    def _native_draws(a, js, full, total, ctx):
        """The draws of slots ``js`` back to back: the span of the page-locked arena the
        flushes' draws were written into when they lie there in slot order (the usual
        case: handed to the library as it is, uploaded by DMA), else a gather."""
        if total == 0:
            return np.zeros(1, np.int32)
        outs = [o for o in a["outs"] if o is not None and o.size]
        if full and outs:
            lease = _lib.arena_of(outs[0])
            start = outs[0].__array_interface__["data"][0]
            pos = start
            for o in outs:
                if lease is None or _lib.arena_of(o) is not lease or o.__array_interface__["data"][0] != pos:
                    break
                pos += 4 * o.size
            else:
                if (pos - start) // 4 == total:
                    off = (start - lease.__array_interface__["data"][0]) // 4
                    return lease[off:off + total]
        flat = np.concatenate(outs) if outs else np.zeros(0, np.int32)
        if full:
            return np.ascontiguousarray(flat[:total], np.int32)
        doff, nsz = a["doff"], a["nsz"]
        parts = [flat[doff[j]:doff[j] + nsz[j]] for j in js.tolist() if nsz[j]]
        return np.concatenate(parts).astype(np.int32, copy=False) if parts else np.zeros(1, np.int32)

    def _run_slots(self, slots, ctx, fill, gate=None):
        t_run = time.perf_counter()
        n = len(slots)
        ctx = ctx or self.model.ctx
        packed = self._pack(slots, ctx)
        if gate is not None and not gate():
            return None
        t_lib = time.perf_counter()
        k = self._top_k
        kw = {"topk": k} if k else {}
        probed = any(s.probes is not None for s in slots)
        if probed:
            kw["probes"] = self._pack_probes(slots)
        traced = self._trace
        if traced:
            kw["trace"] = True
        marks = self._marks
        if marks is not None:
            kw["marks"] = marks
        tol = self._margin_tol
        if tol is not None:
            kw["margins"] = tol
        if self._attrib:
            kw["attrib"] = True
        if slots[0].keys is not None:  # keyed draws: the context generates x0 and the words from the keys
            scale, bound = self.model.keyed_params()
            ctx.arm_keyed([s.keys[0] for s in slots], [s.keys[1] for s in slots], scale, bound)
        if self._fp64():  # the fp64 entry point alone (no optional request: _refuse_fp64)
            out = _lib.RankResult(*ctx.posttrain_rank_f64(self._kp_hp64, *packed))
        else:
            out = _lib.split_rank_result(ctx.posttrain_rank(self._kp_hp, *packed, **kw), **kw)
        score, rank = out.score, out.rank
        t_end = time.perf_counter()
        if fill:
            for i, s in enumerate(slots):
                s.result = {"target_score": float(score[i]), "target_rank": int(rank[i])}
            if marks is not None:
                m_score, m_rank, _ = out.marks
                for i, s in enumerate(slots):
                    s.result["marks"] = [{"epoch": int(e), "score": float(m_score[i][j]), "rank": int(m_rank[i][j])}
                                         for j, e in enumerate(marks)]
            if tol is not None:
                mg = out.margins[0]
                for i, s in enumerate(slots):
                    s.result["margins"] = {"tol": tol, **{name: mg[name][i].item() for name, _ in _lib.MARGIN_FIELDS}}
            if self._attrib:
                a_fit, a_reg, a_delta = out.attrib
                row_off = packed[1]
                for i, s in enumerate(slots):
                    a, z = int(row_off[i]), int(row_off[i + 1])
                    F = (z - a) // 2  # rows f and f + F are fact f and its inverse
                    s.result["attrib"] = {
                        "facts": [tuple(int(v) for v in t) for t in np.asarray(s.rows).reshape(-1, 3)[:F]],
                        "fit": (a_fit[a:a + F] + a_fit[a + F:z]).tolist(),
                        "reg": (a_reg[a:a + F] + a_reg[a + F:z]).tolist(), "delta": float(a_delta[i])}
            if traced:
                for s, loss in zip(slots, out.loss):
                    s.result["loss"] = [float(v) for v in loss]
            if probed:
                p_score, p_rank = out.probes
                j = 0
                for s in slots:
                    s.result["probes"] = [{"triple": t, "score": float(p_score[j + i]), "rank": int(p_rank[j + i])}
                                          for i, (t, _, _) in enumerate(s.probes or [])]
                    j += len(s.probes or [])
            if k:
                top_ids, top_scores = np.asarray(out.top[0]), np.asarray(out.top[1])
                # a list ends at its first -1 (fewer than k unmasked columns)
                short = top_ids < 0
                n_top = np.where(short.any(1), short.argmax(1), top_ids.shape[1])
                for i, s in enumerate(slots):
                    s.result["top_ids"] = top_ids[i, :n_top[i]].tolist()
                    s.result["top_scores"] = top_scores[i, :n_top[i]].tolist()
        stats = {"slots": n, "rows": int(packed[1][-1]), "pack_s": t_lib - t_run, "lib_s": t_end - t_lib,
                 **ctx.last_timing()}
        if not fill:
            stats["_score"], stats["_rank"] = np.array(score), np.array(rank)
        if hasattr(ctx, "hot_intervals"):
            stats["hot_iv"] = ctx.hot_intervals()
        if hasattr(ctx, "last_attn_plan"):
            stats.update(ctx.last_attn_plan())
        self.last_batch_stats = stats
        return stats

    def _base_result(self, key, slots, pending_base):
        if key in self.base_pt_results:
            res = self.base_pt_results[key]
            if self._trace:  # cached without a trace: no post-training runs for its sake
                res.setdefault("loss", None)
            return res
        res = slots[pending_base[key]].result
        self.base_pt_results[key] = res
        return res

    # ------------------------------------------------------------------ reference API
    def compute_relevance(self, pred, triples: list):
        return self.compute_relevance_batch(pred, [triples])[0]

    def compute_relevance_batch(self, pred, rules, checkpoints: list | None = None):
        raise NotImplementedError

    @staticmethod
    def _cf_side(res, k):
        """One post-training of a counterfactual: its target score and rank and its ``top``
        list [(entity id, score)], None when the result was cached without one."""
        ids = res.get("top_ids")
        top = None if ids is None else list(zip(ids[:k], res["top_scores"][:k]))
        return {"score": res["target_score"], "rank": res["target_rank"], "top": top}

    def _cf_rule(self, relevance, detail, k):
        raise NotImplementedError

    def compute_counterfactuals(self, pred, rules, k: int):
        """``compute_relevance_batch(pred, rules)`` -- the same schedule, draws, batches and
        relevances, the generators left where it leaves them -- that also reports what the
        model predicts instead: per rule ``{"relevance", "base", "post"}`` (the sufficient
        engine: ``{"relevance", "conversions": [{"entity", "base", "post"}, ...]}``, one per
        conversion entity), ``base`` / ``post`` = ``{"score", "rank", "top"}`` of the
        post-training without / with the rule's edit, ``top`` the k best tails
        [(entity id, score)] (``num_entities``: the kelpie entity).  No post-training runs for
        the sake of a list: a base result cached while ``top_k`` was 0 reports ``"top": None``."""
        if isinstance(k, bool) or int(k) != k:
            raise TypeError(f"k must be an integer, got {k!r}")
        if not 1 <= int(k) <= self.TOP_K_MAX:
            raise ValueError(f"k must be in [1, {self.TOP_K_MAX}], got {k}")
        old = self._top_k
        self._top_k = max(old, int(k))
        try:
            rels = self.compute_relevance_batch(pred, rules)
        finally:
            self._top_k = old
        return [self._cf_rule(rel, det, int(k)) for rel, det in zip(rels, self.last_results)]

    @staticmethod
    def _se_side(res):
        """One post-training of a side-effects report: its target score and rank and its
        probes' [{"triple", "score", "rank"}], None when the result was cached without them."""
        return {"score": res["target_score"], "rank": res["target_rank"], "probes": res.get("probes")}

    def _se_rule(self, relevance, detail):
        raise NotImplementedError

    def compute_side_effects(self, pred, rules, probes=None, cap=16):
        """``compute_relevance_batch(pred, rules)`` -- the same schedule, draws, batches and
        relevances, the generators left where it leaves them -- that also reports what each
        edit does to the subject's other facts: ``probes`` are triples about the prediction's
        subject (default: :meth:`default_probes`, the first ``cap``), each moved to the slot's
        entity as the prediction is and ranked on the slot's post-trained row as
        ``get_triple_results`` ranks the prediction (post_training_engine.py:101-125).  Per rule
        ``{"relevance", "base", "post"}`` (the sufficient engine: ``{"relevance",
        "conversions": [{"entity", "base", "post"}, ...]}``), ``base`` / ``post`` =
        ``{"score", "rank", "probes"}``, ``probes`` = [{"triple", "score", "rank"}] with the
        triple in original ids.  No post-training runs for the sake of a probe: a base result
        cached without probes reports ``"probes": None``."""
        pred = tuple(int(v) for v in pred)
        if probes is None:
            if isinstance(cap, bool) or int(cap) != cap:
                raise TypeError(f"cap must be an integer, got {cap!r}")
            if int(cap) < 0:
                raise ValueError(f"cap must not be negative, got {cap}")
            probes = self.default_probes(pred, cap)
        probes = [tuple(int(v) for v in t) for t in probes]
        if len(probes) > self.PROBES_MAX:
            raise ValueError(f"at most {self.PROBES_MAX} probes per slot, got {len(probes)}")
        view = self._get_kelpie_dataset(pred[0])
        for t in probes:
            view.as_kelpie_triple(t)  # "Could not find the original entity": before any draw
        self._probe_req = (pred[0], probes)
        try:
            rels = self.compute_relevance_batch(pred, rules)
        finally:
            self._probe_req = None
        return [self._se_rule(rel, det) for rel, det in zip(rels, self.last_results)]

    @staticmethod
    def _tr_side(res):
        """One post-training of a trace report: its target score and rank and the loss of each
        of its steps, None when the result was cached without a trace."""
        loss = res.get("loss")
        return {"score": res["target_score"], "rank": res["target_rank"], "loss": None if loss is None else list(loss)}

    def _tr_rule(self, relevance, detail):
        raise NotImplementedError

    def compute_traces(self, pred, rules):
        """``compute_relevance_batch(pred, rules)`` -- the same schedule, draws, batches and
        relevances, the generators left where it leaves them -- that also reports how every
        post-training went: per rule ``{"relevance", "base", "post"}`` (the sufficient engine:
        ``{"relevance", "conversions": [{"entity", "base", "post"}, ...]}``), ``base`` / ``post``
        = ``{"score", "rank", "loss"}``, ``loss`` the optimizer's loss of each step in step
        order (:attr:`trace`).  No post-training runs for the sake of a trace: a base result
        cached without one reports ``"loss": None``."""
        old = self._trace
        self._trace = True
        try:
            rels = self.compute_relevance_batch(pred, rules)
        finally:
            self._trace = old
        return [self._tr_rule(rel, det) for rel, det in zip(rels, self.last_results)]

    @staticmethod
    def _mk_side(res, epochs):
        """One post-training of a curve report: its target score and rank and its marks
        [{"epoch", "score", "rank"}], None when the result was cached without these marks."""
        marks = res.get("marks")
        if marks is not None and [m["epoch"] for m in marks] != epochs:
            marks = None
        return {"score": res["target_score"], "rank": res["target_rank"],
                "marks": None if marks is None else [dict(m) for m in marks]}

    def _rel_of(self, base, pt):
        """The engine's relevance formula on one (base, post-trained) pair of {"score", "rank"}."""
        raise NotImplementedError

    def _curve(self, base, post):
        """The relevance formula at every mark of a (base, post) pair of _mk_side results."""
        if base["marks"] is None or post["marks"] is None:
            return None
        return [self._rel_of(b, p) for b, p in zip(base["marks"], post["marks"])]

    def _mk_rule(self, relevance, detail, epochs):
        raise NotImplementedError

    def compute_curves(self, pred, rules, epochs):
        """``compute_relevance_batch(pred, rules)`` -- the same schedule, draws, batches and
        relevances, the generators left where it leaves them -- that also reports what every
        post-training had reached after the ``epochs`` (:attr:`marks`): per rule
        ``{"relevance", "epochs", "curve", "base", "post"}`` (the sufficient engine:
        ``{"relevance", "epochs", "curve", "conversions": [{"entity", "base", "post"}, ...]}``
        with a ``curve`` of means), ``base`` / ``post`` = ``{"score", "rank", "marks":
        [{"epoch", "score", "rank"}, ...]}``.  ``curve[j]`` is the engine's own relevance
        formula on the base and post results at mark j: what an engine with ``epochs`` =
        ``epochs[j]`` returns for the same draws per post-training (not the reference started
        with that budget from the same seed, whose later post-trainings draw from elsewhere in
        the stream).  No post-training runs for the sake of a mark: a base result cached
        without these marks reports ``"marks": None`` and a ``curve`` of None.  TypeError /
        ValueError for a bad ``epochs``, before any draw."""
        ep = _lib.check_marks(epochs, int(self._kp_hp.epochs))
        old = self._marks
        self._marks = ep
        try:
            rels = self.compute_relevance_batch(pred, rules)
        finally:
            self._marks = old
        ep = [int(e) for e in ep]
        return [self._mk_rule(rel, det, ep) for rel, det in zip(rels, self.last_results)]

    @staticmethod
    def _mg_side(res, tol):
        """One post-training of a margins report: its target score and rank and its margins,
        None each when the result was cached without margins of this tolerance."""
        mg = res.get("margins")
        if mg is not None and mg["tol"] != tol:
            mg = None
        side = {"score": res["target_score"], "rank": res["target_rank"]}
        for name, _ in _lib.MARGIN_FIELDS:
            side[name] = None if mg is None else mg[name]
        return side

    def _band_of(self, base, pt):
        """(low, high) of the engine's relevance formula in float64 over the rank bands of one
        (base, post-trained) pair of _mg_side results, the score term as computed; None when a
        side has no margins."""
        raise NotImplementedError

    def _score_term(self, base, pt, improvement):
        """The sigmoid term of the relevance formulas, in float64: of the score's improvement
        (the sufficient engine) or worsening (the necessary engine) from base to post."""
        d = float(pt["score"]) - float(base["score"])
        if bool(self.model.is_minimizer()) == bool(improvement):  # smaller is better: an improvement is base - post
            d = -d
        return float(_sigmoid(d))

    def _mg_rule(self, relevance, detail, tol):
        raise NotImplementedError

    def compute_margins(self, pred, rules, tol=1e-4):
        """``compute_relevance_batch(pred, rules)`` -- the same schedule, draws, batches and
        relevances, the generators left where it leaves them -- that also reports how far every
        rank is from changing (:attr:`margin_tol`): per rule ``{"relevance", "relevance_lo",
        "relevance_hi", "base", "post"}`` (the sufficient engine: ``{"relevance",
        "relevance_lo", "relevance_hi", "conversions": [{"entity", "base", "post"}, ...]}``),
        ``base`` / ``post`` = ``{"score", "rank", "rank_lo", "rank_hi", "ties", "gap_better",
        "gap_worse", "id_better", "id_worse"}``.  ``relevance`` is ``compute_relevance_batch``'s
        bit for bit.  ``relevance_lo`` / ``relevance_hi`` are the relevance formula in float64
        over the rank bands: the necessary engine's with ``post.rank_lo - base.rank_hi`` and
        ``post.rank_hi - base.rank_lo``; the sufficient engine's per conversion entity the
        minimum and maximum over the corners (``base.rank``, ``post.rank``) in {lo, hi} x {lo,
        hi} (the formula is monotone in each), then the mean of the lows and the mean of the
        highs.  The band moves the ranks only: the score term stays as computed (a score moved
        by at most delta moves its sigmoid, hence the relevance, by less than delta / 2).  No
        post-training runs for the sake of a margin: a base result cached without margins of
        this ``tol`` reports None for them and for the band.  TypeError / ValueError for a bad
        ``tol`` and NotImplementedError for a combination not offered, before any draw."""
        tol = _lib.check_margin_tol(tol)
        old = self._margin_tol
        self._margin_tol = tol
        try:
            rels = self.compute_relevance_batch(pred, rules)
        finally:
            self._margin_tol = old
        return [self._mg_rule(rel, det, tol) for rel, det in zip(rels, self.last_results)]

    def _at_side(self, res, entity):
        """One post-training of an attributions report: its target score and rank, and (None each
        when the result was cached without attributions) ``delta``, ``score0`` = score - delta
        and its facts ``[{"triple", "fit", "reg"}]`` in the slot's order, the kelpie entity
        written as ``entity``, the entity it clones."""
        at = res.get("attrib")
        side = {"score": res["target_score"], "rank": res["target_rank"], "delta": None, "score0": None, "facts": None}
        if at is not None:
            K = self.dataset.num_entities
            side["delta"] = at["delta"]
            side["score0"] = float(res["target_score"]) - at["delta"]
            side["facts"] = [{"triple": tuple(int(entity) if v == K and k != 1 else v for k, v in enumerate(t)),
                              "fit": f, "reg": r} for t, f, r in zip(at["facts"], at["fit"], at["reg"])]
        return side

    def _at_rule(self, pred, relevance, detail):
        raise NotImplementedError

    def compute_attributions(self, pred, rules):
        """``compute_relevance_batch(pred, rules)`` -- the same schedule, draws, batches and
        relevances, the generators left where it leaves them -- that also reports which of each
        post-training's facts wrote its score (:attr:`attributions`): per rule ``{"relevance",
        "base", "post"}`` (the sufficient engine: ``{"relevance", "conversions": [{"entity",
        "base", "post"}, ...]}``), ``base`` / ``post`` = ``{"score", "rank", "score0", "delta",
        "facts": [{"triple", "fit", "reg"}, ...]}``: the slot's facts (the subject's, or the
        conversion entity's, after the rule's edit) in original ids, what fitting each one added
        to the target score over the post-training, the regulariser's share booked to it, and
        ``score0 + delta == score``.  No post-training runs for the sake of an attribution: a
        base result cached without them reports None.  NotImplementedError for a combination not
        offered, before any draw."""
        old = self._attrib
        self._attrib = True
        try:
            rels = self.compute_relevance_batch(pred, rules)
        finally:
            self._attrib = old
        return [self._at_rule(pred, rel, det) for rel, det in zip(rels, self.last_results)]

    def _schedule_multi(self, items, checkpoints):
        raise NotImplementedError

    def _finalize_multi(self, slots, pending, jobs):
        raise NotImplementedError

    def _multi(self, items, checkpoints=None):
        t0 = time.perf_counter()
        self._deferred_error = None
        with self.rng.deferred():
            slots, pending, jobs = self._schedule_all(items, checkpoints)
        t_sched = time.perf_counter() - t0
        self._run(slots)
        self._collect(slots, self.last_batch_stats)
        self.last_batch_stats["schedule_s"] = t_sched
        outs = self._finalize_multi(slots, pending, jobs)
        self._raise_deferred(slots, pending)
        return outs

    def _batch_items(self, pred, rules):
        """compute_relevance_batch's one-item batch (the sufficient engine adds its
        conversion entities)."""
        return [(pred, rules)]

    def submit_batch(self, pred, rules, checkpoints: list | None = None, hold=False):
        """The first half of ``compute_relevance_batch``: schedule the rules' reference-order
        draws on this thread (with ``checkpoints`` as there) and start their device work on
        the next of two pipeline contexts, without waiting; :meth:`finish_batch` returns the
        relevances.  A later submit may be scheduled while this batch runs -- the
        builder's next speculative window (kelpie_amd/builder.py) -- and rewinding the
        generators to one of this batch's checkpoints undoes both.

        ``hold``: the batch's draws wait and its slots are packed on the batch thread, but
        its library call waits for :meth:`release_batch` (or :meth:`finish_batch`); a
        ``finish_batch(discard=True)`` before that cancels it without any device work."""
        import threading

        from . import rng as _rng_mod
        self._refuse_keyed("submit_batch")
        self._refuse_margins("submit_batch")
        self._refuse_attrib("submit_batch")
        ctxs = self.model.contexts(2)
        self._submit_n = getattr(self, "_submit_n", -1) + 1
        ctx = ctxs[self._submit_n % len(ctxs)]
        busy = getattr(self, "_ctx_last", {}).get(id(ctx))
        if busy is not None:
            busy["thread"].join()  # a context runs one batch at a time (one context: no overlap)
        self._deferred_error = None
        with self.rng.deferred(detach=True) as d:
            slots, pending, jobs = self._schedule_all(self._batch_items(pred, rules), checkpoints)
        st = {"slots": slots, "pending": pending, "jobs": jobs, "deferred": self._deferred_error,
              "ticket": d.last_ticket, "error": None, "stats": None, "go": threading.Event(), "cancel": False}
        self._deferred_error = None
        if not hold:
            st["go"].set()

        def gate():
            st["go"].wait()
            return not st["cancel"]

        def run():
            try:
                _rng_mod.wait_ticket(st["ticket"])
                stats = self._run(slots, ctx=ctx, gate=gate)
                st["stats"] = dict(stats) if stats is not None else None
            except BaseException as e:  # re-raised by finish_batch
                st["error"] = e

        st["thread"] = threading.Thread(target=run, daemon=True)
        st["thread"].start()
        self._ctx_last = {**getattr(self, "_ctx_last", {}), id(ctx): st}
        return st

    def release_batch(self, st):
        """Let a held :meth:`submit_batch` batch start its device work."""
        st["go"].set()

    def finish_batch(self, st, discard=False):
        """Wait for a :meth:`submit_batch` batch and return its relevances (``discard``: only
        wait -- a speculative window the builder does not use -- and return None; a held
        batch not yet released is cancelled instead, with no device work)."""
        if discard and not st["go"].is_set():
            st["cancel"] = True
        st["go"].set()
        st["thread"].join()
        if discard:
            return None
        if st["error"] is not None:
            raise st["error"]
        self._collect(st["slots"], st["stats"])
        outs = self._finalize_multi(st["slots"], st["pending"], st["jobs"])
        self._deferred_error = st["deferred"]
        self._raise_deferred(st["slots"], st["pending"])
        return outs[0]

    def _raise_deferred(self, slots, pending):
        """Re-raise the reference's error of a call the batch stopped at, after caching
        the base post-training it had already run (post_training_engine.py:46-62)."""
        err, self._deferred_error = getattr(self, "_deferred_error", None), None
        if err is None:
            return
        for key, i in pending.items():
            self.base_pt_results.setdefault(key, slots[i].result)
        raise err

    def warm_contexts(self, items, depth=None):
        """Run the batch ``items`` once on every extra pipeline context, so their
        workspaces are allocated and the attention table image is built outside a
        timed region.  Consumes no random draws: the generator states are restored."""
        import os
        if depth is None:
            depth = int(os.environ.get("KELPIE_PIPELINE_DEPTH", "2"))
        ctxs = self.model.contexts(max(1, depth))
        if len(ctxs) < 2:
            return
        cp = StateCheckpoint()
        try:
            self.set_cache()
            self._deferred_error = None
            with self.rng.deferred():
                slots, _, _ = self._schedule_all(items, None)
            self._deferred_error = None
            for ctx in ctxs[1:]:
                st = self._run(slots, ctx=ctx)
                # a warm-up has no gather (_collect), so a sharded run's captured device
                # error is raised here (each rank warms the slots it owns)
                local = st.get("_local") if st else None
                if local is not None and local[4] is not None:
                    raise local[4]
        finally:
            cp.restore()
            self.set_cache()

    def compute_relevance_pipeline(self, batches, depth=None):
        """Equivalent to ``[(self.set_cache(), self.compute_relevance_multi(b))[1] for b in batches]``
        but the host schedules batch k+1 (its reference-order random draws and
        slot assembly) while batch k runs on the device: the library call
        releases the GIL.  Draw order is unchanged because scheduling stays
        sequential on this thread; each batch starts from a cleared cache, so no
        batch's schedule depends on another's results.  ``last_batch_stats`` is
        a list of the per-batch stats.

        With ``depth`` > 1 (default ``KELPIE_PIPELINE_DEPTH``, else 2) up to that many
        batches are in flight, each on its own device context
        (``FrozenModel.contexts``: own stream and workspaces over a replica of the
        frozen tables), so one batch's library-side planning, uploads and result
        download overlap the other's kernels instead of leaving the device idle.  A batch
        with a predecessor and a successor in this call tells its context that ``depth``
        batches share the device (``kp_ctx_set_inflight``: the attention then cuts its query
        tiles into fewer key ranges); the first and last batch, which run partly alone, and
        every other path leave the hint at 1."""
        import collections
        import os
        import threading

        self._refuse_keyed("compute_relevance_pipeline")
        self._refuse_margins("compute_relevance_pipeline")
        self._refuse_attrib("compute_relevance_pipeline")
        if self._fp64():  # before any draw
            raise NotImplementedError("precision='fp64' on compute_relevance_pipeline: the fp64 path runs one "
                                      "batch at a time")
        if depth is None:
            depth = int(os.environ.get("KELPIE_PIPELINE_DEPTH", "2"))
        ctxs = self.model.contexts(max(1, depth))
        # The scheduling thread and the batch threads' packing share the interpreter lock;
        # KELPIE_GIL_SWITCH_US shortens the interpreter's switch interval while the
        # pipeline runs (A/B switch; unset: the interpreter's default)
        import gc
        import sys
        # no cyclic garbage collection while batches are in flight (KELPIE_PIPELINE_NOGC=0
        # keeps it): a collection pass on the scheduling thread holds the interpreter lock
        # for milliseconds while the batch threads wait to pack and launch (headline +1.5 %,
        # three alternating pairs on one box, profiles/r04q/); the objects are freed by
        # reference counting either way, and collection resumes when the call returns
        nogc = os.environ.get("KELPIE_PIPELINE_NOGC", "1") == "1" and gc.isenabled()
        if nogc:
            gc.disable()
        old_switch = sys.getswitchinterval()
        if os.environ.get("KELPIE_GIL_SWITCH_US"):
            sys.setswitchinterval(float(os.environ["KELPIE_GIL_SWITCH_US"]) * 1e-6)

        from . import rng as _rng_mod

        # KELPIE_PIPELINE_TRACE=<path>: a JSON list of (seconds, event, batch) per pipeline
        # stage, for host timelines (diagnostics; tools/pipeline_trace.py)
        trace_path = os.environ.get("KELPIE_PIPELINE_TRACE")
        trace = [] if trace_path else None

        def tr(ev, b):
            if trace is not None:
                trace.append((time.perf_counter(), ev, b))

        # one long-lived worker thread per device context, fed through a queue: starting a
        # batch is a put, not a thread start (Thread.start waits for the new thread to run:
        # ~0.4 ms of the scheduling thread per TransE batch, trace r05r)
        import queue as _queue

        class _Worker:
            def __init__(self):
                self.q = _queue.SimpleQueue()
                self.t = threading.Thread(target=self._loop, daemon=True)
                self.t.start()

            def _loop(self):
                while True:
                    st = self.q.get()
                    if st is None:
                        return
                    try:
                        run(st)
                    finally:
                        st["done"].set()

        class _Handle:  # Thread's join / is_alive over a worker's queued batch
            def __init__(self, worker, st):
                self.ev = st["done"] = threading.Event()
                worker.q.put(st)

            def join(self):
                self.ev.wait()

            def is_alive(self):
                return not self.ev.is_set()

        workers = {}
        use_workers = os.environ.get("KELPIE_PIPELINE_WORKERS", "1") == "1"

        def run(state):
            try:
                b = state["b"]
                tr("run", b)
                # this batch's deferred draws (the scheduling thread did not wait for them)
                _rng_mod.wait_ticket(state.get("ticket"))
                tr("draws", b)
                # the attention planner's hint (kp_ctx_set_inflight): a batch between two others
                # of this call shares the device with depth - 1 of them from start to end
                hint = state.get("inflight", 1)
                if hint > 1 and hasattr(state["ctx"], "set_inflight"):
                    state["ctx"].set_inflight(hint)
                    try:
                        state["stats"] = dict(self._run(state["slots"], ctx=state["ctx"]))
                    finally:
                        state["ctx"].set_inflight(1)
                else:
                    state["stats"] = dict(self._run(state["slots"], ctx=state["ctx"]))
                tr("ran", b)
            except BaseException as e:  # re-raised on the scheduling thread
                state["error"] = e

        tr("enter", -1)
        outs, stats, inflight = [], [], collections.deque()
        late_collect = os.environ.get("KELPIE_PIPELINE_EARLY_START", "1") == "0"  # A/B: collect, then start
        detach = os.environ.get("KELPIE_PIPELINE_DETACH", "1") == "1"

        def finish(state):
            state["thread"].join()
            tr("finish", state["b"])
            if state.get("error") is not None:
                raise state["error"]
            self.base_pt_results = {}
            self._collect(state["slots"], state["stats"])
            o = self._finalize_multi(state["slots"], state["pending"], state["jobs"])
            st = state["stats"]
            st["schedule_s"] = state["schedule_s"]
            stats.append(st)
            outs.append(o)
            self._deferred_error = state.get("deferred")
            tr("finished", state["b"])
            self._raise_deferred(state["slots"], state["pending"])

        # KELPIE_PIPELINE_LOOKAHEAD=N: batches scheduled ahead of the contexts, so that a freed
        # context starts the next batch at once instead of after that batch's schedule (the
        # headline trace r05n shows a context idle ~3 ms while the next batch was scheduled).
        # Measured, alternating on one box (profiles/r05/r05w/): 1 against 0, headline
        # 868 / 878 / 875 vs 884 / 894 / 891 cand/s, ConvE 454 / 456 vs 456 / 457; default 0
        # (each batch scheduled when the previous one has started)
        lookahead = max(0, int(os.environ.get("KELPIE_PIPELINE_LOOKAHEAD", "0")))
        ready = collections.deque()
        todo = iter(enumerate(batches))
        n_batches = len(batches) if hasattr(batches, "__len__") else None  # unknown: no batch is "between"
        stop = False

        def schedule_next():
            """Schedule the next batch into `ready`; False when there is none."""
            nonlocal stop
            nxt = next(todo, None)
            if nxt is None:
                stop = True
                return False
            b, items = nxt
            self.set_cache()
            t0 = time.perf_counter()
            tr("schedule", b)
            self._deferred_error = None
            # detached: the next batch is scheduled while the workers still make this
            # one's draws (TransE: the sequential numpy chain); the batch thread waits
            # for them before packing (KELPIE_PIPELINE_DETACH=0: wait here, A/B)
            with self.rng.deferred(detach=detach) as drng:
                slots, pending, jobs = self._schedule_all(items, None)
            err, self._deferred_error = self._deferred_error, None
            tr("scheduled", b)
            ready.append({"slots": slots, "pending": pending, "jobs": jobs,
                          "schedule_s": time.perf_counter() - t0, "error": None, "deferred": err,
                          "ticket": drng.last_ticket, "b": b})
            if err is not None:
                stop = True  # the sequential reference stops at the failing call
            return True

        def start_next(done):
            """Start the oldest ready batch on its context (batch b uses context b % depth:
            the batch before it there is in `done` or was finished earlier), then collect
            the finished ones: their collection (and the gather, sharded) runs while the
            new batch packs and launches instead of ahead of it."""
            if late_collect or any(d.get("error") is not None for d in done):
                for d in done:
                    finish(d)  # raises the first device failure before the next batch starts
                done = []
            state = ready.popleft()
            state["ctx"] = ctxs[state["b"] % len(ctxs)]
            state["inflight"] = len(ctxs) if n_batches is not None and 0 < state["b"] < n_batches - 1 else 1
            ci = state["b"] % len(ctxs)
            if not use_workers:  # KELPIE_PIPELINE_WORKERS=0: a thread per batch (A/B)
                state["thread"] = threading.Thread(target=run, args=(state,), daemon=True)
                state["thread"].start()
            else:
                if ci not in workers:
                    workers[ci] = _Worker()
                state["thread"] = _Handle(workers[ci], state)
            inflight.append(state)
            for d in done:
                finish(d)

        def join_oldest():
            old = inflight.popleft()
            old["thread"].join()
            tr("joined", old["b"])
            return old

        try:
            while True:
                if ready and (len(inflight) < len(ctxs) or not inflight[0]["thread"].is_alive()):
                    start_next([join_oldest()] if len(inflight) >= len(ctxs) else [])
                elif not stop and len(ready) <= lookahead:
                    schedule_next()
                elif ready:
                    start_next([join_oldest()])  # scheduled far enough ahead: wait for a context
                else:
                    break
            while inflight:
                finish(inflight.popleft())
        finally:
            for st in inflight:  # an earlier batch raised: let the others' device work end
                st["thread"].join()
            for w in workers.values():
                w.q.put(None)
            sys.setswitchinterval(old_switch)
            if nogc:
                gc.enable()
            tr("unwound", -1)
            if sys.exc_info()[0] is None:
                _rng_mod.sync()  # the generators are current again when the call returns
            else:
                try:
                    _rng_mod.sync()
                except Exception:  # noqa: BLE001 -- the error in flight is the one to report
                    pass
            tr("exit", -1)
            if trace is not None:
                import json
                with open(trace_path, "a") as f:
                    f.write(json.dumps(trace) + "\n")
        self.last_batch_stats = stats
        return outs


class NecessaryPostTrainingEngine(PostTrainingEngine):
    """post_training_engine.py:128-157."""

    def compute_relevance_batch(self, pred, rules, checkpoints: list | None = None):
        """Relevances of ``rules`` for ``pred``, identical to calling
        ``compute_relevance`` on each rule in order.  When ``checkpoints`` is a
        list, the generator state after each rule's draws is appended to it."""
        return self.compute_relevance_multi([(pred, rules)], checkpoints)[0]

    def compute_relevance_multi(self, items, checkpoints: list | None = None):
        """[(pred, rules), ...] -> [[relevance per rule], ...] in ONE device batch;
        equal to the sequential compute_relevance calls in that order."""
        return self._multi(items, checkpoints)

    def _calls(self, items):
        """(pred, rule, mode) of every call _schedule_multi makes, in order."""
        for pred, rules in items:
            for rule in rules:
                yield pred, [tuple(t) for t in rule], "necessary"
                if not rule:
                    return

    def _schedule_multi(self, items, checkpoints):
        slots, pending, jobs = [], {}, []
        fast = checkpoints is None and getattr(self.model, "fused_call_draws", False) and not self._keyed()
        for pred, rules in items:
            self._cur_probes = self._probes_of(pred)
            if fast and all(len(r) for r in rules):
                jobs.append(self._schedule_fused_pred(pred, rules, "necessary", slots, pending))
                continue
            pj = []
            for rule in rules:
                rule = [tuple(t) for t in rule]
                idx = self._schedule(pred, rule, "necessary", slots, pending)
                if not rule:
                    # KelpieDataset.undo_removal raises after the post-training
                    # (kelpie_dataset.py:166-167): its draws are spent, nothing after it runs
                    self._deferred_error = Exception("No removal to undo.")
                    jobs.append(pj)
                    return slots, pending, jobs
                pj.append(idx)
                if checkpoints is not None:
                    self._flush_fused()
                    checkpoints.append(StateCheckpoint())
            jobs.append(pj)
        return slots, pending, jobs

    def _finalize_multi(self, slots, pending, jobs):
        minimizer = self.model.is_minimizer()
        outs = []
        self.last_results = []
        rank_w, sig_w, lens = [], [], []
        for pj in jobs:
            lens.append(len(pj))
            for pt_idx, key in pj:
                base = self._base_result(key, slots, pending)
                pt = slots[pt_idx].result
                rank_w.append(pt["target_rank"] - base["target_rank"])
                if minimizer:
                    score_worsening = pt["target_score"] - base["target_score"]
                else:
                    score_worsening = base["target_score"] - pt["target_score"]
                sig_w.append(_sigmoid(score_worsening))
                self.last_results.append((pt, base))
        # int64 tensor + python float -> float32 tensor (A-Q5): one float32 add per call,
        # element-wise over the batch (the same bits as the scalar form)
        if self._fp64():  # the fp64 reference's default dtype is float64: no float32 add
            rel = (np.asarray(rank_w, np.int64).astype(np.float64) + np.asarray(sig_w, np.float64)).tolist()
        else:
            rel = (np.asarray(rank_w, np.int64).astype(np.float32)
                   + np.asarray(sig_w, np.float64).astype(np.float32)).tolist()
        k = 0
        for n in lens:
            outs.append(rel[k:k + n])
            k += n
        return outs


    def _cf_rule(self, relevance, detail, k):
        pt, base = detail
        return {"relevance": relevance, "base": self._cf_side(base, k), "post": self._cf_side(pt, k)}

    def _se_rule(self, relevance, detail):
        pt, base = detail
        return {"relevance": relevance, "base": self._se_side(base), "post": self._se_side(pt)}

    def _tr_rule(self, relevance, detail):
        pt, base = detail
        return {"relevance": relevance, "base": self._tr_side(base), "post": self._tr_side(pt)}

    def _at_rule(self, pred, relevance, detail):
        pt, base = detail
        s = int(pred[0])
        return {"relevance": relevance, "base": self._at_side(base, s), "post": self._at_side(pt, s)}

    def rank_facts(self, pred, k=None):
        """The subject's facts by what fitting them contributed to ``pred``'s score in its base
        post-training (:attr:`attributions`), largest first: ``[{"triple", "fit", "reg"}, ...]``,
        the first ``k`` (None: all).  A model-aware ordering of the candidates beside the
        topological prefilters', from the one post-training every explanation of ``pred`` runs
        anyway.  The base slot runs alone.  With reference draws it takes its draws as a base
        post-training does and puts the generators back where they were: like
        ``compute_relevance_batch(pred, [])`` the call leaves them unchanged, so the result
        depends on their state but later calls do not depend on this one.  With keyed draws it
        asks the generators for nothing and is the base of every keyed relevance of ``pred``.  A
        cached base result with attributions is reused; the result of this call is not cached.
        NotImplementedError for a combination not offered, before any draw."""
        if k is not None and (isinstance(k, bool) or int(k) != k or int(k) < 0):
            raise ValueError(f"k must be a non-negative integer or None, got {k!r}")
        pred = tuple(int(v) for v in pred)
        old = self._attrib
        self._attrib = True
        try:
            self._refuse_keyed()
            self._refuse_margins()
            self._refuse_attrib(items=[(pred, [])])
            self._refuse_fp64()
            res = self.base_pt_results.get(pred)
            if res is None or res.get("attrib") is None:
                res = self._base_alone(pred)
        finally:
            self._attrib = old
        facts = self._at_side(res, pred[0])["facts"]
        order = sorted(range(len(facts)), key=lambda i: (-facts[i]["fit"], i))
        return [facts[i] for i in (order if k is None else order[:int(k)])]

    def _base_alone(self, pred):
        """The base post-training of ``pred`` in a batch of its own; the torch / numpy generators
        end where they began."""
        view = self._get_kelpie_dataset(pred[0])
        kp = tuple(int(v) for v in view.as_kelpie_triple(pred))
        filt = list(view.filter_for(kp[1]))
        if self._keyed():
            slot = _Slot(x0=None, rows=view.base_rows, rng=None, pred=kp, filt=filt,
                         keys=(_keyed.init_key(self._seed, pred),
                               _keyed.slot_key(self._seed, pred, _keyed.ROLE_BASE, "necessary")))
            self._run([slot])
            return slot.result
        before = StateCheckpoint()
        try:
            with self.rng.deferred():
                init = self.rng.rand_init(self.model.dimension)
                slot = self._slot(self.model.kelpie_init(init, self.rng), view.base_rows, kp, filt)
            self._run([slot])
        finally:
            before.restore()
        return slot.result

    def _rel_of(self, base, pt):
        # _finalize_multi's formula, in its scalar form (the same bits)
        if self.model.is_minimizer():
            score_worsening = pt["score"] - base["score"]
        else:
            score_worsening = base["score"] - pt["score"]
        if self._fp64():
            return float(pt["rank"] - base["rank"]) + _sigmoid(score_worsening)
        return float(np.float32(pt["rank"] - base["rank"]) + np.float32(_sigmoid(score_worsening)))

    def _mk_rule(self, relevance, detail, epochs):
        pt, base = detail
        b, p = self._mk_side(base, epochs), self._mk_side(pt, epochs)
        return {"relevance": relevance, "epochs": list(epochs), "curve": self._curve(b, p), "base": b, "post": p}

    def _band_of(self, base, pt):
        if base["rank_lo"] is None or pt["rank_lo"] is None:
            return None
        sig = self._score_term(base, pt, improvement=False)
        return (float(pt["rank_lo"] - base["rank_hi"]) + sig, float(pt["rank_hi"] - base["rank_lo"]) + sig)

    def _mg_rule(self, relevance, detail, tol):
        pt, base = detail
        b, p = self._mg_side(base, tol), self._mg_side(pt, tol)
        band = self._band_of(b, p) or (None, None)
        return {"relevance": relevance, "relevance_lo": band[0], "relevance_hi": band[1], "base": b, "post": p}


class SufficientPostTrainingEngine(PostTrainingEngine):
    """post_training_engine.py:160-207."""

    def _cf_rule(self, relevance, detail, k):
        # one (post-trained, base) pair per conversion entity, in entities_to_convert's order
        return {"relevance": relevance,
                "conversions": [{"entity": int(e), "base": self._cf_side(base, k), "post": self._cf_side(pt, k)}
                                for e, (pt, base) in zip(self.entities_to_convert, detail)]}

    def _se_rule(self, relevance, detail):
        return {"relevance": relevance,
                "conversions": [{"entity": int(e), "base": self._se_side(base), "post": self._se_side(pt)}
                                for e, (pt, base) in zip(self.entities_to_convert, detail)]}

    def _tr_rule(self, relevance, detail):
        return {"relevance": relevance,
                "conversions": [{"entity": int(e), "base": self._tr_side(base), "post": self._tr_side(pt)}
                                for e, (pt, base) in zip(self.entities_to_convert, detail)]}

    def _at_rule(self, pred, relevance, detail):
        return {"relevance": relevance,
                "conversions": [{"entity": int(e), "base": self._at_side(base, e), "post": self._at_side(pt, e)}
                                for e, (pt, base) in zip(self.entities_to_convert, detail)]}

    def _rel_of(self, base, pt):
        # _finalize_multi's formula for one conversion entity
        rank_improvement = base["rank"] - pt["rank"]
        if self.model.is_minimizer():
            score_improvement = base["score"] - pt["score"]
        else:
            score_improvement = pt["score"] - base["score"]
        if self._fp64():
            rel = float(rank_improvement) + _sigmoid(score_improvement)
        else:
            rel = float(np.float32(np.float32(rank_improvement) + np.float32(_sigmoid(score_improvement))))
        return rel / float(base["rank"])

    def _mk_rule(self, relevance, detail, epochs):
        conv = [{"entity": int(e), "base": self._mk_side(base, epochs), "post": self._mk_side(pt, epochs)}
                for e, (pt, base) in zip(self.entities_to_convert, detail)]
        curves = [self._curve(c["base"], c["post"]) for c in conv]
        curve = None
        if curves and all(c is not None for c in curves):  # the mean over the conversions, as the relevance
            curve = [sum(c[j] for c in curves) / len(curves) for j in range(len(epochs))]
        return {"relevance": relevance, "epochs": list(epochs), "curve": curve, "conversions": conv}

    def _band_of(self, base, pt):
        if base["rank_lo"] is None or pt["rank_lo"] is None:
            return None
        sig = np.float64(self._score_term(base, pt, improvement=True))
        with np.errstate(all="ignore"):  # a base rank of 0 divides by zero, as the relevance itself does
            corners = [float((np.float64(b - p) + sig) / np.float64(b))
                       for b in (base["rank_lo"], base["rank_hi"]) for p in (pt["rank_lo"], pt["rank_hi"])]
        return min(corners), max(corners)

    def _mg_rule(self, relevance, detail, tol):
        conv = [{"entity": int(e), "base": self._mg_side(base, tol), "post": self._mg_side(pt, tol)}
                for e, (pt, base) in zip(self.entities_to_convert, detail)]
        bands = [self._band_of(c["base"], c["post"]) for c in conv]
        lo = hi = None
        if bands and all(b is not None for b in bands):  # the mean over the conversions, as the relevance
            lo, hi = sum(b[0] for b in bands) / len(bands), sum(b[1] for b in bands) / len(bands)
        return {"relevance": relevance, "relevance_lo": lo, "relevance_hi": hi, "conversions": conv}

    def __init__(self, model, dataset, hp, rng=None):
        super().__init__(model, dataset, hp, rng)
        self.entities_to_convert = []

    def compute_relevance_batch(self, pred, rules, checkpoints: list | None = None):
        return self.compute_relevance_multi([(pred, rules, self.entities_to_convert)], checkpoints)[0]

    def _batch_items(self, pred, rules):
        return [(pred, rules, self.entities_to_convert)]

    def compute_relevance_multi(self, items, checkpoints: list | None = None):
        """[(pred, rules, entities_to_convert), ...] in ONE device batch."""
        return self._multi(items, checkpoints)

    def _calls(self, items):
        """(pred, rule, mode) of every call _schedule_multi makes, in order."""
        for pred, rules, ents in items:
            pred = tuple(int(v) for v in pred)
            s = pred[0]
            for rule in rules:
                if not ents:
                    return
                for e in ents:
                    crule = Dataset.replace_entity_in_triples([tuple(t) for t in rule], s, e)
                    yield Dataset.replace_entity_in_triple(pred, s, e), crule, "sufficient"
                    if not crule:
                        return

    def _schedule_multi(self, items, checkpoints):
        slots, pending, jobs = [], {}, []
        for pred, rules, ents in items:
            pred = tuple(int(v) for v in pred)
            s = pred[0]
            self._cur_probes = self._probes_of(pred)
            pj = []
            for rule in rules:
                if not ents:
                    self._deferred_error = ZeroDivisionError("division by zero")  # sum([]) / len([])
                    jobs.append(pj)
                    return slots, pending, jobs
                rj = []
                for e in ents:
                    crule = Dataset.replace_entity_in_triples([tuple(t) for t in rule], s, e)
                    cpred = Dataset.replace_entity_in_triple(pred, s, e)
                    rj.append(self._schedule(cpred, crule, "sufficient", slots, pending))
                    if not crule:
                        # KelpieDataset.undo_addition raises after the first conversion's
                        # post-training (kelpie_dataset.py:191-192)
                        self._deferred_error = Exception("No addition to undo.")
                        jobs.append(pj)
                        return slots, pending, jobs
                pj.append(rj)
                if checkpoints is not None:
                    self._flush_fused()
                    checkpoints.append(StateCheckpoint())
            jobs.append(pj)
        return slots, pending, jobs

    def _finalize_multi(self, slots, pending, jobs):
        minimizer = self.model.is_minimizer()
        outs = []
        self.last_results = []
        for pj in jobs:
            out = []
            for rj in pj:
                rels, det = [], []
                for pt_idx, key in rj:
                    base = self._base_result(key, slots, pending)
                    pt = slots[pt_idx].result
                    det.append((pt, base))
                    rank_improvement = base["target_rank"] - pt["target_rank"]
                    if minimizer:
                        score_improvement = base["target_score"] - pt["target_score"]
                    else:
                        score_improvement = pt["target_score"] - base["target_score"]
                    if self._fp64():  # the fp64 reference's default dtype is float64: no float32 add
                        rel = float(rank_improvement) + _sigmoid(score_improvement)
                    else:
                        rel = float(np.float32(np.float32(rank_improvement) + np.float32(_sigmoid(score_improvement))))
                    rel /= float(base["target_rank"])
                    rels.append(rel)
                self.last_results.append(det)
                out.append(sum(rels) / len(rels))
            outs.append(out)
        return outs
