// kp_posttrain.hpp -- the host work the three *_posttrain_rank functions share: the check of
// the batch and of the request (require_request), Adam's step scalars, the kelpie rows'
// padding, the rank rows (kp_common.hpp's RankSet: the slots, the probes and the mark rows are
// each one set, built by one upload, upload_rank_rows, and ranked by one chunked count,
// rank_rows, on the family's one query callable), the trace's offsets and losses (TraceDev),
// the download of every result and the hot-launch timing.  The model-specific step planning is
// pure host code in headers of its own (kp_cx_plan.hpp: ComplEx / DistMult; kp_cv_plan.hpp:
// ConvE; TransE's schedule is kp_sched.cpp), as are the request's checks and its expansion into
// rank rows (kp_batch_check.hpp, kp_probe_check.hpp, kp_trace_check.hpp, kp_marks_check.hpp,
// kp_margins_check.hpp); the launches, and where in the call each upload happens, stay in
// kp_complex.hip / kp_transe.hip / kp_conve.hip.
#pragma once

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "kp_attrib_check.hpp"
#include "kp_batch_check.hpp"
#include "kp_common.hpp"
#include "kp_keyed.hpp"
#include "kp_margins_check.hpp"
#include "kp_marks_check.hpp"
#include "kp_probe_check.hpp"
#include "kp_trace_check.hpp"

// KP_HOST_TIMES=1 (diagnostic): ComplEx and ConvE print, per call on stderr, the host time
// of their phases (planning, uploads, enqueueing the loop, waiting for the device)
inline const bool g_host_times = std::getenv("KP_HOST_TIMES") != nullptr;
inline double host_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The checks of a call, first thing in every *_posttrain_rank, so that a malformed call
// leaves no device work in flight; the first rule broken is the one reported, as KP_EINVAL
// under the model's name: the batch (kp_batch_check.hpp), the top-k request, the probes
// (kp_probe_check.hpp), the trace (kp_trace_check.hpp), the marks (kp_marks_check.hpp), the
// margins (kp_margins_check.hpp), the attributions (kp_attrib_check.hpp).
// `rank64`: the call ranks on launch_rank_f64's fp64 operands; the lists, the probes and the
// marks need them (KP_ENOTSUP under the fp32 diagnostic ranks, KP_TE_RANK / KP_CV_RANK = f32,
// once well formed), the trace does not depend on the rank.
// A batch without slots (kp_api.hip, which then calls no family; rank64 = true) has nothing
// to check a list or a probe against: k and the probe count are refused under the entry
// points' names, the trace and the marks by their own rules.
inline void require_request(const kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq, bool rank64,
                            const char* model) {
  const std::string who = model;
  if (bt->n_slots == 0) {
    KP_REQUIRE(rq.k >= 0 && rq.k <= 32, "kp_posttrain_rank_topk: k must be in [0, 32]");
    KP_REQUIRE(rq.n_probes() == 0, "kp_posttrain_rank_probes: probes without a slot");
    KP_REQUIRE(!rq.keyed || rq.keyed->n_slots == 0, who + ": keyed draws: n_slots differs from the batch's");
  } else {
    if (const char* why = kp_check_batch(c->n_ent, c->n_rel2, c->dim, bt)) throw KpError{KP_EINVAL, who + ": " + why};
    if (rq.keyed) {  // an armed call: the keyed request, before any device work (kp_keyed.hpp)
      int code = KP_EINVAL;
      if (const char* why = kp_check_keyed(c->model, hp, bt->n_slots, bt->row_off, rq.keyed, &code))
        throw KpError{code, who + ": keyed draws: " + why};
    }
    if (rq.f64) {  // kp_posttrain_rank_f64: its buffers, then the family, then what it does not offer yet
      KP_REQUIRE(rq.f64->x0 && rq.f64->out_score, who + ": fp64: missing x0 or out_score");
      if (c->model != KP_MODEL_COMPLEX && c->model != KP_MODEL_DISTMULT)
        throw KpError{KP_ENOTSUP, who + ": fp64 post-training serves ComplEx and DistMult only"};
      if (rq.k != 0 || rq.n_probes() > 0 || rq.trace || rq.marks)
        throw KpError{KP_ENOTSUP, who + ": fp64: top-k, probes, trace and marks are not offered"};
    }
    KP_REQUIRE(rq.k >= 0 && rq.k <= 32, who + ": top-k: k must be in [0, 32]");
    KP_REQUIRE(rq.k == 0 || (rq.ids && rq.scores), who + ": top-k: missing output");
    if (rq.k > 0 && !rank64)
      throw KpError{KP_ENOTSUP, who + ": top-k needs the fp64 rank (the fp32 rank switch is set)"};
    if (rq.probes) {
      if (const char* why = kp_check_probes(c->n_ent, c->n_rel2, bt->n_slots, rq.probes))
        throw KpError{KP_EINVAL, who + ": probes: " + why};
      if (rq.probes->n > 0 && !rank64)
        throw KpError{KP_ENOTSUP, who + ": probes need the fp64 rank (the fp32 rank switch is set)"};
    }
    // ConvE refuses its hyper-parameters here, ahead of the trace's own batch_size rule
    // (ComplEx / DistMult refuse theirs before this function, TransE after it)
    if (c->model == KP_MODEL_CONVE)
      KP_REQUIRE(hp->batch_size >= 1 && hp->epochs >= 0, "ConvE: bad hyper-parameters");
  }
  if (rq.trace)
    if (const char* why = kp_check_trace(c->model, hp, bt->n_slots, bt->row_off, bt->rows, rq.trace))
      throw KpError{KP_EINVAL, who + ": trace: " + why};
  if (rq.marks) {
    if (const char* why = kp_check_marks(hp, rq.marks)) throw KpError{KP_EINVAL, who + ": marks: " + why};
    if (!rank64) throw KpError{KP_ENOTSUP, who + ": marks need the fp64 rank (the fp32 rank switch is set)"};
  }
  if (rq.margins) {
    int code = KP_EINVAL;
    if (const char* why = kp_check_margins(rq.margins, rq.n_probes(), rq.n_marks(), rank64, &code))
      throw KpError{code, who + ": margins: " + why};
  }
  if (rq.attrib) {
    int code = KP_EINVAL;
    if (const char* why = kp_check_attrib(c->model, hp, c->n_ent, bt->n_slots, bt->row_off, bt->pred, rq.attrib, &code))
      throw KpError{code, who + ": attributions: " + why};
  }
}

// Adam's per-step scalars at step t (0-based) of a call: lr / (1 - beta1^(t+1)) and
// sqrt(1 - beta2^(t+1)), in double and rounded once (CxOpt / CvOpt step_size, bc2_sqrt)
struct AdamStep {
  float step_size, bc2_sqrt;
};
inline AdamStep adam_step(const kp_hp* hp, int t) {
  const double step = (double)(t + 1);
  return {(float)((double)hp->lr / (1.0 - std::pow((double)hp->beta1, step))),
          (float)std::sqrt(1.0 - std::pow((double)hp->beta2, step))};
}

// x0 [ns][dim] zero-padded to [ns][dp] in `xp` (kept by the caller for download_results)
// and uploaded into `b`; with `keyed`, generated there instead (kp_keyed.hip)
inline float* upload_x0(kp_ctx* c, DevBuf& b, const kp_batch* bt, std::vector<float>& xp,
                        const kp_keyed* keyed = nullptr) {
  const int ns = bt->n_slots;
  if (keyed) {  // an armed call: the rows are generated where the upload would land
    xp.assign((size_t)ns * c->dp, 0.f);
    float* dX = ensure_n<float>(b, xp.size());
    keyed_x0_dev(c, keyed, ns, dX);
    return dX;
  }
  xp.assign((size_t)ns * c->dp, 0.f);
  for (int s = 0; s < ns; ++s)
    std::memcpy(&xp[(size_t)s * c->dp], bt->x0 + (size_t)s * c->dim, sizeof(float) * c->dim);
  return upload(c, b, xp.data(), xp.size());
}

// The margins of n rank rows ranked `cap` rows at a launch: every result array [n] in `out`,
// the thresholds and the per-workgroup partials of one launch in `part`.  Sized where the rank
// inputs and the rank rows are sized, never inside the step loop.  Not wanted (or n == 0): an
// empty MarginDev (cap 0).
inline MarginDev margin_buffers(kp_ctx* c, DevBuf& out, DevBuf& part, const kp_margins* m, const kp_margin_out* want,
                                int n, int cap) {
  MarginDev d;
  if (!m || !kp_margin_wanted(*want) || n <= 0) return d;
  d.tol = m->tol;
  d.cap = cap;
  d.nblk = (c->n_ent + 255) / 256;
  char* o = reinterpret_cast<char*>(out.ensure((size_t)n * 48));
  d.rank_lo = reinterpret_cast<int64_t*>(o);
  d.rank_hi = d.rank_lo + n;
  d.ties = d.rank_hi + n;
  d.gap_better = reinterpret_cast<double*>(d.ties + n);
  d.gap_worse = d.gap_better + n;
  d.id_better = reinterpret_cast<int32_t*>(d.gap_worse + n);
  d.id_worse = d.id_better + n;
  const size_t cells = (size_t)cap * d.nblk;
  char* w = reinterpret_cast<char*>(part.ensure((size_t)cap * 16 + cells * 36));
  d.thr = reinterpret_cast<double*>(w);
  d.pkey = reinterpret_cast<unsigned long long*>(d.thr + 2 * (size_t)cap);
  d.pcol = reinterpret_cast<int32_t*>(d.pkey + 2 * cells);
  d.pcnt = d.pcol + 2 * cells;
  return d;
}

// enqueue the download of the margins a caller asked for
inline void download_margins(kp_ctx* c, const MarginDev& d, const kp_margin_out& o, size_t n) {
  if (d.cap == 0) return;
  const auto to_host = [c](void* dst, const void* src, size_t bytes) {
    if (dst) KP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  };
  to_host(o.rank_lo, d.rank_lo, 8 * n);
  to_host(o.rank_hi, d.rank_hi, 8 * n);
  to_host(o.ties, d.ties, 8 * n);
  to_host(o.gap_better, d.gap_better, 8 * n);
  to_host(o.gap_worse, d.gap_worse, 8 * n);
  to_host(o.id_better, d.id_better, 4 * n);
  to_host(o.id_worse, d.id_worse, 4 * n);
}

// What a set of rank rows (kp_common.hpp's RankSet) needs besides its rows:
//   the slots:  row s is (s, p_s, o_s) (kp_slot_rows), X the post-trained kelpie rows;
//   the probes: row r is probe r, (slot, p, o) (kp_probe_rows), X the same rows;
//   the marks:  row s * nm + j is (s * nm + j, p, o) of slot s with the slot's filter list
//               (kp_mark_rows), X the family's mark workspace [ns][nm][dp].
constexpr size_t PROBE_WS_BYTES = (size_t)64 << 20;  // a chunk's query rows and bitmaps, as TOPK_WS_BYTES
constexpr int PROBE_GROUP = 16;                      // kp_rank_f64_count's rows per workgroup row (RQ)
struct RankSetReq {
  // the diagnostic variable that forces the rows per chunk (KP_PROBE_CHUNK, KP_MARKS_CHUNK);
  // nullptr: the set is one chunk (the slots are never chunked)
  const char* chunk_env = nullptr;
  // false (the fp32 diagnostic ranks, KP_TE_RANK / KP_CV_RANK = f32): the inputs and the
  // results only, no fp64 operands and no bitmaps
  bool rank64 = true;
  // ConvE, else 0: what a chunk row's pass through the encoder holds, counted into the chunk's
  // budget; the rows' encoder sources are then uploaded as well, and the chunk's encoder output
  // is `enc_q` (the slots: ConveWs::q, sized by the caller) or, when nullptr, sized here
  size_t enc_row_bytes = 0;
  float* enc_q = nullptr;
  const kp_margins* mg = nullptr;  // kp_posttrain_rank_margins, and which of its outputs are the set's
  const kp_margin_out* mg_want = nullptr;
  int k = 0;  // kp_posttrain_rank_topk (the slots only): the lists' length
};

// Upload a set of rank rows and size every buffer of `ws` it uses.  The caller chooses where in
// its call this happens: an upload's position decides what it overlaps (an upload from pageable
// memory after the step loop waits for the whole loop on the device, so the rank kernels are
// enqueued only then).  The uploads read host vectors that end with the caller: pageable copies
// are staged before hipMemcpyAsync returns.
inline RankSet upload_rank_rows(kp_ctx* c, RankRowsWs& ws, const float* X, const std::vector<int32_t>& trip,
                                const std::vector<int32_t>& po, const int32_t* filt_off, const int32_t* filt,
                                size_t n_filt, const RankSetReq& rq = {}) {
  RankSet d;
  const int n = (int)po.size();
  if (n == 0) return d;
  const int nwords = (c->n_ent + 1 + 31) / 32;
  d.n = d.chunk = n;
  if (rq.chunk_env) {
    const char* a = std::getenv(rq.chunk_env);
    d.chunk = kp_probe_chunk(n, sizeof(double) * c->dp + sizeof(uint32_t) * nwords + rq.enc_row_bytes, PROBE_WS_BYTES,
                             PROBE_GROUP, a ? std::max(0, std::atoi(a)) : 0);
  }
  d.X = X;
  d.rows = upload(c, ws.trip, trip.data(), trip.size());
  d.po = upload(c, ws.po, po.data(), po.size());
  d.filt_off = upload(c, ws.filt_off, filt_off, (size_t)n + 1);
  d.filt = upload(c, ws.filt, filt, n_filt);
  d.target = ensure_n<float>(ws.target, (size_t)n);
  d.rank = ensure_n<int64_t>(ws.rank, (size_t)n);
  if (rq.rank64) {
    d.q = ensure_n<double>(ws.q64, (size_t)d.chunk * c->dp);
    d.t = ensure_n<double>(ws.t64, 2 * (size_t)d.chunk);
    d.kcol = d.t + d.chunk;
    d.bits = ensure_n<uint32_t>(ws.bits, (size_t)d.chunk * nwords);
  }
  if (rq.enc_row_bytes > 0) {
    std::vector<int2> src((size_t)n);
    for (int r = 0; r < n; ++r) src[r] = make_int2(-trip[3 * (size_t)r] - 1, trip[3 * (size_t)r + 1]);
    d.enc_src = upload(c, ws.enc_src, src.data(), src.size());
    d.enc_q = rq.enc_q ? rq.enc_q : ensure_n<float>(ws.enc_q, (size_t)d.chunk * c->dp);
  }
  if (rq.mg) d.mg = margin_buffers(c, ws.mg_out, ws.mg_part, rq.mg, rq.mg_want, n, d.chunk);
  if (rq.k > 0) {
    d.k = rq.k;
    d.top_ids = ensure_n<int32_t>(c->rank.top_ids, (size_t)n * rq.k);
    d.top_scores = ensure_n<float>(c->rank.top_scores, (size_t)n * rq.k);
  }
  return d;
}

// the batch's slots as rank rows on the kelpie rows dX, with the call's lists and margins
// (`ws`: c->rank.slots, or kp_posttrain_rank_f64's c->rank.f64; `sr`: the family's rank64,
// enc_row_bytes and enc_q)
inline RankSet upload_slots(kp_ctx* c, RankRowsWs& ws, const kp_batch* bt, const PostReq& rq, const float* dX,
                            RankSetReq sr = {}) {
  std::vector<int32_t> trip, po;
  kp_slot_rows(bt->n_slots, bt->pred, trip, po);
  sr.k = rq.k;
  sr.mg = rq.margins;
  sr.mg_want = rq.margins ? &rq.margins->slots : nullptr;
  return upload_rank_rows(c, ws, dX, trip, po, bt->filt_off, bt->filt, (size_t)bt->filt_off[bt->n_slots], sr);
}

// the probes as rank rows on the slots' kelpie rows dX
inline RankSet upload_probes(kp_ctx* c, const kp_batch* bt, const PostReq& rq, const float* dX,
                             size_t enc_row_bytes = 0) {
  if (rq.n_probes() == 0) return {};
  std::vector<int32_t> trip, po;
  kp_probe_rows(bt->n_slots, rq.probes, trip, po);
  RankSetReq sr;
  sr.chunk_env = "KP_PROBE_CHUNK";
  sr.enc_row_bytes = enc_row_bytes;
  sr.mg = rq.margins;
  sr.mg_want = rq.margins ? &rq.margins->probes : nullptr;
  return upload_rank_rows(c, c->rank.probes, dX, trip, po, rq.probes->filt_off, rq.probes->filt,
                          (size_t)rq.probes->filt_off[rq.probes->n], sr);
}

// rank a set of rows, chunk by chunk: `queries(d, r0, m)` enqueues the family's query kernel
// for the rows [r0, r0 + m) (their fp64 rows, target and kelpie column scores into d.q / d.t /
// d.kcol), then the count runs over those rows
template <class F>
inline void rank_rows(kp_ctx* c, const RankSet& d, int act, F&& queries) {
  for (int r0 = 0; r0 < d.n; r0 += d.chunk) {
    const int m = std::min(d.chunk, d.n - r0);
    queries(d, r0, m);
    launch_rank_f64(c, d, r0, m, act);
  }
}

// the marks on the device: the mark rows X [ns][nm][dp] in the family's workspace (every row
// the padded x0 until a step captures it), the rows as rank rows, and which step captures which
struct MarksDev {
  int nm = 0;         // marks per slot (0: no marks)
  float* X = nullptr;
  RankSet rows;       // n = ns * nm
  KpMarkPlan plan;
};

// plan the marks, size the mark workspace `ws`, start every mark row as its slot's padded x0
// (dX, already uploaded on the stream) and upload the rank rows; with the call's other
// uploads, ahead of the step loop
inline MarksDev upload_marks(kp_ctx* c, DevBuf& ws, const kp_hp* hp, const kp_batch* bt, const PostReq& rq,
                             const float* dX, size_t enc_row_bytes = 0) {
  MarksDev d;
  if (!rq.marks) return d;
  const int ns = bt->n_slots, nm = rq.marks->n;
  std::vector<int32_t> trip, po, fo, filt;
  const char* why = kp_marks_plan(c->model, hp, ns, bt->row_off, bt->rows, rq.marks, d.plan);
  if (!why) why = kp_mark_rows(ns, nm, bt->pred, bt->filt_off, bt->filt, trip, po, fo, filt);
  if (why) throw KpError{KP_EINVAL, std::string("marks: ") + why};
  d.nm = nm;
  d.X = ensure_n<float>(ws, (size_t)ns * nm * c->dp);
  for (int j = 0; j < nm; ++j)
    KP_HIP(hipMemcpy2DAsync(d.X + (size_t)j * c->dp, sizeof(float) * (size_t)nm * c->dp, dX, sizeof(float) * c->dp,
                            sizeof(float) * c->dp, ns, hipMemcpyDeviceToDevice, c->stream));
  RankSetReq sr;
  sr.chunk_env = "KP_MARKS_CHUNK";
  sr.enc_row_bytes = enc_row_bytes;
  sr.mg = rq.margins;
  sr.mg_want = rq.margins ? &rq.margins->marks : nullptr;
  d.rows = upload_rank_rows(c, c->rank.marks, d.X, trip, po, fo.data(), filt.data(), filt.size(), sr);
  return d;
}

// kp_posttrain_rank_trace's common part on the device (c->rank.tr_*; loss == nullptr: no
// trace): the slots' offsets into the losses and the losses of every step
struct TraceDev {
  int32_t* off = nullptr;  // [ns + 1]
  float* loss = nullptr;   // [total]
  int total = 0;
};
inline TraceDev upload_trace(kp_ctx* c, const kp_batch* bt, const PostReq& rq) {
  TraceDev t;
  if (!rq.trace) return t;
  const int ns = bt->n_slots;
  t.total = rq.trace->trace_off[ns];
  t.off = upload(c, c->rank.tr_off, rq.trace->trace_off, (size_t)ns + 1);
  t.loss = ensure_n<float>(c->rank.tr_loss, (size_t)std::max(1, t.total));
  return t;
}

// per entry of a host-driven step loop's active lists (entry i of step t is slot slot_of(i)):
// the mark row its update also stores, or -1
template <class SlotOf>
inline std::vector<int32_t> marks_act_rows(const MarksDev& d, const std::vector<int>& act_off, int T, SlotOf&& slot_of) {
  std::vector<int32_t> rows(std::max(1, act_off.empty() ? 0 : act_off[T]), -1);
  for (int t = 0; t < T && t < d.plan.T; ++t)
    for (int i = act_off[t]; i < act_off[t + 1]; ++i) rows[i] = kp_marks_row_at(d.plan, slot_of(i), t);
  return rows;
}

// does step t capture a mark row
inline bool marks_at_step(const MarksDev& d, int t) {
  return d.nm > 0 && t < d.plan.T && d.plan.step_off[t + 1] > d.plan.step_off[t];
}

// the tail of a call: enqueue the downloads of the trace's losses, the marks' results, the
// kelpie rows (when out_x is set), the target scores, the ranks, the top-k lists and the
// probes' results (each when asked for), wait for the stream once, unpad the rows into out_x.
// Returns the host time at which the wait began (0 unless KP_HOST_TIMES).
inline double download_results(kp_ctx* c, const kp_batch* bt, const float* dX, const RankSet& r,
                               std::vector<float>& xp, const PostReq& rq = {}, const RankSet& pd = {},
                               const TraceDev& tr = {}, const MarksDev& md = {}) {
  const int ns = bt->n_slots;
  const auto to_host = [c](void* dst, const void* src, size_t bytes) {
    KP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  };
  if (tr.total > 0) to_host(rq.trace->out_loss, tr.loss, sizeof(float) * (size_t)tr.total);
  if (md.nm > 0) {
    const size_t n = (size_t)md.rows.n;
    to_host(rq.marks->out_score, md.rows.target, sizeof(float) * n);
    to_host(rq.marks->out_rank, md.rows.rank, sizeof(int64_t) * n);
    if (rq.marks->out_x)
      KP_HIP(hipMemcpy2DAsync(rq.marks->out_x, sizeof(float) * c->dim, md.X, sizeof(float) * c->dp,
                              sizeof(float) * c->dim, n, hipMemcpyDeviceToHost, c->stream));
  }
  if (bt->out_x) to_host(xp.data(), dX, sizeof(float) * xp.size());
  to_host(bt->out_score, r.target, sizeof(float) * ns);
  to_host(bt->out_rank, r.rank, sizeof(int64_t) * ns);
  if (rq.k > 0) {
    to_host(rq.ids, r.top_ids, sizeof(int32_t) * (size_t)ns * rq.k);
    to_host(rq.scores, r.top_scores, sizeof(float) * (size_t)ns * rq.k);
  }
  if (pd.n > 0) {
    to_host(rq.probes->out_score, pd.target, sizeof(float) * pd.n);
    to_host(rq.probes->out_rank, pd.rank, sizeof(int64_t) * pd.n);
  }
  if (rq.margins) {
    download_margins(c, r.mg, rq.margins->slots, (size_t)ns);
    download_margins(c, pd.mg, rq.margins->probes, (size_t)pd.n);
    download_margins(c, md.rows.mg, rq.margins->marks, (size_t)md.rows.n);
  }
  const double t_wait = g_host_times ? host_ms() : 0.0;
  KP_HIP(hipStreamSynchronize(c->stream));
  if (bt->out_x)
    for (int s = 0; s < ns; ++s)
      std::memcpy(bt->out_x + (size_t)s * c->dim, &xp[(size_t)s * c->dp], sizeof(float) * c->dim);
  return t_wait;
}

// the timing of a call whose hot launches were bracketed by the context's event pairs
// (2i, 2i + 1), one c->hot_pairs entry (work units, 0) each: the call (ev0 -> ev1), its
// loop (loop0 -> loop1), each hot launch's duration and interval, and the work sum in
// units of n_ent.  After the stream has been synchronised.
inline void record_hot_timing(kp_ctx* c, int64_t hot_launches, hipEvent_t loop0, hipEvent_t loop1) {
  float ms_all = 0.f, ms_loop = 0.f;
  KP_HIP(hipEventElapsedTime(&ms_all, c->ev0, c->ev1));
  KP_HIP(hipEventElapsedTime(&ms_loop, loop0, loop1));
  double hot = 0.0, work = 0.0;
  for (size_t i = 0; i < c->hot_pairs.size(); ++i) {
    float ms = 0.f;
    KP_HIP(hipEventElapsedTime(&ms, c->event(2 * i), c->event(2 * i + 1)));
    c->hot_pairs[i].second = ms * 1e-3;
    hot += ms * 1e-3;
    kp_push_interval(c, c->event(2 * i), c->event(2 * i + 1));
    work += c->hot_pairs[i].first * (double)c->n_ent;
  }
  c->timing.device_s = ms_all * 1e-3;
  c->timing.loop_s = ms_loop * 1e-3;
  c->timing.hot_s = hot;
  c->timing.hot_launches = hot_launches;
  c->timing.hot_work = work;
}
