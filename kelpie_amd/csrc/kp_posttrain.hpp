// kp_posttrain.hpp -- the host work the three *_posttrain_rank functions share: the batch
// check, Adam's step scalars, the kelpie rows' padding, the rank inputs, the result download
// and the hot-launch timing.  The model-specific step planning is pure host code in headers
// of its own (kp_cx_plan.hpp: ComplEx / DistMult; kp_cv_plan.hpp: ConvE; TransE's schedule
// is kp_sched.cpp); the launches, and where in the call the rank inputs are uploaded, stay
// in kp_complex.hip / kp_transe.hip / kp_conve.hip.
#pragma once

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "kp_batch_check.hpp"
#include "kp_common.hpp"
#include "kp_marks_check.hpp"
#include "kp_probe_check.hpp"
#include "kp_trace_check.hpp"

// KP_HOST_TIMES=1 (diagnostic): ComplEx and ConvE print, per call on stderr, the host time
// of their phases (planning, uploads, enqueueing the loop, waiting for the device)
inline const bool g_host_times = std::getenv("KP_HOST_TIMES") != nullptr;
inline double host_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the structural checks of kp_batch_check.hpp, thrown as KP_EINVAL under the model's name;
// first thing in every *_posttrain_rank, so a malformed batch leaves no device work in flight
inline void require_batch(const kp_ctx* c, const kp_batch* bt, const char* model) {
  if (const char* why = kp_check_batch(c->n_ent, c->n_rel2, c->dim, bt))
    throw KpError{KP_EINVAL, std::string(model) + ": " + why};
}

// kp_posttrain_rank_topk's k and outputs, checked right after the batch and before the first
// upload.  `rank64`: the call ranks on launch_rank_f64's fp64 operands; the fp32 diagnostic
// rank (KP_TE_RANK / KP_CV_RANK = f32) has none to select from
inline void require_topk(const TopkOut& tk, bool rank64, const char* model) {
  if (tk.k < 0 || tk.k > 32) throw KpError{KP_EINVAL, std::string(model) + ": top-k: k must be in [0, 32]"};
  if (tk.k > 0 && (!tk.ids || !tk.scores)) throw KpError{KP_EINVAL, std::string(model) + ": top-k: missing output"};
  if (tk.k > 0 && !rank64)
    throw KpError{KP_ENOTSUP, std::string(model) + ": top-k needs the fp64 rank (the fp32 rank switch is set)"};
}

// kp_posttrain_rank_probes' probes (kp_probe_check.hpp), checked right after the batch and
// the top-k request and before the first upload; like the lists they need the fp64 rank
inline void require_probes(const kp_ctx* c, const kp_batch* bt, const TopkOut& tk, bool rank64, const char* model) {
  if (!tk.probes) return;
  if (const char* why = kp_check_probes(c->n_ent, c->n_rel2, bt->n_slots, tk.probes))
    throw KpError{KP_EINVAL, std::string(model) + ": probes: " + why};
  if (tk.probes->n > 0 && !rank64)
    throw KpError{KP_ENOTSUP, std::string(model) + ": probes need the fp64 rank (the fp32 rank switch is set)"};
}

// kp_posttrain_rank_trace's request (kp_trace_check.hpp), checked after the batch and the
// probes and before the first upload.  The trace does not depend on the rank, so the fp32
// rank switches are no reason to refuse it
inline void require_trace(const kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const TopkOut& tk, const char* model) {
  if (!tk.trace) return;
  if (const char* why = kp_check_trace(c->model, hp, bt->n_slots, bt->row_off, bt->rows, tk.trace))
    throw KpError{KP_EINVAL, std::string(model) + ": trace: " + why};
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
// and uploaded into `b`
inline float* upload_x0(kp_ctx* c, DevBuf& b, const kp_batch* bt, std::vector<float>& xp) {
  const int ns = bt->n_slots;
  xp.assign((size_t)ns * c->dp, 0.f);
  for (int s = 0; s < ns; ++s)
    std::memcpy(&xp[(size_t)s * c->dp], bt->x0 + (size_t)s * c->dim, sizeof(float) * c->dim);
  return upload(c, b, xp.data(), xp.size());
}

// the rank's inputs and results on the device (c->rank)
struct RankDev {
  int32_t* po;        // [ns] the ranked objects
  int32_t* filt_off;  // the filter CSR
  int32_t* filt;
  float* target;  // [ns]
  int64_t* rank;  // [ns]
  int32_t* top_ids = nullptr;   // [ns][k] (kp_posttrain_rank_topk, k > 0)
  float* top_scores = nullptr;  // [ns][k]
};

// upload the ranked objects and the filter CSR, size the result buffers.  The caller
// chooses where in its call this happens: an upload's position decides what it overlaps.
inline RankDev upload_rank_inputs(kp_ctx* c, const kp_batch* bt, const TopkOut& tk = {}) {
  const int ns = bt->n_slots;
  std::vector<int32_t> po(ns);
  for (int s = 0; s < ns; ++s) po[s] = bt->pred[3 * s + 2];
  RankDev r;
  r.po = upload(c, c->rank.po, po.data(), po.size());
  r.filt_off = upload(c, c->rank.filt_off, bt->filt_off, (size_t)ns + 1);
  r.filt = upload(c, c->rank.filt, bt->filt, (size_t)bt->filt_off[ns]);
  r.target = reinterpret_cast<float*>(c->rank.target.ensure(sizeof(float) * (size_t)ns));
  r.rank = reinterpret_cast<int64_t*>(c->rank.rank.ensure(sizeof(int64_t) * (size_t)ns));
  if (tk.k > 0) {
    r.top_ids = reinterpret_cast<int32_t*>(c->rank.top_ids.ensure(sizeof(int32_t) * (size_t)ns * tk.k));
    r.top_scores = reinterpret_cast<float*>(c->rank.top_scores.ensure(sizeof(float) * (size_t)ns * tk.k));
  }
  return r;
}

// launch_rank_f64's fp64 operands: the queries [ns][dp], and the target scores [ns]
// followed by the kelpie column scores [ns]
struct Rank64Dev {
  double *q, *t, *kcol;
};
inline Rank64Dev rank64_buffers(kp_ctx* c, int ns) {
  Rank64Dev r;
  r.q = reinterpret_cast<double*>(c->rank.q64.ensure(sizeof(double) * (size_t)ns * c->dp));
  r.t = reinterpret_cast<double*>(c->rank.t64.ensure(sizeof(double) * 2 * (size_t)ns));
  r.kcol = r.t + ns;
  return r;
}

// the probes on the device (c->rank.p_*): inputs and results of all n probes, and the fp64
// operands of one chunk of probe rows (the chunks run one after the other on the stream)
constexpr size_t PROBE_WS_BYTES = (size_t)64 << 20;  // a chunk's query rows and bitmaps, as TOPK_WS_BYTES
constexpr int PROBE_GROUP = 16;                      // kp_rank_f64_count's rows per workgroup row (RQ)
struct ProbeDev {
  int n = 0, chunk = 0;
  int32_t* trip = nullptr;  // [n][3] (slot, p, o)
  int32_t* po = nullptr;    // [n]
  int32_t* filt_off = nullptr;
  int32_t* filt = nullptr;
  float* target = nullptr;  // [n]
  int64_t* rank = nullptr;  // [n]
  double *q = nullptr, *t = nullptr, *kcol = nullptr;  // [chunk][dp], [chunk], [chunk]
};

// upload the probes and size every probe buffer; called with the call's other uploads,
// ahead of the step loop.  `extra_row_bytes`: what else the model holds per probe row of a
// chunk (ConvE: the encoder's rows), counted into the chunk's budget
inline ProbeDev upload_probes(kp_ctx* c, const kp_batch* bt, const TopkOut& tk, size_t extra_row_bytes = 0) {
  ProbeDev d;
  const int n = tk.n_probes();
  if (n == 0) return d;
  const kp_probes* pr = tk.probes;
  std::vector<int32_t> trip((size_t)n * 3), po(n);
  for (int s = 0; s < bt->n_slots; ++s)
    for (int i = pr->probe_off[s]; i < pr->probe_off[s + 1]; ++i) {
      trip[3 * (size_t)i] = s;
      trip[3 * (size_t)i + 1] = pr->probes[2 * (size_t)i];
      trip[3 * (size_t)i + 2] = po[i] = pr->probes[2 * (size_t)i + 1];
    }
  const int nwords = (c->n_ent + 1 + 31) / 32;
  int forced = 0;
  if (const char* a = std::getenv("KP_PROBE_CHUNK")) forced = std::max(0, std::atoi(a));
  d.n = n;
  d.chunk = kp_probe_chunk(n, sizeof(double) * c->dp + sizeof(uint32_t) * nwords + extra_row_bytes, PROBE_WS_BYTES,
                           PROBE_GROUP, forced);
  d.trip = upload(c, c->rank.p_trip, trip.data(), trip.size());
  d.po = upload(c, c->rank.p_po, po.data(), po.size());
  d.filt_off = upload(c, c->rank.p_filt_off, pr->filt_off, (size_t)n + 1);
  d.filt = upload(c, c->rank.p_filt, pr->filt, (size_t)pr->filt_off[n]);
  d.target = reinterpret_cast<float*>(c->rank.p_target.ensure(sizeof(float) * (size_t)n));
  d.rank = reinterpret_cast<int64_t*>(c->rank.p_rank.ensure(sizeof(int64_t) * (size_t)n));
  d.q = reinterpret_cast<double*>(c->rank.p_q64.ensure(sizeof(double) * (size_t)d.chunk * c->dp));
  d.t = reinterpret_cast<double*>(c->rank.p_t64.ensure(sizeof(double) * 2 * (size_t)d.chunk));
  d.kcol = d.t + d.chunk;
  (void)c->rank.p_bits.ensure(sizeof(uint32_t) * (size_t)d.chunk * nwords);
  return d;
}

// rank the probe rows, chunk by chunk: `queries(r0, m)` enqueues the model's probe form of
// its query kernel for the probes [r0, r0 + m) (their fp64 rows, target and kelpie column
// scores into d.q / d.t / d.kcol), then the slots' own count runs over those rows (k = 0)
// (`bits`: the chunk's filter bitmaps; the mark rows, ranked the same way, bring their own)
template <class F>
inline void rank_probes(kp_ctx* c, const ProbeDev& d, int act, F&& queries, DevBuf* bits = nullptr) {
  for (int r0 = 0; r0 < d.n; r0 += d.chunk) {
    const int m = std::min(d.chunk, d.n - r0);
    queries(r0, m);
    launch_rank_f64(c, m, d.q, d.t, d.kcol, d.po + r0, d.filt_off + r0, d.filt, d.target + r0, d.rank + r0, act, 0,
                    nullptr, nullptr, bits ? bits : &c->rank.p_bits);
  }
}

// kp_posttrain_rank_marks' request (kp_marks_check.hpp), checked after the batch, the probes
// and the trace and before the first upload; like the lists and the probes the marks need the
// fp64 rank
inline void require_marks(const kp_hp* hp, const TopkOut& tk, bool rank64, const char* model) {
  if (!tk.marks) return;
  if (const char* why = kp_check_marks(hp, tk.marks))
    throw KpError{KP_EINVAL, std::string(model) + ": marks: " + why};
  if (!rank64)
    throw KpError{KP_ENOTSUP, std::string(model) + ": marks need the fp64 rank (the fp32 rank switch is set)"};
}

// the marks on the device: the mark rows X [ns][nm][dp] in the family's workspace (every row
// the padded x0 until a step captures it) and, in c->rank.m_*, the rows as rank rows in the
// probes' layout -- row s * nm + j is (row, p, o) of slot s with the slot's filter list -- so
// the probe form of the family's query kernel reads "row trip[3 r] of X" from the mark
// workspace and rank_probes counts them
struct MarksDev {
  int nm = 0;         // marks per slot (0: no marks)
  float* X = nullptr;
  ProbeDev rows;      // n = ns * nm
  KpMarkPlan plan;
};

// plan the marks, size every mark buffer, upload the rank rows and start every mark row as
// its slot's padded x0 (dX, already uploaded on the stream); with the call's other uploads,
// ahead of the step loop.  `ws`: the family's mark workspace; `extra_row_bytes` as upload_probes'
inline MarksDev upload_marks(kp_ctx* c, DevBuf& ws, const kp_hp* hp, const kp_batch* bt, const TopkOut& tk,
                             const float* dX, size_t extra_row_bytes = 0) {
  MarksDev d;
  if (!tk.marks) return d;
  const int ns = bt->n_slots, nm = tk.marks->n, n = ns * nm;
  if (const char* why = kp_marks_plan(c->model, hp, ns, bt->row_off, bt->rows, tk.marks, d.plan))
    throw KpError{KP_EINVAL, std::string("marks: ") + why};
  KP_REQUIRE((int64_t)ns * nm <= INT32_MAX / 4, "marks: too many mark rows");
  d.nm = nm;
  d.X = reinterpret_cast<float*>(ws.ensure(sizeof(float) * (size_t)n * c->dp));
  for (int j = 0; j < nm; ++j)
    KP_HIP(hipMemcpy2DAsync(d.X + (size_t)j * c->dp, sizeof(float) * (size_t)nm * c->dp, dX, sizeof(float) * c->dp,
                            sizeof(float) * c->dp, ns, hipMemcpyDeviceToDevice, c->stream));
  std::vector<int32_t> trip((size_t)n * 3), po(n), fo((size_t)n + 1, 0);
  int64_t nf = 0;
  for (int s = 0; s < ns; ++s) nf += (int64_t)nm * (bt->filt_off[s + 1] - bt->filt_off[s]);
  KP_REQUIRE(nf <= INT32_MAX, "marks: the mark rows' filter lists exceed 2^31 - 1 entries");
  std::vector<int32_t> filt((size_t)std::max<int64_t>(1, nf));
  for (int s = 0; s < ns; ++s)
    for (int j = 0; j < nm; ++j) {
      const size_t r = (size_t)s * nm + j;
      trip[3 * r] = (int32_t)r;
      trip[3 * r + 1] = bt->pred[3 * s + 1];
      trip[3 * r + 2] = po[r] = bt->pred[3 * s + 2];
      const int len = bt->filt_off[s + 1] - bt->filt_off[s];
      if (len > 0) std::memcpy(&filt[fo[r]], bt->filt + bt->filt_off[s], sizeof(int32_t) * len);
      fo[r + 1] = fo[r] + len;
    }
  const int nwords = (c->n_ent + 1 + 31) / 32;
  int forced = 0;
  if (const char* a = std::getenv("KP_MARKS_CHUNK")) forced = std::max(0, std::atoi(a));
  ProbeDev& p = d.rows;
  p.n = n;
  p.chunk = kp_probe_chunk(n, sizeof(double) * c->dp + sizeof(uint32_t) * nwords + extra_row_bytes, PROBE_WS_BYTES,
                           PROBE_GROUP, forced);
  p.trip = upload(c, c->rank.m_trip, trip.data(), trip.size());
  p.po = upload(c, c->rank.m_po, po.data(), po.size());
  p.filt_off = upload(c, c->rank.m_filt_off, fo.data(), fo.size());
  p.filt = upload(c, c->rank.m_filt, filt.data(), filt.size());
  p.target = reinterpret_cast<float*>(c->rank.m_target.ensure(sizeof(float) * (size_t)n));
  p.rank = reinterpret_cast<int64_t*>(c->rank.m_rank.ensure(sizeof(int64_t) * (size_t)n));
  p.q = reinterpret_cast<double*>(c->rank.m_q64.ensure(sizeof(double) * (size_t)p.chunk * c->dp));
  p.t = reinterpret_cast<double*>(c->rank.m_t64.ensure(sizeof(double) * 2 * (size_t)p.chunk));
  p.kcol = p.t + p.chunk;
  (void)c->rank.m_bits.ensure(sizeof(uint32_t) * (size_t)p.chunk * nwords);
  // the uploads above read host vectors that end with this call: pageable copies are staged
  // before hipMemcpyAsync returns
  return d;
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

// enqueue the downloads of the marks' results, ahead of download_results' one wait
inline void download_marks(kp_ctx* c, const kp_batch* bt, const TopkOut& tk, const MarksDev& d) {
  if (d.nm == 0) return;
  const size_t n = (size_t)d.rows.n;
  KP_HIP(hipMemcpyAsync(tk.marks->out_score, d.rows.target, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipMemcpyAsync(tk.marks->out_rank, d.rows.rank, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream));
  if (tk.marks->out_x)
    KP_HIP(hipMemcpy2DAsync(tk.marks->out_x, sizeof(float) * c->dim, d.X, sizeof(float) * c->dp, sizeof(float) * c->dim,
                            n, hipMemcpyDeviceToHost, c->stream));
}

// the tail of a call: enqueue the downloads of the kelpie rows (when out_x is set), the
// target scores, the ranks, the top-k lists and the probes' results (when asked for), wait
// for the stream once, unpad the rows into out_x.
// Returns the host time at which the wait began (0 unless KP_HOST_TIMES).
inline double download_results(kp_ctx* c, const kp_batch* bt, const float* dX, const RankDev& r,
                               std::vector<float>& xp, const TopkOut& tk = {}, const ProbeDev& pd = {}) {
  const int ns = bt->n_slots;
  if (bt->out_x) KP_HIP(hipMemcpyAsync(xp.data(), dX, sizeof(float) * xp.size(), hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipMemcpyAsync(bt->out_score, r.target, sizeof(float) * ns, hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipMemcpyAsync(bt->out_rank, r.rank, sizeof(int64_t) * ns, hipMemcpyDeviceToHost, c->stream));
  if (tk.k > 0) {
    const size_t n = (size_t)ns * tk.k;
    KP_HIP(hipMemcpyAsync(tk.ids, r.top_ids, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    KP_HIP(hipMemcpyAsync(tk.scores, r.top_scores, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  }
  if (pd.n > 0) {
    KP_HIP(hipMemcpyAsync(tk.probes->out_score, pd.target, sizeof(float) * pd.n, hipMemcpyDeviceToHost, c->stream));
    KP_HIP(hipMemcpyAsync(tk.probes->out_rank, pd.rank, sizeof(int64_t) * pd.n, hipMemcpyDeviceToHost, c->stream));
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
