// kp_common.hpp -- shared host/device helpers of the Kelpie HIP library (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/kelpie_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define KP_WAVE 64

// ----------------------------------------------------------------------------
// error plumbing
// ----------------------------------------------------------------------------
struct KpError {
  int code;
  std::string msg;
};

#define KP_HIP(expr)                                                              \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess)                                                         \
      throw KpError{KP_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)}; \
  } while (0)

#define KP_REQUIRE(cond, msg)                         \
  do {                                                \
    if (!(cond)) throw KpError{KP_EINVAL, (msg)};     \
  } while (0)

// grow-only device buffer.  A buffer bound to its context's stream (`s`, set by
// kp_ctx_create for the context's own workspaces) grows stream-ordered: the new
// allocation comes from the device's default memory pool (hipMallocAsync) and the old one
// goes back to it (hipFreeAsync) once the stream reaches the free -- no device-wide
// synchronisation (hipFree waits for the whole device, every context's queued work
// included, which stalled the batch thread that grew the buffer behind the other batches
// in flight), and no superseded allocation is kept.  An unbound buffer (call-local
// scratch) keeps its superseded allocations until release().
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipStream_t s = nullptr;
  hipMemPool_t pool = nullptr;  // the library's own pool of the device (kp_device_pool)
  std::vector<void*> old;
  void* ensure(size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (bytes > cap) {
      const size_t want = bytes + bytes / 4;
      void* q = nullptr;
      if (s) {
        if (pool)
          KP_HIP(hipMallocFromPoolAsync(&q, want, pool, s));
        else
          KP_HIP(hipMallocAsync(&q, want, s));
        if (p) KP_HIP(hipFreeAsync(p, s));
      } else {
        KP_HIP(hipMalloc(&q, want));
        if (p) old.push_back(p);
      }
      p = q;
      cap = want;
    }
    return p;
  }
  template <class T>
  T* as() { return reinterpret_cast<T*>(p); }
  void release() {
    if (p) (void)(s ? hipFreeAsync(p, s) : hipFree(p));
    for (void* q : old) (void)hipFree(q);
    old.clear();
    p = nullptr;
    cap = 0;
  }
};

// ----------------------------------------------------------------------------
// the context's device buffers, by name.  Each struct below holds DevBufs only and lists
// every one of them in all(); kp_ctx::buffers() joins the lists, and kp_ctx_create (stream
// and pool binding) and kp_ctx_destroy (release) walk nothing else.  KP_WS_COMPLETE fails
// the build when a member is added to a struct but not to its list, so no buffer can be
// left unbound (an unbound buffer grows with hipMalloc / hipFree, which synchronise the
// whole device).  A context belongs to one model family; the other families' buffers stay
// empty.
// ----------------------------------------------------------------------------
#define KP_WS_COMPLETE(S)                                                                          \
  static_assert(sizeof(S) == sizeof(DevBuf) * std::tuple_size<decltype(std::declval<S&>().all())>::value, \
                #S "::all() must list every DevBuf member")

// images of the frozen tables and layers, built on first use and kept (their *_ready flags
// are in kp_ctx)
struct ImageBufs {
  DevBuf e3;                // kp_attn3's split image of dE
  DevBuf e3ts, e3pre;       // kp_attn3's fp64 tile sums / prefix sums of dE over tiles
  DevBuf eT;                // dE transposed [dp][round_up(n_ent, 256)] fp32 (fp64 rank scoring)
  DevBuf cvf_fw3, cvf_bw3;  // kp_cv_fused.hpp's permuted split images of the ConvE FC weight
  DevBuf cv_wtm, cv_trel;   // shared-encoder split: map-row-18-19 FC columns, the relations' FC terms
  DevBuf cv_wtl, cv_wfm;    // the kelpie rows' FC columns and the mid columns, transposed
  DevBuf cv_wlc;            // the kelpie rows' FC columns [dim][4608]
  auto all() {
    return std::array{&e3, &e3ts, &e3pre, &eT, &cvf_fw3, &cvf_bw3, &cv_wtm, &cv_trel, &cv_wtl, &cv_wfm, &cv_wlc};
  }
};
KP_WS_COMPLETE(ImageBufs);

// join the buffer lists of a struct's own members and of its member structs
template <size_t... N>
inline auto kp_join(const std::array<DevBuf*, N>&... lists) {
  std::array<DevBuf*, (N + ...)> out{};
  size_t i = 0;
  ((std::copy(lists.begin(), lists.end(), out.begin() + i), i += N), ...);
  return out;
}

// the buffers of one set of rank rows (RankSet below: kp_posttrain.hpp's upload_rank_rows
// fills it, rank_rows counts it): the rows' (row, p, o) [n][3], objects [n], filter CSR and
// results [n]; one chunk of rows' fp64 queries [chunk][dp], target | kelpie column scores
// [2][chunk] and filter bitmaps; ConvE: the rows' encoder sources (-row - 1, p) [n] and one
// chunk's encoder output [chunk][dp] (the slots' is ConveWs::q); the rows' margins [n] and one
// chunk's margin workspace (MarginDev)
struct RankRowsWs {
  DevBuf trip, po, filt_off, filt;
  DevBuf target, rank;
  DevBuf q64, t64, bits;
  DevBuf enc_src, enc_q;
  DevBuf mg_out, mg_part;
  auto all() {
    return std::array{&trip, &po, &filt_off, &filt, &target, &rank, &q64, &t64, &bits, &enc_src, &enc_q, &mg_out, &mg_part};
  }
};
KP_WS_COMPLETE(RankRowsWs);

// what every *_posttrain_rank shares (kp_posttrain.hpp fills it): the four sets of rank rows,
// what only the slots have, and the trace.
//   slots:  row s is (s, p_s, o_s) on the post-trained kelpie rows; never chunked;
//   probes: kp_posttrain_rank_probes, row r is probe r, (slot, p, o), on the same rows;
//   marks:  kp_posttrain_rank_marks, row s * marks + j is (row, p, o) of slot s on the family's
//           mark workspace [ns][marks][dp], with the slot's filter list;
//   f64:    kp_posttrain_rank_f64's slots, on its double rows.
// The sets share a type and nothing else: the probes and the marks rank while the earlier
// sets' downloads are still pending, and an fp64 call leaves every buffer of the fp32 path as
// it was.
// Two borrowers outside a post-training call, kept so that a context allocates what it
// always did: complex_all_scores uploads its heads / relations into slots.trip / slots.po, and
// transe_all_scores writes its score matrix into scores.
struct RankWs {
  RankRowsWs slots;
  DevBuf scores;  // fp32 score matrix [ns][ld] (KP_TE_RANK / KP_CV_RANK = f32)
  // kp_posttrain_rank_topk (kp_rank.hip owns the first two): the waves' candidate lists
  // [chunk slots][4 column blocks][k] (sort keys, columns) of one chunk of slots, and the
  // final lists [ns][k]
  DevBuf cand_key, cand_col;
  DevBuf top_ids, top_scores;
  DevBuf tr_off, tr_loss;  // kp_posttrain_rank_trace: the trace offsets [ns + 1] and the losses [steps]
  RankRowsWs probes, marks, f64;
  auto all() {
    return kp_join(slots.all(), std::array{&scores, &cand_key, &cand_col, &top_ids, &top_scores, &tr_off, &tr_loss},
                   probes.all(), marks.all(), f64.all());
  }
};
KP_WS_COMPLETE(RankWs);

// kp_complex.hip: the workspaces of the post-training step in one precision (kp_complex.hip's
// CxDev<T> is their device side; rows, state, sums, queries and partials are T, the plan's
// uploads the same in either)
struct CxStepWs {
  DevBuf x, s1, s2;                // kelpie rows [ns][dp] and their Adagrad / Adam moments
  DevBuf plans, queries, targets;  // CxPlan, CxQuery, the queries' frozen targets
  DevBuf pairs, acts;              // frozen-head (h, r) pairs; per-step active slots
  DevBuf stepq, stept;             // per-step query / tail items
  DevBuf contrib;                  // per-step gradient contributions [items][dp]
  DevBuf tsum, qpair, lsef;        // target sums [queries][dp]; pair queries [pairs][dp], their frozen lse
  DevBuf am, al, ao;               // attention partials per split / key range (max, sum, output)
  DevBuf qs;                       // the step's queries [nq][dp]
  auto all() {
    return std::array{&x, &s1, &s2, &plans, &queries, &targets, &pairs, &acts, &stepq, &stept, &contrib,
                      &tsum, &qpair, &lsef, &am, &al, &ao, &qs};
  }
};
KP_WS_COMPLETE(CxStepWs);

// kp_complex.hip: the step's workspaces once per precision -- f32, and f64 for
// kp_posttrain_rank_f64 -- two objects that share a type and no buffer (an fp64 call leaves
// every buffer of the fp32 path as it was), and what only the fp32 path has
struct ComplexWs {
  CxStepWs f32, f64;
  template <class T>
  CxStepWs& step() {
    return sizeof(T) == sizeof(double) ? f64 : f32;
  }
  DevBuf score_q, score_out;       // complex_scores_dev's queries, complex_all_scores' scores
  // kp_posttrain_rank_trace: the step's fp64 loss term per item [items] and the frozen rows'
  // regulariser factors [n_ent] / [n_rel2] (fp64, once per batch)
  DevBuf tr_term, tr_fe, tr_fr;
  // kp_posttrain_rank_marks: the mark rows [ns][marks][dp] and, per entry of acts, the mark
  // row its update also stores (-1: none)
  DevBuf marks, mark_row;
  // kp_posttrain_rank_attrib: the row map's index lists (kp_cx_rowmap.hpp); the slots' score
  // gradients c [ns][dp] (fp64); per slot the step's D_t and x_t, the initial rows and the N2
  // norm (fp32: [3][ns][dp] + [ns]); the results fit | reg [rows] and delta [ns] (fp64)
  DevBuf at_map, at_c, at_f, at_out;
  auto all() {
    return kp_join(f32.all(), std::array{&score_q, &score_out, &tr_term, &tr_fe, &tr_fr, &marks, &mark_row, &at_map,
                                         &at_c, &at_f, &at_out},
                   f64.all());
  }
};
KP_WS_COMPLETE(ComplexWs);

// kp_transe.hip
struct TranseWs {
  DevBuf x;                 // kelpie rows [ns][dp]
  DevBuf slots, rows, rng;  // TeSlot, the batch's training rows and draws
  DevBuf order;             // slots, longest first
  DevBuf heads, rels;       // score queries: the ranked triples' (-1, relation), and transe_all_scores' pairs
  DevBuf marks, mark_ep;    // kp_posttrain_rank_marks: the mark rows [ns][marks][dp]; the header and the epochs' marks
  auto all() {
    return std::array{&x, &slots, &rows, &rng, &order, &heads, &rels, &marks, &mark_ep};
  }
};
KP_WS_COMPLETE(TranseWs);

// kp_keyed.hip: the keyed draws' inputs on the device (the keys, the slots' row and word
// offsets, the slot lists of the two permutation launches), the sorting network's global
// scratch for slots beyond its LDS form, and kp_keyed_draws' own outputs (the armed call
// generates into the family's x and rng)
struct KeyedWs {
  DevBuf init_key, slot_key;    // [ns] uint64
  DevBuf row_off, rng_off;      // [ns + 1] int32 / int64
  DevBuf lds_slots, big_slots;  // int32 slot lists: rows <= 4096 / beyond
  DevBuf scratch;               // [workgroups][N] (key word, row) pairs of the global network
  DevBuf x, rng;                // kp_keyed_draws' rows [ns][dp] and words; ComplEx's armed permutations
  auto all() {
    return std::array{&init_key, &slot_key, &row_off, &rng_off, &lds_slots, &big_slots, &scratch, &x, &rng};
  }
};
KP_WS_COMPLETE(KeyedWs);

// kp_conve.hip
struct ConveWs {
  DevBuf x, s1, s2;               // kelpie rows [ns][dp] and their Adam moments
  DevBuf kinst, finst, acts;      // CvInst, CvFInst, CvAct
  DevBuf tails;                   // the kelpie pairs' distinct tails
  DevBuf keep_bits;               // the dropout keep bits plus a zero guard word
  DevBuf fcf, fpairs;             // frozen-head pairs: FC rows [pairs][dim] and their (h, r)
  DevBuf flat;                    // flattened feature maps [rows][hidden]: the frozen pairs', then the
                                  // step's (unfused path), then encode_eval's
  DevBuf slab;                    // FC split-K slabs [KS][rows][dim]; encode_eval's FC output
  DevBuf relu, g3;                // fused path: ReLU bytes; kp_cv_dx's split gradient
  DevBuf sr_src, sr_rng, psr;     // shared-encoder split: kelpie rows' sources, pair ranges, pair -> row
  DevBuf relu_s, slab_l;          // its kelpie rows' ReLU bytes and FC slabs [KSL][rows][dim]
  DevBuf mid, map_l, map_m;       // pairs' mid FC terms; kelpie rows' / pairs' map rows (then gradients)
  DevBuf gs, dls;                 // kelpie rows' summed pair dfc; their lhs image gradient
  DevBuf q;                       // encoder output: the step's rows in the loop (dQ), the ranked
                                  // triples' rows after it (dQr)
  DevBuf enc_src, enc_bits;       // per-step encoder rows: sources and keep-bit offsets
  DevBuf fchunks, fpart;          // frozen-head pairs' chunks per step and their partial gradients
  DevBuf gscale;                  // 1 / (b (n_ent + 1)) per kelpie instance
  DevBuf o;                       // attention output [rows * splits][dp]
  DevBuf dfc, gk, dflat, dl;      // backward: dL/dfc, g . x, dL/dflat (unfused), lhs image gradient
  // kp_posttrain_rank_trace: a step's rows [rows][dp], one chunk's logits [chunk][ld] and the
  // rows' summed BCE terms (fp64)
  DevBuf tr_rows, tr_scores, tr_rowloss;
  // kp_posttrain_rank_marks: the mark rows [ns][marks][dp] and, per entry of the active lists,
  // the mark row its update also stores (-1: none).  (Every set of rank rows' encoder
  // sources, and the probes' and the mark rows' encoder outputs, are with the set: RankRowsWs.)
  DevBuf marks, mark_row;
  auto all() {
    return std::array{&x, &s1, &s2, &kinst, &finst, &acts, &tails, &keep_bits, &fcf, &fpairs, &flat, &slab,
                      &relu, &g3, &sr_src, &sr_rng, &psr, &relu_s, &slab_l, &mid, &map_l, &map_m, &gs, &dls,
                      &q, &enc_src, &enc_bits, &fchunks, &fpart, &gscale, &o, &dfc, &gk, &dflat, &dl,
                      &tr_rows, &tr_scores, &tr_rowloss, &marks, &mark_row};
  }
};
KP_WS_COMPLETE(ConveWs);

struct Timing {
  double device_s = 0.0;  // whole call on the device (first upload .. last kernel)
  double loop_s = 0.0;    // post-training loop
  double hot_s = 0.0;     // sum of the dominant kernel's launch durations
  int64_t hot_launches = 0;
  double hot_work = 0.0;  // work units of the dominant kernel (see kp_last_timing)
};

struct kp_train_state;  // kp_train.hip: optimizer state of a full-model training run
struct kp_cv_train;     // kp_train_conve.hip: ConvE full-model training state

struct kp_ctx : ImageBufs {
  int device = 0;
  int n_cu = 256;  // compute units of the device (one attention workgroup per CU)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int model = 0;
  int n_ent = 0, n_rel2 = 0, dim = 0, dp = 0;  // dp: padded row stride (multiple of 16)
  int hidden = 0;                              // ConvE
  float* dE = nullptr;                         // [n_ent][dp] zero-padded
  float* dR = nullptr;                         // [n_rel2][dp]
  // ConvE frozen layers
  float* d_conv_w = nullptr;
  float* d_conv_b = nullptr;
  float* d_fc_w = nullptr;   // [dim][hidden]
  float* d_fc_wt = nullptr;  // [hidden][dim], the unfused backward GEMM's operand (conve_fc_wt, on first use)
  float* d_fc_b = nullptr;
  float* d_bn_a = nullptr;
  float* d_bn_b = nullptr;
  std::vector<float> hE;     // host copy (ConvE/TransE helpers)
  // per-batch workspaces (the once-built images are the ImageBufs base)
  RankWs rank;
  ComplexWs cx;
  TranseWs te;
  ConveWs cv;
  KeyedWs kd;
  // kp_ctx_arm_keyed's copy of the request (keyed.init_key / slot_key point into the vectors)
  bool keyed_armed = false;
  kp_keyed keyed{};
  std::vector<uint64_t> keyed_init, keyed_slot;
  std::string err;
  Timing timing;
  bool time_hot = true;
  // attention contraction: 0 = fp32 MFMA (kp_attn.hpp), 1 = bf16x3 MFMA (kp_attn3.hpp)
  int attn_mode = 0;
  int attn_part = 0;  // kp_attn3 partition: 0 chosen per launch, 1 stream-K, 2 XCD-grouped ranges (KP_ATTN_PART)
  int attn_inflight = 1;  // batches whose attention launches share the device (kp_ctx_set_inflight)
  int attn_ranges = 0;    // > 0: kp_attn3 runs that many ranges, one workgroup per unit (KP_ATTN_RANGES)
  struct AttnLast {       // plan of the last batch's largest hot attention launch (kp_last_attn_plan)
    int nq = -1, inflight = 1, ranges = 0, n_parts = 0, n_wg = 0;
  } attn_last;
  bool e3_ready = false;     // ImageBufs::e3
  bool e3pre_ready = false;  // e3ts, e3pre
  bool eT_ready = false;
  int cv_fused = 1;        // ConvE d = 200: fused encoder kernels (kp_cv_fused.hpp), KP_CV_FUSED
  int cv_rank64 = 1;       // ConvE post-training rank on fp64 logits (KP_CV_RANK=f32: fp32 sigmoid scores)
  int cv_dx_block = 0;     // ConvE: the 256-thread kp_cv_dx instead of kp_cv_dx1 (KP_CV_DX=block, A/B)
  int te_norm = 2;         // TransE score norm p (kp_model_desc.norm_p): 2 or 1
  int te_rank64 = 1;       // TransE post-training rank on fp64 squared distances (KP_TE_RANK=f32: fp32 norms)
  bool cvf_ready = false;   // cvf_fw3, cvf_bw3
  int cv_shared = 1;        // ConvE fused path: the shared-encoder split (kp_cv_fused.hpp), KP_CV_SHARED
  bool cv_shared_ready = false;  // cv_wtm, cv_trel, cv_wtl, cv_wfm, cv_wlc
  int attn3_wpc[2] = {0, 0};  // co-resident kp_attn3 workgroups per CU, [softmax, BCE] (occupancy API)
  kp_train_state* train = nullptr;  // kp_train_epoch's state (freed with the context)
  kp_cv_train* cvtrain = nullptr;   // kp_conve_train_*'s state (freed with the context)
  std::vector<hipEvent_t> evpool;
  std::vector<std::pair<double, double>> hot_pairs;  // (work units, seconds) per hot launch
  std::vector<double> hot_iv;  // [start, end] per hot launch, seconds since the device's time base
  // every DevBuf of the context: all of them live on its stream (DevBuf::s).  kp_ctx holds
  // no DevBuf of its own; a new one goes into one of the structs above, whose all() then
  // has to name it
  std::vector<DevBuf*> buffers() {
    std::vector<DevBuf*> v;
    auto add = [&v](auto list) { v.insert(v.end(), list.begin(), list.end()); };
    add(ImageBufs::all());
    add(rank.all());
    add(cx.all());
    add(te.all());
    add(cv.all());
    add(kd.all());
    return v;
  }
  hipEvent_t event(size_t i) {
    while (evpool.size() <= i) {
      hipEvent_t e;
      KP_HIP(hipEventCreate(&e));
      evpool.push_back(e);
    }
    return evpool[i];
  }
};


static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// room for n elements of T in `b`
template <class T>
static inline T* ensure_n(DevBuf& b, size_t n) {
  return reinterpret_cast<T*>(b.ensure(sizeof(T) * n));
}

// upload helper
template <class T>
static inline T* upload(kp_ctx* c, DevBuf& b, const T* src, size_t n) {
  T* d = ensure_n<T>(b, n);
  if (n) KP_HIP(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return d;
}

// ----------------------------------------------------------------------------
// device helpers
// ----------------------------------------------------------------------------
// Sum over each 16-lane row with DPP (VALU lane moves, no LDS round trip):
// xor 1, xor 2 (quad_perm), half-mirror (quads of 8), mirror (halves of 16).
// Every lane of the row ends with the same bits (each step adds a symmetric pair).
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
  return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ----------------------------------------------------------------------------
// entry points implemented per model family
// ----------------------------------------------------------------------------
// the names the families' messages carry, by kp_model_desc.model
inline const char* kp_model_name(int model) {
  static const char* const names[] = {"TransE", "ComplEx", "ConvE", "DistMult"};
  return names[model];
}

// what a post-training call asks for besides its slots' scores and ranks (kp_api.hip builds
// it from the entry point's arguments; all absent: kp_posttrain_rank)
struct PostReq {
  // kp_posttrain_rank_topk: the k best unmasked columns of every slot into the caller's
  // ids / scores [n_slots][k]; k == 0: no lists
  int k = 0;
  int32_t* ids = nullptr;
  float* scores = nullptr;
  // kp_posttrain_rank_probes' request (nullptr or n == 0: no probes)
  const kp_probes* probes = nullptr;
  int n_probes() const { return probes ? probes->n : 0; }
  // kp_posttrain_rank_trace's request (nullptr: no trace)
  const kp_trace* trace = nullptr;
  // kp_posttrain_rank_marks' request (nullptr: no marks)
  const kp_marks* marks = nullptr;
  int n_marks() const { return marks ? marks->n : 0; }
  // kp_posttrain_rank_margins' request (nullptr: no margins)
  const kp_margins* margins = nullptr;
  // kp_posttrain_rank_attrib's request (nullptr: no attributions)
  const kp_attrib* attrib = nullptr;
  // kp_posttrain_rank_f64's request (nullptr: the fp32 / bf16x3 step): the double inputs,
  // hyper-parameters and outputs.  ComplEx / DistMult; the lists, the probes, the trace and
  // the marks are not offered with it yet (require_request)
  const kp_f64* f64 = nullptr;
  // the armed context's keyed request (nullptr: the draws are the batch's x0 / rng_off / rng):
  // the batch's three buffers are NULL and the family generates them (kp_keyed.hip)
  const kp_keyed* keyed = nullptr;
};
// kp_keyed.hip: the keyed draws on the context's stream.  keyed_x0_dev: the slots' rows
// [ns][dp] into dX, padding included.  keyed_rng_dev: the slots' words into dRng at the offsets
// rng_off (host, [ns + 1]: kp_keyed_words_host's prefix sums).
void keyed_x0_dev(kp_ctx* c, const kp_keyed* k, int ns, float* dX);
void keyed_rng_dev(kp_ctx* c, const kp_hp* hp, const kp_keyed* k, int ns, const int32_t* row_off,
                   const int64_t* rng_off, int32_t* dRng);
// kp_keyed_draws: the request check, the generation into the keyed workspace and the download
void keyed_draws(kp_ctx* c, const kp_hp* hp, int ns, const int32_t* row_off, const kp_keyed* k, float* out_x0,
                 int64_t* out_rng_off, int32_t* out_rng, int64_t cap);
void complex_posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* b, const PostReq& rq = {});
// kp_complex.hip, product policy
void distmult_posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* b, const PostReq& rq = {});
void complex_all_scores(kp_ctx* c, int n, const int32_t* heads, const int32_t* rels, float* out);
// scores of n (head, rel) pairs over the frozen entities into a device buffer [n][ld]
// (complex_*: ComplEx and DistMult contexts, by the context's product)
void complex_scores_dev(kp_ctx* c, int n, const int32_t* d_heads, const int32_t* d_rels, float* d_out, int ld);
void transe_scores_dev(kp_ctx* c, int n, const int32_t* d_heads, const int32_t* d_rels, float* d_out, int ld);
void conve_scores_dev(kp_ctx* c, int n, const int32_t* d_heads, const int32_t* d_rels, float* d_out, int ld);
void launch_convertible_reduce(kp_ctx* c, int n, const float* d_scores, int ld, int obj, const int32_t* d_fo,
                               const int32_t* d_f, int minimizer, uint8_t* d_keep);
void transe_posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* b, const PostReq& rq = {});
void transe_all_scores(kp_ctx* c, int n, const int32_t* heads, const int32_t* rels, float* out);
void conve_posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* b, const PostReq& rq = {});
void conve_all_scores(kp_ctx* c, int n, const int32_t* heads, const int32_t* rels, float* out);
// ConvE encoder output (eval mode) of n (lhs, rel) pairs -> [n][dp] (criage_first_step, conve.py:102-124)
void conve_encode_dev(kp_ctx* c, int n, const int2* d_src, float* d_out);
// baseline engines (kp_baselines.hip)
void dp_relevance(kp_ctx* c, int n, const int32_t* items, float eps, float lambd, int step_sign, int rel_sign,
                  float* out);
void criage_relevance(kp_ctx* c, int n, const int32_t* items, int n_ents, const int32_t* ent_ids,
                      const int32_t* tails_off, const int32_t* tails, double* out, int32_t* status);

// shared rank kernel launcher (kp_rank.hip): scores [n][ld] already on device,
// column `kcol` = kelpie score (or -1 when absent)
void launch_score_gemm(kp_ctx* c, const float* dQ, int nq, float* d_out, int ld, int act);
// kp_train.hip: one MultiClassNLLOptimizer epoch on the context's tables (ComplEx)
void complex_train_epoch(kp_ctx* c, const kp_hp* hp, int n, const int32_t* triples, const int32_t* perm, int epoch);
// kp_train.hip: one PairwiseRankingOptimizer epoch (TransE): positive and corrupted rows in order
void transe_train_epoch(kp_ctx* c, const kp_hp* hp, int n, const int32_t* pos, const int32_t* neg, int epoch);
void train_state_free(kp_ctx* c);
// kp_train_conve.hip: ConvE BCEOptimizer training (see include/kelpie_hip.h kp_conve_train_*)
void cv_train_free(kp_ctx* c);
void conve_train_begin(kp_ctx* c, const float* bn_w, const float* bn_b, const float* bn_m, const float* bn_v);
void conve_train_step(kp_ctx* c, int B, const int32_t* pairs, const int32_t* tail_off, const int32_t* tails,
                      const float* in_noise, const float* fm_noise, const float* hid_noise, float lr,
                      float label_smoothing, int bn_train);
void conve_train_read(kp_ctx* c, float* conv_w, float* conv_b, float* fc_w, float* fc_b, float* bn_w, float* bn_b,
                      float* bn_m, float* bn_v);
// out[z][m][n] = act(sum_{k in split z} A[m][k] B[n][k] + (z == 0 ? bias[n] : 0)), fp32 MFMA
void launch_gemm_abt(kp_ctx* c, const float* A, int lda, int M, const float* B, int ldb, int N, int K, float* out,
                     int ldo, const float* bias, int act, int ksplit);
enum { RANK_TRIPLE_RESULTS = 0, RANK_PREDICT_TAILS = 1, RANK_SORT_POSITION = 2 };
// launch_rank_f64's score kinds
enum { RANK64_DOT = 0, RANK64_SIGMOID = 1, RANK64_DIST = 2, RANK64_DIST1 = 3 };
// The margins of a set of rank rows on the device: the results [n] of every row, and the
// workspace of one launch of `cap` rows over `nblk` column blocks of 256 (no allocation at
// launch time: kp_posttrain.hpp's margin_buffers sizes both with the call's other buffers).
struct MarginDev {
  double tol = 0.0;
  int64_t *rank_lo = nullptr, *rank_hi = nullptr, *ties = nullptr;  // [n]
  double *gap_better = nullptr, *gap_worse = nullptr;               // [n]
  int32_t *id_better = nullptr, *id_worse = nullptr;                // [n]
  double* thr = nullptr;               // [cap][2] thr_lo, thr_hi
  unsigned long long* pkey = nullptr;  // [cap][nblk][2] the blocks' nearest better / worse keys
  int32_t* pcol = nullptr;             // [cap][nblk][2] their columns (-1: none)
  int32_t* pcnt = nullptr;             // [cap][nblk][3] the blocks' counts: lo, hi, ties
  int cap = 0, nblk = 0;
  // the same workspace for the rows from r0 on
  MarginDev at(size_t r0) const {
    MarginDev m = *this;
    m.rank_lo += r0, m.rank_hi += r0, m.ties += r0, m.gap_better += r0, m.gap_worse += r0, m.id_better += r0,
        m.id_worse += r0;
    return m;
  }
};
// A set of rows to rank, on the device (one RankRowsWs each; kp_posttrain.hpp's
// upload_rank_rows builds every set).  Row r is (row, p, o): the family's query kernel reads
// "row rows[3 r] of X", relation p, object o.  The inputs and results of all n rows, and the
// fp64 operands and filter bitmaps of one chunk of rows (the chunks run one after the other on
// the stream; the slots are one chunk).
struct RankSet {
  int n = 0, chunk = 0;
  const float* X = nullptr;  // the rows rows[3 r] indexes (kp_posttrain_rank_f64: its queries hold the double rows)
  int32_t* rows = nullptr;   // [n][3] (row, p, o)
  int32_t* po = nullptr;     // [n] the objects
  int32_t* filt_off = nullptr;  // the filter CSR
  int32_t* filt = nullptr;
  float* target = nullptr;  // [n] results
  int64_t* rank = nullptr;  // [n]
  // one chunk (nullptr under the fp32 diagnostic ranks): the fp64 queries [chunk][dp], the target
  // scores [chunk] (q . E_o, or the kelpie column when o is the kelpie) and the kelpie column
  // scores [chunk], the filter bitmaps over the n_ent + 1 columns
  double *q = nullptr, *t = nullptr, *kcol = nullptr;
  uint32_t* bits = nullptr;
  int2* enc_src = nullptr;  // ConvE: [n] the rows' encoder sources (-row - 1, p)
  float* enc_q = nullptr;   // ConvE: [chunk][dp] the chunk's encoder output
  MarginDev mg;             // the rows' margins (cap 0: none), one chunk's workspace
  // the slots only (kp_posttrain_rank_topk, k > 0): the k best unmasked columns of every row
  // (better value first, equal values by column), ids and converted scores [n][k], -1 / 0 past
  // the last unmasked column
  int k = 0;
  int32_t* top_ids = nullptr;
  float* top_scores = nullptr;
};
// get_triple_results in fp64 (kp_rank.hip) of the rows [r0, r0 + m) of a set, whose queries
// the family has just written into the set's chunk: rank = #{e not filtered : score_e counts
// against the target} over the frozen entities (one sequential fp64 chain over d each) plus the
// kelpie column, the target itself by the `own` rule; with the set's lists and margins (include/
// kelpie_hip.h, "Rank margins"), which change neither the ranks nor any other result
void launch_rank_f64(kp_ctx* c, const RankSet& d, int r0, int m, int act);
void launch_rank_count(kp_ctx* c, int n_slots, const float* d_scores, int ld, int n_cols,
                       const int32_t* d_pred_o, const int32_t* d_filt_off, const int32_t* d_filt,
                       int minimizer, float* d_target, int64_t* d_rank,
                       int mode = 0);

// Per-device time base: one event recorded (and completed) when the device's first
// context is created.  Hot-launch intervals of every context on the device are taken
// against it, so launches of contexts that run at once can be merged on one axis
// (kp_hot_intervals).
inline hipEvent_t kp_time_base(int device, hipStream_t stream) {
  static std::mutex mu;
  static hipEvent_t base[64] = {};
  std::lock_guard<std::mutex> lk(mu);
  if (device < 0 || device >= 64) return nullptr;
  if (!base[device]) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    if (hipEventRecord(e, stream) != hipSuccess || hipEventSynchronize(e) != hipSuccess) {
      (void)hipEventDestroy(e);
      return nullptr;
    }
    base[device] = e;
  }
  return base[device];
}

// append the [start, end] of one timed launch (events a -> b) to c->hot_iv
inline void kp_push_interval(kp_ctx* c, hipEvent_t a, hipEvent_t b) {
  const hipEvent_t t0 = kp_time_base(c->device, c->stream);
  float ms_a = 0.f, ms_b = 0.f;
  if (!t0 || hipEventElapsedTime(&ms_a, t0, a) != hipSuccess || hipEventElapsedTime(&ms_b, t0, b) != hipSuccess)
    return;
  c->hot_iv.push_back(ms_a * 1e-3);
  c->hot_iv.push_back(ms_b * 1e-3);
}
