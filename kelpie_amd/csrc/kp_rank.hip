// kp_rank.hip -- all-entity scoring (fp32 MFMA) and the filtered rank of
// PostTrainingEngine.get_triple_results (post_training_engine.py:101-125).
// The fp64 rank is one path for every set of rank rows (kp_posttrain.hpp's RankSet: the slots,
// the probes, the marks, kp_posttrain_rank_f64's slots): launch_rank_f64 ranks a range of a
// set's rows, with the set's lists and margins when it has them.  Every kernel of it states
// the per-column fp64 chain (rank64_chain), the count rule (rank64_counts, rank64_own), the
// filter-bit test (filter_bit) and the conversion to a score (rank64_score) by calling the one
// definition, so the count, its margin form, the kelpie column and the merges cannot drift
// apart; RANK64_DISPATCH turns the score kind into the kernels' MODE.
#include "kp_common.hpp"
#include "kp_margins_check.hpp"

static_assert(KP_MG_DOT == RANK64_DOT && KP_MG_SIGMOID == RANK64_SIGMOID && KP_MG_DIST == RANK64_DIST &&
                  KP_MG_DIST1 == RANK64_DIST1,
              "kp_margins_check.hpp restates launch_rank_f64's score kinds");

// ----------------------------------------------------------------------------
// score GEMM:  out[q][e] = act( Q[q] . E[e] )  for e < n_ent
//   Q [nq][dp], E [n_ent][dp] (dp multiple of 16, zero padded), out row stride ld.
//   fp32 MFMA v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain).  Block tile
//   64 queries x 64 entities x BK 32, 4 waves; wave w owns queries [16w,16w+16)
//   x 64 entities (4 accumulators).  C layout: row (query) = 4*(l>>4)+r,
//   col (entity) = l&15 -> lanes store consecutive entities (coalesced).
//   act: 0 identity (ComplEx), 1 sigmoid (ConvE, conve.py:156).
// ----------------------------------------------------------------------------
#define SG_BM 64
#define SG_BN 64
#define SG_BK 32
#define SG_LD (SG_BK + 4)

__global__ __launch_bounds__(256) void kp_gemm_abt(const float* __restrict__ A, int lda, int M,
                                                   const float* __restrict__ B, int ldb, int N, int k_begin,
                                                   int k_end, float* __restrict__ out, int ldo,
                                                   const float* __restrict__ bias, int act) {
  __shared__ __attribute__((aligned(16))) float Qs[SG_BM * SG_LD];
  __shared__ __attribute__((aligned(16))) float Es[SG_BN * SG_LD];
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int q0 = blockIdx.y * SG_BM;
  const int e0 = blockIdx.x * SG_BN;
  // split-K: blockIdx.z selects a K range and an output slab
  const int ksplit = gridDim.z;
  const int klen = (k_end - k_begin + ksplit - 1) / ksplit;
  const int kb = k_begin + blockIdx.z * ((klen + SG_BK - 1) / SG_BK * SG_BK);
  const int ke = min(k_end, kb + (klen + SG_BK - 1) / SG_BK * SG_BK);
  out += (size_t)blockIdx.z * M * ldo;
  f32x4 acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int k0 = kb; k0 < ke; k0 += SG_BK) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      int f = tid + 256 * u;
      int row = f >> 3, c4 = (f & 7) * 4;
      float4 vq = make_float4(0.f, 0.f, 0.f, 0.f), ve = vq;
      int kk = k0 + c4;
      if (q0 + row < M && kk < ke) vq = *reinterpret_cast<const float4*>(A + (size_t)(q0 + row) * lda + kk);
      if (e0 + row < N && kk < ke) ve = *reinterpret_cast<const float4*>(B + (size_t)(e0 + row) * ldb + kk);
      *reinterpret_cast<float4*>(&Qs[row * SG_LD + c4]) = vq;
      *reinterpret_cast<float4*>(&Es[row * SG_LD + c4]) = ve;
    }
    __syncthreads();
    // k permuted within each 16-deep chunk: MFMA i of a chunk pairs lane group g with
    // k = kk + 4g + i on both operands, so a lane's A and B values for four MFMAs are
    // one 16-byte LDS read each (the sum over k is unchanged, only its order)
#pragma unroll
    for (int kk = 0; kk < SG_BK; kk += 16) {
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(&Qs[(16 * w + c) * SG_LD + kk + 4 * g]);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(&Es[(16 * n + c) * SG_LD + kk + 4 * g]);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i], b4[i], acc[n], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    int e = e0 + 16 * n + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int q = q0 + 16 * w + 4 * g + r;
      if (q < M && e < N) {
        float v = acc[n][r];
        if (bias && blockIdx.z == 0) v += bias[e];
        if (act == 1) v = 1.0f / (1.0f + expf(-v));  // torch.sigmoid in float32 (accurate exp)
        out[(size_t)q * ldo + e] = v;
      }
    }
  }
}

// ----------------------------------------------------------------------------
// filtered rank, one workgroup per slot.
//   scores[s][0..n_cols) (column n_cols-1 is the kelpie entity when present)
//   minimizer: v_e = 1e6 for e in F, v_o = target, rank = #{v_e <= target}
//   maximizer: v_e = -1e6 for e in F,             rank = #{v_e >= target}
//   (post_training_engine.py:110-119; an o in F is excluded for maximizers)
// ----------------------------------------------------------------------------
// mode RANK_TRIPLE_RESULTS: PostTrainingEngine.get_triple_results (post_training_engine.py:101-125):
//   minimizer: filtered -> 1e6, o restored, count <= target; maximizer: filtered ->
//   -1e6 (o NOT restored when filtered), count >= target.
// mode RANK_PREDICT_TAILS: Model.predict_tails (model.py:42-68): filtered -> +-1e6, o
//   restored, count <= / >= target.
// mode RANK_SORT_POSITION: ConvE.predict_tails (conve.py:160-184): filtered -> 0.0, o
//   restored, rank = 1 + #(v > target), the position of o in a descending sort when
//   no other entity ties with it (torch.sort's order among ties is unspecified).
__global__ __launch_bounds__(256) void kp_rank_count(int n_slots, const float* __restrict__ scores, int ld,
                                                     int n_cols, const int32_t* __restrict__ pred_o,
                                                     const int32_t* __restrict__ filt_off,
                                                     const int32_t* __restrict__ filt, int minimizer,
                                                     float* __restrict__ target_out,
                                                     int64_t* __restrict__ rank_out, int mode) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bits[];
  __shared__ int partial[4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const int nwords = (n_cols + 31) >> 5;
  for (int i = tid; i < nwords; i += blockDim.x) bits[i] = 0u;
  __syncthreads();
  const int f0 = filt_off[s], f1 = filt_off[s + 1];
  for (int i = f0 + tid; i < f1; i += blockDim.x) {
    int e = filt[i];
    if (e >= 0 && e < n_cols) atomicOr(&bits[e >> 5], 1u << (e & 31));
  }
  __syncthreads();
  const float* row = scores + (size_t)s * ld;
  const int o = pred_o[s];
  const float target = row[o];
  int cnt = 0;
  if (minimizer) {
    for (int e = tid; e < n_cols; e += blockDim.x) {
      float v = row[e];
      if ((bits[e >> 5] >> (e & 31)) & 1u) v = 1e6f;
      if (e == o) v = target;
      cnt += (v <= target) ? 1 : 0;
    }
  } else if (mode == RANK_SORT_POSITION) {
    for (int e = tid; e < n_cols; e += blockDim.x) {
      float v = row[e];
      if ((bits[e >> 5] >> (e & 31)) & 1u) v = 0.0f;
      if (e == o) v = target;
      cnt += (v > target) ? 1 : 0;
    }
    if (tid == 0) cnt += 1;
  } else {
    for (int e = tid; e < n_cols; e += blockDim.x) {
      float v = row[e];
      if ((bits[e >> 5] >> (e & 31)) & 1u) v = -1e6f;
      if (mode == RANK_PREDICT_TAILS && e == o) v = target;
      cnt += (v >= target) ? 1 : 0;
    }
  }
  // block reduce
  for (int o2 = 32; o2 > 0; o2 >>= 1) cnt += __shfl_xor(cnt, o2, 64);
  if ((tid & 63) == 0) partial[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += partial[w];
    rank_out[s] = tot;
    target_out[s] = target;
  }
}

void launch_rank_count(kp_ctx* c, int n_slots, const float* d_scores, int ld, int n_cols,
                       const int32_t* d_pred_o, const int32_t* d_filt_off, const int32_t* d_filt,
                       int minimizer, float* d_target, int64_t* d_rank, int mode) {
  if (n_slots <= 0) return;
  size_t shm = (size_t)((n_cols + 31) / 32) * 4;
  KP_REQUIRE(shm <= 150 * 1024, "rank: too many entities for the LDS filter bitmap");
  hipLaunchKernelGGL(kp_rank_count, dim3(n_slots), dim3(256), shm, c->stream, n_slots, d_scores, ld, n_cols,
                     d_pred_o, d_filt_off, d_filt, minimizer, d_target, d_rank, mode);
  KP_HIP(hipGetLastError());
}

// ----------------------------------------------------------------------------
// fp64 filtered rank of a maximizer (ComplEx get_triple_results, post_training_engine.py:
// 101-125).  At the reference's random init the post-trained target sits among dense
// near-ties (scores ~1e-6, nearest neighbour ~1e-11 away), and an fp32 dot product over
// 400 terms with cancellation is off by ~1e-5 relative: enough to move the rank.  The
// reference's fp64 run is the exact version of the same computation, so the device
// scores in fp64 (exact products of the fp32 operands, one fp64 FMA chain over d per
// entity, the same order for the target) and compares in fp64.  No score matrix is
// written: each thread scores one entity for RQ slots and counts against their targets.
// ----------------------------------------------------------------------------
constexpr int RQ = 16;  // slots per workgroup row of the grid

// E^T [dp][ldt] (fp32, zero columns past n_ent), once per context
__global__ void kp_transpose_table(const float* __restrict__ E, int n_ent, int dp, float* __restrict__ ET, int ldt) {
  __shared__ float tile[32][33];
  const int e0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int e = e0 + i, d = d0 + tx;
    tile[i][tx] = (e < n_ent && d < dp) ? E[(size_t)e * dp + d] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int d = d0 + i, e = e0 + tx;
    if (d < dp && e < ldt) ET[(size_t)d * ldt + e] = tile[tx][i];
  }
}

// per slot: the filter bitmap over the n_ent + 1 columns (kelpie last)
__global__ __launch_bounds__(256) void kp_rank_filter_bits(int n_slots, int nwords, const int32_t* __restrict__ filt_off,
                                                           const int32_t* __restrict__ filt, int n_cols,
                                                           uint32_t* __restrict__ bits) {
  const int s = blockIdx.x;
  uint32_t* b = bits + (size_t)s * nwords;
  for (int i = threadIdx.x; i < nwords; i += blockDim.x) b[i] = 0u;
  __syncthreads();
  for (int i = filt_off[s] + threadIdx.x; i < filt_off[s + 1]; i += blockDim.x) {
    const int e = filt[i];
    if (e >= 0 && e < n_cols) atomicOr(&b[e >> 5], 1u << (e & 31));
  }
}

// torch.sigmoid on a float32 logit (conve.py:157): 1 / (1 + exp(-x)) in float32.  It
// reaches 1.0 at x ~ 16.64, so when the target's fp32 score is 1.0 the reference's rank
// counts every saturated entity as a tie, however far apart the logits are; the device
// ranks on fp64 logits and counts those ties explicitly (saturated: the float32 sigmoid
// is 1.0).  Below saturation, equal float32 scores are rounding coincidences of either
// side's logits and are not counted (the full-size fixtures: counting them moved the
// rank deltas out of the reference's own spread).
__device__ __forceinline__ bool sigmoid_f32_saturated(double x) { return 1.0f / (1.0f + expf(-(float)x)) == 1.0f; }
__device__ __forceinline__ float sigmoid_f32(double x) { return 1.0f / (1.0f + expf(-(float)x)); }

// The score kinds (`act`, the kernels' MODE).  RANK64_DOT: the scores are the fp64 values
// (ComplEx, DistMult); RANK64_SIGMOID: the scores are sigmoid(logit) and the rank compares the
// monotone logits, with a saturated target (float32 score 1.0) tied by every saturated entity
// as the reference's fp32 scores tie them (ConvE); RANK64_DIST: a minimizer whose scores are L2
// distances and the rank compares their squares (TransE: get_triple_results' minimizer branch);
// RANK64_DIST1: the same minimizer on L1 distances (TransE norm p = 1).
__device__ __forceinline__ bool rank64_minimizer(int act) { return act == RANK64_DIST || act == RANK64_DIST1; }

// is column e of row s masked by the row's filter list
__device__ __forceinline__ bool filter_bit(const uint32_t* __restrict__ bits, int nwords, int s, int e) {
  return (bits[(size_t)s * nwords + (e >> 5)] >> (e & 31)) & 1u;
}

// The count rule: does an unmasked column of compared value c count against the threshold thr
// of a row whose target's compared value is ct (the rank: thr = ct; the margins: thr_lo, thr_hi)
__device__ __forceinline__ bool rank64_counts(int act, double c, double thr, double ct) {
  if (rank64_minimizer(act)) return c <= thr;
  return c >= thr || (act == RANK64_SIGMOID && sigmoid_f32_saturated(ct) && sigmoid_f32_saturated(c));
}
// `own`: does the target's column count itself, whatever the rounding of its own score (a
// minimizer's target is restored before the count, a maximizer's filtered target is left out)
__device__ __forceinline__ bool rank64_own(int act, bool filtered) { return rank64_minimizer(act) || !filtered; }

// a compared value as the score the caller sees
__device__ __forceinline__ float rank64_score(int act, double v) {
  return act == RANK64_SIGMOID ? sigmoid_f32(v) : act == RANK64_DIST ? (float)sqrt(v) : (float)v;  // DOT, DIST1
}

// Host: runs the statements with `MODE` the compile-time constant of the score kind `act`
#define RANK64_CASE(M, ...)  \
  case M: {                  \
    constexpr int MODE = M;  \
    __VA_ARGS__;             \
  } break;
#define RANK64_DISPATCH(act, ...)                                      \
  switch (act) {                                                       \
    RANK64_CASE(RANK64_DOT, __VA_ARGS__)                               \
    RANK64_CASE(RANK64_SIGMOID, __VA_ARGS__)                           \
    RANK64_CASE(RANK64_DIST, __VA_ARGS__)                              \
    RANK64_CASE(RANK64_DIST1, __VA_ARGS__)                             \
    default: throw KpError{KP_EINVAL, "rank: unknown score kind"};     \
  }

// kelpie column and target: one thread per row (counts the kelpie column, writes the fp32
// target score).  A minimizer's target counts itself even when filtered.
__global__ void kp_rank_f64_kelpie(int n_slots, int n_ent, int nwords, const uint32_t* __restrict__ bits,
                                   const int32_t* __restrict__ pred_o, const double* __restrict__ t64,
                                   const double* __restrict__ kcol64, int act, float* __restrict__ target_out,
                                   unsigned long long* __restrict__ rank) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const bool filtered = filter_bit(bits, nwords, s, n_ent);
  rank[s] = ((rank64_minimizer(act) && pred_o[s] == n_ent) || (!filtered && rank64_counts(act, kcol64[s], t64[s], t64[s])))
                ? 1ull
                : 0ull;
  target_out[s] = rank64_score(act, t64[s]);
}

// ----------------------------------------------------------------------------
// top-k tails (kp_posttrain_rank_topk): the k best unmasked columns of every slot, from the
// values the rank compares.  A column's sort key is its fp64 value mapped to an unsigned
// integer whose order is the value's (reversed for maximizers), so a smaller key is a
// better column for every kind; keys tie only on equal values, and the lower column wins.
// Masked or absent entries carry column -1 (as unsigned the largest: they sort last).
// ----------------------------------------------------------------------------
constexpr int TOPK_MAX = 32;
__device__ __forceinline__ unsigned long long topk_key(double v, bool minimizer) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v + 0.0);  // -0 -> +0
  const unsigned long long asc = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  return minimizer ? asc : ~asc;
}
__device__ __forceinline__ double topk_value(unsigned long long key, bool minimizer) {
  const unsigned long long asc = minimizer ? key : ~key;
  const unsigned long long u = (asc >> 63) ? (asc & 0x7fffffffffffffffull) : ~asc;
  return __longlong_as_double((long long)u);
}
// (key, column) order: a before b
__device__ __forceinline__ bool topk_before(unsigned long long ka, uint32_t ca, unsigned long long kb, uint32_t cb) {
  return ka < kb || (ka == kb && ca < cb);
}

// MODE: RANK64_DOT (dot products, maximizer), RANK64_SIGMOID (dot products = logits, with
// the saturated float32 sigmoid ties), RANK64_DIST (squared L2), RANK64_DIST1 (L1).
// TOPK: after the count, every wave sorts its 64 columns of each slot by (key, column)
// across its lanes (a bitonic network of shuffles: no atomics, no LDS) and its first k
// lanes write the wave's list [k] into top.cand_key / cand_col [slot][4 gridDim.x][k].  The
// target's column carries t64, the value the count compares the others with.  Without TOPK
// `top` is empty and the kernel is the count alone.
template <bool TOPK>
struct TopkArgs {};
template <>
struct TopkArgs<true> {
  int k;
  unsigned long long* cand_key;
  int32_t* cand_col;
};

// The per-column fp64 chain: v[j] for the rows s0 + j, j < ns, of this thread's column e of
// E^T, one sequential chain over d per (row, column).  The rows q [ns][dp] are wave-uniform
// (scalar loads).  The count and its margin form both call this, so with tol = 0 the margins'
// band is the rank bit for bit.  (Returned by value: accumulators handed over by reference
// cost both kernels registers, 72 against 45 and 59.)
struct Rank64Acc {
  double v[RQ];
};
template <int MODE>
__device__ __forceinline__ Rank64Acc rank64_chain(const double* __restrict__ q, int dp, int ns,
                                                  const float* __restrict__ ET, int ldt, int e) {
  Rank64Acc acc;
#pragma unroll
  for (int j = 0; j < RQ; ++j) acc.v[j] = 0.0;
  for (int d = 0; d < dp; ++d) {
    const double v = (double)ET[(size_t)d * ldt + e];
#pragma unroll
    for (int j = 0; j < RQ; ++j)
      if (j < ns) {
        if constexpr (MODE == RANK64_DIST) {
          const double df = q[(size_t)j * dp + d] - v;  // exact: fp32 operands, fp64 difference
          acc.v[j] = __fma_rn(df, df, acc.v[j]);
        } else if constexpr (MODE == RANK64_DIST1) {
          acc.v[j] += fabs(q[(size_t)j * dp + d] - v);
        } else {
          acc.v[j] = __fma_rn(q[(size_t)j * dp + d], v, acc.v[j]);
        }
      }
  }
  return acc;
}

template <int MODE, bool TOPK = false>
__global__ __launch_bounds__(256) void kp_rank_f64_count(int n_slots, int n_ent, int dp, const double* __restrict__ Q,
                                                         const double* __restrict__ t64,
                                                         const int32_t* __restrict__ pred_o, const float* __restrict__ ET,
                                                         int ldt, int nwords, const uint32_t* __restrict__ bits,
                                                         unsigned long long* __restrict__ rank, TopkArgs<TOPK> top) {
  __shared__ int part[4][RQ];
  const int s0 = blockIdx.y * RQ;
  const int e = blockIdx.x * 256 + threadIdx.x;  // < ldt: ET is zero-padded
  const int ns = min(RQ, n_slots - s0);
  const Rank64Acc chain = rank64_chain<MODE>(Q + (size_t)s0 * dp, dp, ns, ET, ldt, e);
  const double(&acc)[RQ] = chain.v;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < RQ; ++j) {
    int hit = 0;
    if (j < ns && e < n_ent) {
      const int s = s0 + j;
      const bool filtered = filter_bit(bits, nwords, s, e);
      hit = e == pred_o[s] ? rank64_own(MODE, filtered) : !filtered && rank64_counts(MODE, acc[j], t64[s], t64[s]);
    }
    for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);
    if (lane == 0) part[w][j] = hit;
  }
  __syncthreads();
  if (threadIdx.x < ns) {
    const int j = threadIdx.x;
    const int tot = part[0][j] + part[1][j] + part[2][j] + part[3][j];
    if (tot) atomicAdd(&rank[s0 + j], (unsigned long long)tot);
  }
  if constexpr (TOPK) {
    constexpr bool MINI = MODE == RANK64_DIST || MODE == RANK64_DIST1;  // rank64_minimizer(MODE)
    const size_t lists = (size_t)4 * gridDim.x;
#pragma unroll
    for (int j = 0; j < RQ; ++j) {
      if (j < ns) {  // block-uniform
        const int s = s0 + j;
        unsigned long long key = ~0ull;
        uint32_t col = 0xffffffffu;
        if (e < n_ent) {
          const bool filtered = filter_bit(bits, nwords, s, e);
          const bool is_o = e == pred_o[s];
          if (!filtered || (MINI && is_o)) {  // a minimizer's filtered target is restored
            key = topk_key(is_o ? t64[s] : acc[j], MINI);
            col = (uint32_t)e;
          }
        }
        // ascending bitonic sort of the wave's 64 (key, column) pairs over its lanes
#pragma unroll
        for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
          for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const unsigned long long pk = __shfl_xor(key, stride, 64);
            const uint32_t pc = __shfl_xor(col, stride, 64);
            const bool want_min = ((lane & stride) == 0) == ((lane & size) == 0);
            // distinct pairs: exactly one is before the other; equal pairs (absent entries) swap freely
            const bool take = topk_before(pk, pc, key, col) == want_min;
            key = take ? pk : key;
            col = take ? pc : col;
          }
        }
        if (lane < top.k) {
          const size_t at = ((size_t)s * lists + (size_t)4 * blockIdx.x + w) * top.k + lane;
          top.cand_key[at] = key;
          top.cand_col[at] = (int32_t)col;
        }
      }
    }
  }
}

// merge of a slot's `lists` sorted wave lists [lists][k] plus the kelpie column into its final
// list, one workgroup per slot.  The k best heads (first entries) name the only lists that
// can hold one of the k best columns (a list whose head is not among the k best heads has k
// better columns before any of its own), so: pick the k best heads, load those lists (at
// most k * k entries), pick the k best of them.  Each pick is the block's minimum of
// (key, column) after the previous pick: comparisons only, the same result on every run.
__device__ __forceinline__ void topk_block_min(unsigned long long& key, uint32_t& col, uint32_t& pay,
                                               unsigned long long* sk, uint32_t* sc, uint32_t* sp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long pk = __shfl_xor(key, o, 64);
    const uint32_t pc = __shfl_xor(col, o, 64);
    const uint32_t pp = __shfl_xor(pay, o, 64);
    if (topk_before(pk, pc, key, col)) key = pk, col = pc, pay = pp;
  }
  __syncthreads();  // the previous round's readers are done with sk / sc / sp
  if (lane == 0) sk[w] = key, sc[w] = col, sp[w] = pay;
  __syncthreads();
  key = sk[0], col = sc[0], pay = sp[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (topk_before(sk[i], sc[i], key, col)) key = sk[i], col = sc[i], pay = sp[i];
}

__global__ __launch_bounds__(256) void kp_rank_topk_merge(int n_ent, int nwords, int lists, int k, int act,
                                                          const unsigned long long* __restrict__ cand_key,
                                                          const int32_t* __restrict__ cand_col,
                                                          const uint32_t* __restrict__ bits,
                                                          const int32_t* __restrict__ pred_o,
                                                          const double* __restrict__ t64,
                                                          const double* __restrict__ kcol64, int32_t* __restrict__ out_ids,
                                                          float* __restrict__ out_scores) {
  __shared__ unsigned long long sk[4];
  __shared__ uint32_t sc[4], sp[4];
  __shared__ int pick[TOPK_MAX];                          // the chosen lists (-1: none)
  __shared__ unsigned long long lk[TOPK_MAX * TOPK_MAX];  // their entries
  __shared__ uint32_t lc[TOPK_MAX * TOPK_MAX];
  const int s = blockIdx.x, tid = threadIdx.x;
  const bool mini = rank64_minimizer(act);
  const unsigned long long* ck = cand_key + (size_t)s * lists * k;
  const int32_t* cc = cand_col + (size_t)s * lists * k;
  // phase 1: the k best heads
  unsigned long long last_k = 0;
  uint32_t last_c = 0;
  for (int r = 0; r < k; ++r) {
    unsigned long long bk = ~0ull;
    uint32_t bc = 0xffffffffu, bl = 0xffffffffu;
    for (int l = tid; l < lists; l += 256) {
      const unsigned long long hk = ck[(size_t)l * k];
      const uint32_t hc = (uint32_t)cc[(size_t)l * k];
      if (hc != 0xffffffffu && (r == 0 || topk_before(last_k, last_c, hk, hc)) && topk_before(hk, hc, bk, bc))
        bk = hk, bc = hc, bl = (uint32_t)l;
    }
    topk_block_min(bk, bc, bl, sk, sc, sp);
    if (tid == 0) pick[r] = bc == 0xffffffffu ? -1 : (int)bl;
    last_k = bk, last_c = bc;
    // once the heads run out every later pick is empty too (bc stays -1: nothing is after it)
  }
  __syncthreads();
  // phase 2: the chosen lists' entries, and the kelpie column as one more entry
  for (int i = tid; i < k * k; i += 256) {
    const int l = pick[i / k];
    lk[i] = l < 0 ? ~0ull : ck[(size_t)l * k + i % k];
    lc[i] = l < 0 ? 0xffffffffu : (uint32_t)cc[(size_t)l * k + i % k];
  }
  const bool kfilt = filter_bit(bits, nwords, s, n_ent);
  const bool k_is_o = pred_o[s] == n_ent;
  const bool k_in = !kfilt || (mini && k_is_o);
  const unsigned long long kk = k_in ? topk_key(k_is_o ? t64[s] : kcol64[s], mini) : ~0ull;
  const uint32_t kc = k_in ? (uint32_t)n_ent : 0xffffffffu;
  __syncthreads();
  for (int r = 0; r < k; ++r) {
    unsigned long long bk = ~0ull;
    uint32_t bc = 0xffffffffu, bp = 0;
    for (int i = tid; i <= k * k; i += 256) {
      const unsigned long long ek = i < k * k ? lk[i] : kk;
      const uint32_t ec = i < k * k ? lc[i] : kc;
      if (ec != 0xffffffffu && (r == 0 || topk_before(last_k, last_c, ek, ec)) && topk_before(ek, ec, bk, bc))
        bk = ek, bc = ec;
    }
    topk_block_min(bk, bc, bp, sk, sc, sp);
    if (tid == 0) {
      out_ids[(size_t)s * k + r] = (int32_t)bc;
      out_scores[(size_t)s * k + r] = bc != 0xffffffffu ? rank64_score(act, topk_value(bk, mini)) : 0.f;
    }
    last_k = bk, last_c = bc;
  }
}

// ----------------------------------------------------------------------------
// rank margins (kp_posttrain_rank_margins; include/kelpie_hip.h, "Rank margins"): per rank row
// the band [rank_lo, rank_hi] of the rank under a tolerance on the compared values, the exact
// ties and the nearest better / worse column.  Three launches after the row's own count, none
// with an atomic: the thresholds (one thread per row, kp_margins_check.hpp's rule), the margin
// form of the count (the count's grid and its fp64 chain per column, so c_e is the value the
// rank compared; every workgroup leaves its counts and its nearest (key, column) pairs of each
// row in the workspace) and the merge (one wave per row: the workgroups' partials in a fixed
// order, the kelpie column, `own`).  A nearest pair's key orders like topk_key on the worse
// side and reversed on the better side, so both sides take the minimum by topk_before: the
// closest value, the lower column among equal ones.
// ----------------------------------------------------------------------------
constexpr uint32_t MG_NONE = 0xffffffffu;

__global__ void kp_rank_margin_thr(int n, int act, const double* __restrict__ t64, double tol,
                                   double* __restrict__ thr) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  double lo, hi;
  kp_margin_thresholds(act, t64[s], tol, &lo, &hi);
  thr[2 * s] = lo;
  thr[2 * s + 1] = hi;
}

// one unmasked column other than the target, of value c at column e, against a row's target ct
// and thresholds: its counts (lo | hi << 8 | tie << 16) and, when it is strictly better /
// worse than the target, its candidate pair for that side (written over what the caller
// passed: a caller that holds a candidate already merges by topk_before)
__device__ __forceinline__ int margin_column(int act, double c, uint32_t e, double ct, double thr_lo, double thr_hi,
                                             unsigned long long& bk, uint32_t& bc, unsigned long long& wk,
                                             uint32_t& wc) {
  const bool mini = rank64_minimizer(act);
  const bool lo = rank64_counts(act, c, thr_lo, ct);
  const bool hi = rank64_counts(act, c, thr_hi, ct);
  const unsigned long long k = topk_key(c, mini);
  if (mini ? c < ct : c > ct) bk = ~k, bc = e;
  if (mini ? c > ct : c < ct) wk = k, wc = e;
  return (lo ? 1 : 0) | (hi ? 1 << 8 : 0) | (c == ct ? 1 << 16 : 0);
}

// the minimum (key, column) pair over the wave's lanes, in every lane
__device__ __forceinline__ void margin_wave_min(unsigned long long& key, uint32_t& col) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long pk = __shfl_xor(key, o, 64);
    const uint32_t pc = __shfl_xor(col, o, 64);
    if (topk_before(pk, pc, key, col)) key = pk, col = pc;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void kp_rank_f64_margin(int n_slots, int n_ent, int dp, const double* __restrict__ Q,
                                                          const double* __restrict__ t64,
                                                          const int32_t* __restrict__ pred_o,
                                                          const float* __restrict__ ET, int ldt, int nwords,
                                                          const uint32_t* __restrict__ bits,
                                                          const double* __restrict__ thr,
                                                          unsigned long long* __restrict__ pkey,
                                                          int32_t* __restrict__ pcol, int32_t* __restrict__ pcnt) {
  __shared__ int cnt_s[4][RQ];
  __shared__ unsigned long long key_s[4][RQ][2];
  __shared__ uint32_t col_s[4][RQ][2];
  const int s0 = blockIdx.y * RQ;
  const int e = blockIdx.x * 256 + threadIdx.x;  // < ldt: ET is zero-padded
  const int ns = min(RQ, n_slots - s0);
  const Rank64Acc chain = rank64_chain<MODE>(Q + (size_t)s0 * dp, dp, ns, ET, ldt, e);
  const double(&acc)[RQ] = chain.v;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < RQ; ++j) {
    if (j < ns) {  // block-uniform
      const int s = s0 + j;
      int cnt = 0;
      unsigned long long bk = ~0ull, wk = ~0ull;
      uint32_t bc = MG_NONE, wc = MG_NONE;
      if (e < n_ent && e != pred_o[s]) {
        if (!filter_bit(bits, nwords, s, e))
          cnt = margin_column(MODE, acc[j], (uint32_t)e, t64[s], thr[2 * s], thr[2 * s + 1], bk, bc, wk, wc);
      }
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);  // three fields of at most 64 each
      margin_wave_min(bk, bc);
      margin_wave_min(wk, wc);
      if (lane == 0) {
        cnt_s[w][j] = cnt;
        key_s[w][j][0] = bk, col_s[w][j][0] = bc;
        key_s[w][j][1] = wk, col_s[w][j][1] = wc;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * ns) {  // thread (j, side): the four waves' partials in wave order
    const int j = threadIdx.x >> 1, side = threadIdx.x & 1;
    const size_t at = (size_t)(s0 + j) * gridDim.x + blockIdx.x;
    unsigned long long k = key_s[0][j][side];
    uint32_t c = col_s[0][j][side];
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (topk_before(key_s[i][j][side], col_s[i][j][side], k, c)) k = key_s[i][j][side], c = col_s[i][j][side];
    pkey[2 * at + side] = k;
    pcol[2 * at + side] = (int32_t)c;
    if (side == 0) {
      int lo = 0, hi = 0, ties = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        lo += cnt_s[i][j] & 0xff, hi += (cnt_s[i][j] >> 8) & 0xff, ties += cnt_s[i][j] >> 16;
      }
      pcnt[3 * at] = lo, pcnt[3 * at + 1] = hi, pcnt[3 * at + 2] = ties;
    }
  }
}

// one wave per row: the row's nblk partials, the kelpie column and `own` into its margins
__global__ __launch_bounds__(64) void kp_rank_margin_merge(int n_ent, int nwords, int nblk, int act,
                                                           const uint32_t* __restrict__ bits,
                                                           const int32_t* __restrict__ pred_o,
                                                           const double* __restrict__ t64,
                                                           const double* __restrict__ kcol64,
                                                           const double* __restrict__ thr,
                                                           const unsigned long long* __restrict__ pkey,
                                                           const int32_t* __restrict__ pcol,
                                                           const int32_t* __restrict__ pcnt, MarginDev out) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const bool mini = rank64_minimizer(act);
  long long lo = 0, hi = 0, ties = 0;
  unsigned long long bk = ~0ull, wk = ~0ull;
  uint32_t bc = MG_NONE, wc = MG_NONE;
  for (int b = lane; b < nblk; b += 64) {
    const size_t at = (size_t)s * nblk + b;
    lo += pcnt[3 * at], hi += pcnt[3 * at + 1], ties += pcnt[3 * at + 2];
    if (topk_before(pkey[2 * at], (uint32_t)pcol[2 * at], bk, bc)) bk = pkey[2 * at], bc = (uint32_t)pcol[2 * at];
    if (topk_before(pkey[2 * at + 1], (uint32_t)pcol[2 * at + 1], wk, wc))
      wk = pkey[2 * at + 1], wc = (uint32_t)pcol[2 * at + 1];
  }
  const double ct = t64[s];
  const int o = pred_o[s];
  if (lane == 0) {
    if (o != n_ent && !filter_bit(bits, nwords, s, n_ent)) {  // the kelpie column, unless it is the target or masked
      unsigned long long kbk = ~0ull, kwk = ~0ull;
      uint32_t kbc = MG_NONE, kwc = MG_NONE;
      const int cnt =
          margin_column(act, kcol64[s], (uint32_t)n_ent, ct, thr[2 * s], thr[2 * s + 1], kbk, kbc, kwk, kwc);
      lo += cnt & 0xff, hi += (cnt >> 8) & 0xff, ties += cnt >> 16;
      if (topk_before(kbk, kbc, bk, bc)) bk = kbk, bc = kbc;  // one more candidate of this lane's
      if (topk_before(kwk, kwc, wk, wc)) wk = kwk, wc = kwc;
    }
    const int own = rank64_own(act, filter_bit(bits, nwords, s, o)) ? 1 : 0;  // the target column itself
    lo += own, hi += own;
  }
  for (int d = 32; d > 0; d >>= 1) {
    lo += __shfl_xor(lo, d, 64), hi += __shfl_xor(hi, d, 64), ties += __shfl_xor(ties, d, 64);
  }
  margin_wave_min(bk, bc);
  margin_wave_min(wk, wc);
  if (lane != 0) return;
  const double vt = kp_margin_units(act, ct);
  if (out.rank_lo) out.rank_lo[s] = lo;
  if (out.rank_hi) out.rank_hi[s] = hi;
  if (out.ties) out.ties[s] = ties;
  if (out.id_better) out.id_better[s] = (int32_t)bc;
  if (out.id_worse) out.id_worse[s] = (int32_t)wc;
  if (out.gap_better)
    out.gap_better[s] = bc == MG_NONE ? (double)INFINITY : fabs(kp_margin_units(act, topk_value(~bk, mini)) - vt);
  if (out.gap_worse)
    out.gap_worse[s] = wc == MG_NONE ? (double)INFINITY : fabs(kp_margin_units(act, topk_value(wk, mini)) - vt);
}

// bytes of candidate workspace a launch may hold: the slots run in chunks of whole slot rows
constexpr size_t TOPK_WS_BYTES = (size_t)64 << 20;

// Rank the rows [r0, r0 + m) of a set (m <= d.chunk; their fp64 rows, target and kelpie column
// scores are in d.q / d.t / d.kcol): the filter bitmaps, the kelpie column and the target
// scores, the rows' margins when the set has them (three launches, none with an atomic: the
// thresholds, the margin form of the count, the merge of its per-workgroup partials), then the
// count -- with the set's lists (d.k > 0, the whole set at once) in chunks of whole workgroup
// rows that keep the waves' candidate lists within TOPK_WS_BYTES, each followed by its merge.
void launch_rank_f64(kp_ctx* c, const RankSet& d, int r0, int m, int act) {
  if (m <= 0) return;
  KP_REQUIRE(m <= d.chunk && (d.k == 0 || (r0 == 0 && m == d.n)), "rank: the set does not hold this launch");
  const int ldt = (c->n_ent + 255) / 256 * 256;
  if (!c->eT_ready) {
    float* ET = ensure_n<float>(c->eT, (size_t)c->dp * ldt);
    hipLaunchKernelGGL(kp_transpose_table, dim3(ldt / 32, (c->dp + 31) / 32), dim3(256), 0, c->stream, c->dE,
                       c->n_ent, c->dp, ET, ldt);
    KP_HIP(hipGetLastError());
    c->eT_ready = true;
  }
  const float* ET = c->eT.as<float>();
  const int n_cols = c->n_ent + 1;
  const int nwords = (n_cols + 31) / 32;
  const int32_t* po = d.po + r0;
  unsigned long long* rank = reinterpret_cast<unsigned long long*>(d.rank + r0);
  hipLaunchKernelGGL(kp_rank_filter_bits, dim3(m), dim3(256), 0, c->stream, m, nwords, d.filt_off + r0, d.filt, n_cols,
                     d.bits);
  KP_HIP(hipGetLastError());
  hipLaunchKernelGGL(kp_rank_f64_kelpie, dim3((m + 63) / 64), dim3(64), 0, c->stream, m, c->n_ent, nwords, d.bits, po,
                     d.t, d.kcol, act, d.target + r0, rank);
  KP_HIP(hipGetLastError());
  if (d.mg.cap > 0) {
    const MarginDev mg = d.mg.at((size_t)r0);
    const int nblk = ldt / 256;
    KP_REQUIRE(m <= mg.cap && nblk == mg.nblk, "margins: the workspace does not hold this launch");
    hipLaunchKernelGGL(kp_rank_margin_thr, dim3((m + 63) / 64), dim3(64), 0, c->stream, m, act, d.t, mg.tol, mg.thr);
    KP_HIP(hipGetLastError());
    RANK64_DISPATCH(act, hipLaunchKernelGGL(kp_rank_f64_margin<MODE>, dim3(nblk, (m + RQ - 1) / RQ), dim3(256), 0,
                                            c->stream, m, c->n_ent, c->dp, d.q, d.t, po, ET, ldt, nwords, d.bits,
                                            mg.thr, mg.pkey, mg.pcol, mg.pcnt));
    KP_HIP(hipGetLastError());
    hipLaunchKernelGGL(kp_rank_margin_merge, dim3(m), dim3(64), 0, c->stream, c->n_ent, nwords, nblk, act, d.bits, po,
                       d.t, d.kcol, mg.thr, mg.pkey, mg.pcol, mg.pcnt, mg);
    KP_HIP(hipGetLastError());
  }
  if (d.k == 0) {
    RANK64_DISPATCH(act, hipLaunchKernelGGL(kp_rank_f64_count<MODE>, dim3(ldt / 256, (m + RQ - 1) / RQ), dim3(256), 0,
                                            c->stream, m, c->n_ent, c->dp, d.q, d.t, po, ET, ldt, nwords, d.bits, rank,
                                            TopkArgs<false>{}));
    KP_HIP(hipGetLastError());
    return;
  }
  // every wave of the scoring grid leaves a list of k candidates per slot (12 bytes each)
  const int lists = 4 * (ldt / 256);
  const size_t per_slot = (size_t)lists * d.k;  // candidates
  const int rows_fit = (int)std::max<size_t>(1, TOPK_WS_BYTES / (per_slot * 12 * RQ));
  const int chunk = std::min(m, rows_fit * RQ);
  unsigned long long* ck = ensure_n<unsigned long long>(c->rank.cand_key, per_slot * chunk);
  int32_t* cc = ensure_n<int32_t>(c->rank.cand_col, per_slot * chunk);
  for (int s0 = 0; s0 < m; s0 += chunk) {
    const int ms = std::min(chunk, m - s0);
    const uint32_t* b = d.bits + (size_t)s0 * nwords;
    RANK64_DISPATCH(act, hipLaunchKernelGGL((kp_rank_f64_count<MODE, true>), dim3(ldt / 256, (ms + RQ - 1) / RQ),
                                            dim3(256), 0, c->stream, ms, c->n_ent, c->dp, d.q + (size_t)s0 * c->dp,
                                            d.t + s0, po + s0, ET, ldt, nwords, b, rank + s0,
                                            TopkArgs<true>{d.k, ck, cc}));
    KP_HIP(hipGetLastError());
    hipLaunchKernelGGL(kp_rank_topk_merge, dim3(ms), dim3(256), 0, c->stream, c->n_ent, nwords, lists, d.k, act, ck, cc,
                       b, po + s0, d.t + s0, d.kcol + s0, d.top_ids + (size_t)s0 * d.k, d.top_scores + (size_t)s0 * d.k);
    KP_HIP(hipGetLastError());
  }
}

void launch_gemm_abt(kp_ctx* c, const float* A, int lda, int M, const float* B, int ldb, int N, int K, float* out,
                     int ldo, const float* bias, int act, int ksplit) {
  if (M <= 0 || N <= 0) return;
  KP_REQUIRE(K % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0, "gemm: K and leading dims must be multiples of 4");
  dim3 grid((N + SG_BN - 1) / SG_BN, (M + SG_BM - 1) / SG_BM, std::max(1, ksplit));
  hipLaunchKernelGGL(kp_gemm_abt, grid, dim3(256), 0, c->stream, A, lda, M, B, ldb, N, 0, K, out, ldo, bias, act);
  KP_HIP(hipGetLastError());
}

void launch_score_gemm(kp_ctx* c, const float* dQ, int nq, float* d_out, int ld, int act) {
  launch_gemm_abt(c, dQ, c->dp, nq, c->dE, c->dp, c->n_ent, c->dp, d_out, ld, nullptr, act, 1);
}

// ----------------------------------------------------------------------------
// conversion-entity test of RelevanceEngine.select_entities_to_convert
// (engine.py:103-120), one workgroup per candidate head: keep iff the target's
// raw score lies strictly inside (-1e6, max of the filter-masked row) for
// maximizers, or inside (min, 1e6) for minimizers.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kp_convertible_reduce(int n, const float* __restrict__ scores, int ld,
                                                             int n_ent, int obj,
                                                             const int32_t* __restrict__ filt_off,
                                                             const int32_t* __restrict__ filt, int minimizer,
                                                             uint8_t* __restrict__ keep) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bits[];
  __shared__ float part[4];
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  const int nwords = (n_ent + 31) >> 5;
  for (int k = tid; k < nwords; k += blockDim.x) bits[k] = 0u;
  __syncthreads();
  for (int k = filt_off[i] + tid; k < filt_off[i + 1]; k += blockDim.x) {
    int e = filt[k];
    if (e >= 0 && e < n_ent) atomicOr(&bits[e >> 5], 1u << (e & 31));
  }
  __syncthreads();
  const float* row = scores + (size_t)i * ld;
  const float t = row[obj];
  float ext = minimizer ? 3.0e38f : -3.0e38f;
  for (int e = tid; e < n_ent; e += blockDim.x) {
    float v = row[e];
    if ((bits[e >> 5] >> (e & 31)) & 1u) v = minimizer ? 1e6f : -1e6f;
    ext = minimizer ? fminf(ext, v) : fmaxf(ext, v);
  }
  for (int o = 32; o > 0; o >>= 1) {
    float other = __shfl_xor(ext, o, 64);
    ext = minimizer ? fminf(ext, other) : fmaxf(ext, other);
  }
  if ((tid & 63) == 0) part[tid >> 6] = ext;
  __syncthreads();
  if (tid == 0) {
    float e2 = part[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) e2 = minimizer ? fminf(e2, part[w]) : fmaxf(e2, part[w]);
    keep[i] = minimizer ? ((1e6f > t && t > e2) ? 1 : 0) : ((-1e6f < t && t < e2) ? 1 : 0);
  }
}

void launch_convertible_reduce(kp_ctx* c, int n, const float* d_scores, int ld, int obj, const int32_t* d_fo,
                               const int32_t* d_f, int minimizer, uint8_t* d_keep) {
  if (n <= 0) return;
  size_t shm = (size_t)((c->n_ent + 31) / 32) * 4;
  KP_REQUIRE(shm <= 150 * 1024, "convertible: too many entities for the LDS filter bitmap");
  hipLaunchKernelGGL(kp_convertible_reduce, dim3(n), dim3(256), shm, c->stream, n, d_scores, ld, c->n_ent, obj, d_fo,
                     d_f, minimizer, d_keep);
  KP_HIP(hipGetLastError());
}
