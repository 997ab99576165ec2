// kp_rank.hip -- all-entity scoring (fp32 MFMA) and the filtered rank of
// PostTrainingEngine.get_triple_results (post_training_engine.py:101-125).
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

// kelpie column and target: one thread per slot (counts the kelpie column, writes the
// fp32 target score)
// act RANK64_DOT: the scores are the fp64 values (ComplEx); RANK64_SIGMOID: the scores
// are sigmoid(logit) and the rank compares the monotone logits, with a saturated target
// (float32 score 1.0) tied by every saturated entity as the reference's fp32 scores tie
// them (ConvE); RANK64_DIST: a
// minimizer whose scores are L2 distances and the rank compares their squares (TransE:
// get_triple_results' minimizer branch, the target counting itself even when filtered);
// RANK64_DIST1: the same minimizer on L1 distances (TransE norm p = 1)
__global__ void kp_rank_f64_kelpie(int n_slots, int n_ent, int nwords, const uint32_t* __restrict__ bits,
                                   const int32_t* __restrict__ pred_o, const double* __restrict__ t64,
                                   const double* __restrict__ kcol64, int act, float* __restrict__ target_out,
                                   unsigned long long* __restrict__ rank) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const bool filtered = (bits[(size_t)s * nwords + (n_ent >> 5)] >> (n_ent & 31)) & 1u;
  if (act == RANK64_DIST || act == RANK64_DIST1)
    rank[s] = (pred_o[s] == n_ent || (!filtered && kcol64[s] <= t64[s])) ? 1ull : 0ull;
  else if (act == RANK64_SIGMOID)
    rank[s] = (!filtered && (kcol64[s] >= t64[s] || (sigmoid_f32_saturated(t64[s]) && sigmoid_f32_saturated(kcol64[s]))))
                  ? 1ull
                  : 0ull;
  else
    rank[s] = (!filtered && kcol64[s] >= t64[s]) ? 1ull : 0ull;
  target_out[s] = act == RANK64_SIGMOID ? sigmoid_f32(t64[s])
                  : act == RANK64_DIST  ? (float)sqrt(t64[s])
                                        : (float)t64[s];  // DOT, DIST1
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
  double acc[RQ];
#pragma unroll
  for (int j = 0; j < RQ; ++j) acc[j] = 0.0;
  // the slot rows are wave-uniform: scalar loads, one fp64 FMA chain over d per (slot, entity)
  const double* q = Q + (size_t)s0 * dp;
  for (int d = 0; d < dp; ++d) {
    const double v = (double)ET[(size_t)d * ldt + e];
#pragma unroll
    for (int j = 0; j < RQ; ++j)
      if (j < ns) {
        if constexpr (MODE == RANK64_DIST) {
          const double df = q[(size_t)j * dp + d] - v;  // exact: fp32 operands, fp64 difference
          acc[j] = __fma_rn(df, df, acc[j]);
        } else if constexpr (MODE == RANK64_DIST1) {
          acc[j] += fabs(q[(size_t)j * dp + d] - v);
        } else {
          acc[j] = __fma_rn(q[(size_t)j * dp + d], v, acc[j]);
        }
      }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < RQ; ++j) {
    int hit = 0;
    if (j < ns && e < n_ent) {
      const int s = s0 + j;
      const bool filtered = (bits[(size_t)s * nwords + (e >> 5)] >> (e & 31)) & 1u;
      // the target counts itself whatever the rounding of its own score (a maximizer's
      // only if unfiltered: its filtered score is set back after the count)
      if constexpr (MODE == RANK64_DIST || MODE == RANK64_DIST1)
        hit = e == pred_o[s] || (!filtered && acc[j] <= t64[s]);
      else if constexpr (MODE == RANK64_SIGMOID)
        hit = !filtered && (e == pred_o[s] || acc[j] >= t64[s] ||
                            (sigmoid_f32_saturated(t64[s]) && sigmoid_f32_saturated(acc[j])));
      else
        hit = !filtered && (e == pred_o[s] || acc[j] >= t64[s]);
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
    constexpr bool MINI = MODE == RANK64_DIST || MODE == RANK64_DIST1;
    const size_t lists = (size_t)4 * gridDim.x;
#pragma unroll
    for (int j = 0; j < RQ; ++j) {
      if (j < ns) {  // block-uniform
        const int s = s0 + j;
        unsigned long long key = ~0ull;
        uint32_t col = 0xffffffffu;
        if (e < n_ent) {
          const bool filtered = (bits[(size_t)s * nwords + (e >> 5)] >> (e & 31)) & 1u;
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
  const bool mini = act == RANK64_DIST || act == RANK64_DIST1;
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
  const bool kfilt = (bits[(size_t)s * nwords + (n_ent >> 5)] >> (n_ent & 31)) & 1u;
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
      float sc32 = 0.f;
      if (bc != 0xffffffffu) {
        const double v = topk_value(bk, mini);
        sc32 = act == RANK64_SIGMOID ? sigmoid_f32(v) : act == RANK64_DIST ? (float)sqrt(v) : (float)v;
      }
      out_ids[(size_t)s * k + r] = (int32_t)bc;
      out_scores[(size_t)s * k + r] = sc32;
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
                                             bool t_sat, unsigned long long& bk, uint32_t& bc,
                                             unsigned long long& wk, uint32_t& wc) {
  const bool mini = act == RANK64_DIST || act == RANK64_DIST1;
  bool lo = mini ? c <= thr_lo : c >= thr_lo;
  bool hi = mini ? c <= thr_hi : c >= thr_hi;
  if (act == RANK64_SIGMOID && t_sat && sigmoid_f32_saturated(c)) lo = hi = true;
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
  double acc[RQ];
#pragma unroll
  for (int j = 0; j < RQ; ++j) acc[j] = 0.0;
  // kp_rank_f64_count's chain, operation for operation: the same c_e
  const double* q = Q + (size_t)s0 * dp;
  for (int d = 0; d < dp; ++d) {
    const double v = (double)ET[(size_t)d * ldt + e];
#pragma unroll
    for (int j = 0; j < RQ; ++j)
      if (j < ns) {
        if constexpr (MODE == RANK64_DIST) {
          const double df = q[(size_t)j * dp + d] - v;
          acc[j] = __fma_rn(df, df, acc[j]);
        } else if constexpr (MODE == RANK64_DIST1) {
          acc[j] += fabs(q[(size_t)j * dp + d] - v);
        } else {
          acc[j] = __fma_rn(q[(size_t)j * dp + d], v, acc[j]);
        }
      }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < RQ; ++j) {
    if (j < ns) {  // block-uniform
      const int s = s0 + j;
      int cnt = 0;
      unsigned long long bk = ~0ull, wk = ~0ull;
      uint32_t bc = MG_NONE, wc = MG_NONE;
      if (e < n_ent && e != pred_o[s]) {
        const bool filtered = (bits[(size_t)s * nwords + (e >> 5)] >> (e & 31)) & 1u;
        if (!filtered) {
          const double ct = t64[s];
          const bool t_sat = MODE == RANK64_SIGMOID && sigmoid_f32_saturated(ct);
          cnt = margin_column(MODE, acc[j], (uint32_t)e, ct, thr[2 * s], thr[2 * s + 1], t_sat, bk, bc, wk, wc);
        }
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
  const bool mini = act == RANK64_DIST || act == RANK64_DIST1;
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
    const bool kfilt = (bits[(size_t)s * nwords + (n_ent >> 5)] >> (n_ent & 31)) & 1u;
    if (o != n_ent && !kfilt) {  // the kelpie column, unless it is the target or masked
      const bool t_sat = act == RANK64_SIGMOID && sigmoid_f32_saturated(ct);
      unsigned long long kbk = ~0ull, kwk = ~0ull;
      uint32_t kbc = MG_NONE, kwc = MG_NONE;
      const int cnt =
          margin_column(act, kcol64[s], (uint32_t)n_ent, ct, thr[2 * s], thr[2 * s + 1], t_sat, kbk, kbc, kwk, kwc);
      lo += cnt & 0xff, hi += (cnt >> 8) & 0xff, ties += cnt >> 16;
      if (topk_before(kbk, kbc, bk, bc)) bk = kbk, bc = kbc;  // one more candidate of this lane's
      if (topk_before(kwk, kwc, wk, wc)) wk = kwk, wc = kwc;
    }
    // own: what the rank counts for the target column itself (a minimizer's target is restored
    // before the count, a maximizer's filtered target is left out)
    const bool ofilt = (bits[(size_t)s * nwords + (o >> 5)] >> (o & 31)) & 1u;
    const int own = (mini || !ofilt) ? 1 : 0;
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

// the margins of n rows whose filter bitmaps, targets and kelpie column scores the rows' own
// rank has just read
static void launch_margins(kp_ctx* c, int n, const double* d_q64, const double* d_t64, const double* d_kcol64,
                           const int32_t* d_pred_o, const uint32_t* bits, int nwords, int ldt, int act,
                           const MarginDev& mg) {
  const int nblk = ldt / 256;
  KP_REQUIRE(n <= mg.cap && nblk == mg.nblk, "margins: the workspace does not hold this launch");
  hipLaunchKernelGGL(kp_rank_margin_thr, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, act, d_t64, mg.tol, mg.thr);
  KP_HIP(hipGetLastError());
  const dim3 grid(nblk, (n + RQ - 1) / RQ);
#define KP_MARGIN_LAUNCH(MODE)                                                                                  \
  hipLaunchKernelGGL(kp_rank_f64_margin<MODE>, grid, dim3(256), 0, c->stream, n, c->n_ent, c->dp, d_q64, d_t64, \
                     d_pred_o, c->eT.as<float>(), ldt, nwords, bits, mg.thr, mg.pkey, mg.pcol, mg.pcnt)
  if (act == RANK64_DIST)
    KP_MARGIN_LAUNCH(RANK64_DIST);
  else if (act == RANK64_DIST1)
    KP_MARGIN_LAUNCH(RANK64_DIST1);
  else if (act == RANK64_SIGMOID)
    KP_MARGIN_LAUNCH(RANK64_SIGMOID);
  else
    KP_MARGIN_LAUNCH(RANK64_DOT);
#undef KP_MARGIN_LAUNCH
  KP_HIP(hipGetLastError());
  hipLaunchKernelGGL(kp_rank_margin_merge, dim3(n), dim3(64), 0, c->stream, c->n_ent, nwords, nblk, act, bits, d_pred_o,
                     d_t64, d_kcol64, mg.thr, mg.pkey, mg.pcol, mg.pcnt, mg);
  KP_HIP(hipGetLastError());
}

// bytes of candidate workspace a launch may hold: the slots run in chunks of whole slot rows
constexpr size_t TOPK_WS_BYTES = (size_t)64 << 20;

void launch_rank_f64(kp_ctx* c, int n_slots, const double* d_q64, const double* d_t64, const double* d_kcol64,
                     const int32_t* d_pred_o, const int32_t* d_filt_off, const int32_t* d_filt, float* d_target,
                     int64_t* d_rank, int act, int topk, int32_t* d_top_ids, float* d_top_scores, DevBuf* bits_buf,
                     const MarginDev* mg) {
  if (n_slots <= 0) return;
  const int ldt = (c->n_ent + 255) / 256 * 256;
  if (!c->eT_ready) {
    float* ET = ensure_n<float>(c->eT, (size_t)c->dp * ldt);
    hipLaunchKernelGGL(kp_transpose_table, dim3(ldt / 32, (c->dp + 31) / 32), dim3(256), 0, c->stream, c->dE,
                       c->n_ent, c->dp, ET, ldt);
    KP_HIP(hipGetLastError());
    c->eT_ready = true;
  }
  const int n_cols = c->n_ent + 1;
  const int nwords = (n_cols + 31) / 32;
  DevBuf& bb = bits_buf ? *bits_buf : c->rank.bits;
  uint32_t* bits = ensure_n<uint32_t>(bb, (size_t)n_slots * nwords);
  unsigned long long* rank = reinterpret_cast<unsigned long long*>(d_rank);
  hipLaunchKernelGGL(kp_rank_filter_bits, dim3(n_slots), dim3(256), 0, c->stream, n_slots, nwords, d_filt_off, d_filt,
                     n_cols, bits);
  KP_HIP(hipGetLastError());
  hipLaunchKernelGGL(kp_rank_f64_kelpie, dim3((n_slots + 63) / 64), dim3(64), 0, c->stream, n_slots, c->n_ent, nwords,
                     bits, d_pred_o, d_t64, d_kcol64, act, d_target, rank);
  KP_HIP(hipGetLastError());
  if (mg) launch_margins(c, n_slots, d_q64, d_t64, d_kcol64, d_pred_o, bits, nwords, ldt, act, *mg);
  if (topk > 0) {
    // every wave of the scoring grid leaves a list of k candidates per slot (12 bytes each):
    // the slots run in chunks of whole slot rows that keep the lists within TOPK_WS_BYTES
    const int lists = 4 * (ldt / 256);
    const size_t per_slot = (size_t)lists * topk;  // candidates
    const int rows_fit = (int)std::max<size_t>(1, TOPK_WS_BYTES / (per_slot * 12 * RQ));
    const int chunk = std::min(n_slots, rows_fit * RQ);
    unsigned long long* ck =
        reinterpret_cast<unsigned long long*>(c->rank.cand_key.ensure(sizeof(unsigned long long) * per_slot * chunk));
    int32_t* cc = ensure_n<int32_t>(c->rank.cand_col, per_slot * chunk);
    for (int s0 = 0; s0 < n_slots; s0 += chunk) {
      const int m = std::min(chunk, n_slots - s0);
      const dim3 grid(ldt / 256, (m + RQ - 1) / RQ);
      const double* q = d_q64 + (size_t)s0 * c->dp;
      const uint32_t* b = bits + (size_t)s0 * nwords;
#define KP_TOPK_LAUNCH(MODE)                                                                                       \
  hipLaunchKernelGGL((kp_rank_f64_count<MODE, true>), grid, dim3(256), 0, c->stream, m, c->n_ent, c->dp, q,        \
                     d_t64 + s0, d_pred_o + s0, c->eT.as<float>(), ldt, nwords, b, rank + s0, TopkArgs<true>{topk, ck, cc})
      if (act == RANK64_DIST)
        KP_TOPK_LAUNCH(RANK64_DIST);
      else if (act == RANK64_DIST1)
        KP_TOPK_LAUNCH(RANK64_DIST1);
      else if (act == RANK64_SIGMOID)
        KP_TOPK_LAUNCH(RANK64_SIGMOID);
      else
        KP_TOPK_LAUNCH(RANK64_DOT);
#undef KP_TOPK_LAUNCH
      KP_HIP(hipGetLastError());
      hipLaunchKernelGGL(kp_rank_topk_merge, dim3(m), dim3(256), 0, c->stream, c->n_ent, nwords, lists, topk, act, ck,
                         cc, b, d_pred_o + s0, d_t64 + s0, d_kcol64 + s0, d_top_ids + (size_t)s0 * topk,
                         d_top_scores + (size_t)s0 * topk);
      KP_HIP(hipGetLastError());
    }
    return;
  }
  const dim3 grid(ldt / 256, (n_slots + RQ - 1) / RQ);
  if (act == RANK64_DIST)
    hipLaunchKernelGGL(kp_rank_f64_count<RANK64_DIST>, grid, dim3(256), 0, c->stream, n_slots, c->n_ent, c->dp, d_q64,
                       d_t64, d_pred_o, c->eT.as<float>(), ldt, nwords, bits, rank, TopkArgs<false>{});
  else if (act == RANK64_DIST1)
    hipLaunchKernelGGL(kp_rank_f64_count<RANK64_DIST1>, grid, dim3(256), 0, c->stream, n_slots, c->n_ent, c->dp, d_q64,
                       d_t64, d_pred_o, c->eT.as<float>(), ldt, nwords, bits, rank, TopkArgs<false>{});
  else if (act == RANK64_SIGMOID)
    hipLaunchKernelGGL(kp_rank_f64_count<RANK64_SIGMOID>, grid, dim3(256), 0, c->stream, n_slots, c->n_ent, c->dp,
                       d_q64, d_t64, d_pred_o, c->eT.as<float>(), ldt, nwords, bits, rank, TopkArgs<false>{});
  else
    hipLaunchKernelGGL(kp_rank_f64_count<RANK64_DOT>, grid, dim3(256), 0, c->stream, n_slots, c->n_ent, c->dp, d_q64,
                       d_t64, d_pred_o, c->eT.as<float>(), ldt, nwords, bits, rank, TopkArgs<false>{});
  KP_HIP(hipGetLastError());
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
