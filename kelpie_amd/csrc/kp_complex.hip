// kp_complex.hip -- ComplEx batched post-training (KelpieComplEx +
// KelpieMultiClassNLLOptimizer) and ranking, for gfx950.
//
// Reference semantics (src/link_prediction/models/complex.py:59-112,144-159,
// src/link_prediction/optimization/multiclass_nll_optimizer.py:57-164):
//   rows   = kelpie triples + inverses; per epoch torch.randperm; minibatches of
//            min(batch_size, R) rows stepping by batch_size;
//   loss   = CrossEntropy(q_i . E_all^T, t_i) (mean) + N3;  E_all = [E ; x]
//   step   = Adagrad / Adam / SGD on the single kelpie row x.
//
// Decomposition used here (ComplEx), per minibatch of b rows:
//   * rows whose head is the kelpie ("queries"): q = x o r changes every step.
//     Rows sharing a relation share q and the softmax, so they are merged
//     into one query with count c, kelpie-target count ck and frozen-target
//     sum Tsum.  Each query needs, over the FROZEN entities, the softmax
//     statistics (m, l) and O = sum_e exp(s_e - m) E_e -> kp_cx_attn, a
//     flash-attention-shaped pass with K = V = E on fp32 MFMA.
//   * rows whose head is frozen ("tails"; their target is always the kelpie):
//     q is fixed, so the frozen log-sum-exp is computed once per batch
//     (kp_cx_attn in pair mode) and each step only needs q . x.
//   * the kelpie column (entity |E|) is merged analytically in kp_cx_update,
//     which assembles the single-row gradient and applies the optimizer.
//   When R <= batch_size (one step per epoch) the permutation only reorders
//   the batch, so every epoch reuses one plan; otherwise each (epoch, step)
//   gets its own plan from the permutation.
//
// DistMult (src/link_prediction/models/distmult.py:38-68, same optimizer) is the same step
// with the real product q = x * r on plain [d] rows: the kernels and the host function are
// written over a product policy (CxProd / DmProd below), and only the policy differs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <type_traits>

#include "kp_attn.hpp"
#include "kp_attn3.hpp"
#include "kp_attn64.hpp"
#include "kp_cx_plan.hpp"
#include "kp_cx_rowmap.hpp"
#include "kp_posttrain.hpp"

namespace {
using namespace kpattn;

// the ComplEx product from exact fp64 products of the fp32 operands (kp_cx_rankq64)
__device__ __forceinline__ double cx_q64(const float* __restrict__ lhs, const float* __restrict__ rel, int d,
                                         int half) {
  if (d < half) return (double)lhs[d] * (double)rel[d] - (double)lhs[d + half] * (double)rel[d + half];
  if (d < 2 * half) {
    const int i = d - half;
    return (double)lhs[i] * (double)rel[d] + (double)lhs[d] * (double)rel[i];
  }
  return 0.0;
}

// kp_posttrain_rank_f64: the same product on an fp64 left operand (the kelpie row), each
// product and the sum rounded once, as torch's float64 ops round them (complex.py:65-72)
__device__ __forceinline__ double cx_q64(const double* __restrict__ lhs, const float* __restrict__ rel, int d,
                                         int half) {
  if (d < half) return lhs[d] * (double)rel[d] - lhs[d + half] * (double)rel[d + half];
  if (d < 2 * half) {
    const int i = d - half;
    return lhs[i] * (double)rel[d] + lhs[d] * (double)rel[i];
  }
  return 0.0;
}

// ----------------------------------------------------------------------------
// Product policies.  The kernels below are written once over the model's product
// q = lhs o rel; a policy holds its fp32 and fp64 forms, the Jacobian J_rel^T applied in
// the contribution, and the regulariser modulus.  `w` is the policy's extent of a row:
// the complex width d / 2 for ComplEx (rows [Re | Im]), the row width d for DistMult.
// A row is G runs of w coordinates; coordinate i of run h is element i + h * w, and the
// G elements of one i form one regulariser factor.
// ----------------------------------------------------------------------------
struct CxProd {  // ComplEx (complex.py:59-112)
  static constexpr int G = 2;
  static int extent(int dim) { return dim / 2; }
  static __device__ __forceinline__ float q(const float* __restrict__ lhs, const float* __restrict__ rel, int d,
                                            int w) {
    return cx_q(lhs, rel, d, w);
  }
  static __device__ __forceinline__ double q64(const float* __restrict__ lhs, const float* __restrict__ rel, int d,
                                               int w) {
    return cx_q64(lhs, rel, d, w);
  }
  static __device__ __forceinline__ double q64(const double* __restrict__ lhs, const float* __restrict__ rel, int d,
                                               int w) {
    return cx_q64(lhs, rel, d, w);
  }
  static __device__ __forceinline__ double mod64(const double* xv) { return sqrt(xv[0] * xv[0] + xv[1] * xv[1]); }
  static __device__ __forceinline__ void emit(double* __restrict__ out, int i, int w, const double* xv,
                                              const double* rv, const double* dv, double cf) {
    const double a = xv[0], b = xv[1], cc = rv[0], ee = rv[1];
    const double dre = dv[0], dim_ = dv[1];
    const double qre = a * cc - b * ee, qim = a * ee + b * cc;
    out[i] = dre * cc + dim_ * ee + cf * qre;
    out[i + w] = -dre * ee + dim_ * cc + cf * qim;
  }
  // kp_posttrain_rank_attrib: J_r v = v o r and J_r^T v at one coordinate, (re, im) pairs
  static __device__ __forceinline__ void fwd(const double* v, const double* rv, double* out) {
    out[0] = v[0] * rv[0] - v[1] * rv[1];
    out[1] = v[0] * rv[1] + v[1] * rv[0];
  }
  static __device__ __forceinline__ void bwd(const double* v, const double* rv, double* out) {
    out[0] = v[0] * rv[0] + v[1] * rv[1];
    out[1] = -v[0] * rv[1] + v[1] * rv[0];
  }
  // the factor of one (re, im) pair: the complex modulus (complex.py:80-84)
  static __device__ __forceinline__ float mod(const float* xv) { return sqrtf(xv[0] * xv[0] + xv[1] * xv[1]); }
  static __device__ __forceinline__ double mod64(const float* xv) {
    return sqrt((double)xv[0] * xv[0] + (double)xv[1] * xv[1]);
  }
  // out = J_r^T dv + cf q at coordinate i:  J_r^T (u, v) = (u c + v e, -u e + v c)
  static __device__ __forceinline__ void emit(float* __restrict__ out, int i, int w, const double* xv,
                                              const double* rv, const double* dv, double cf) {
    const double a = xv[0], b = xv[1], cc = rv[0], ee = rv[1];
    const double dre = dv[0], dim_ = dv[1];
    const double qre = a * cc - b * ee, qim = a * ee + b * cc;
    out[i] = (float)(dre * cc + dim_ * ee + cf * qre);
    out[i + w] = (float)(-dre * ee + dim_ * cc + cf * qim);
  }
};

struct DmProd {  // DistMult (distmult.py:38-68): plain [d] rows, q = lhs * rel
  static constexpr int G = 1;
  static int extent(int dim) { return dim; }
  static __device__ __forceinline__ float q(const float* __restrict__ lhs, const float* __restrict__ rel, int d,
                                            int w) {
    return d < w ? __fmul_rn(lhs[d], rel[d]) : 0.f;
  }
  static __device__ __forceinline__ double q64(const float* __restrict__ lhs, const float* __restrict__ rel, int d,
                                               int w) {
    return d < w ? (double)lhs[d] * (double)rel[d] : 0.0;
  }
  static __device__ __forceinline__ double q64(const double* __restrict__ lhs, const float* __restrict__ rel, int d,
                                               int w) {
    return d < w ? lhs[d] * (double)rel[d] : 0.0;
  }
  static __device__ __forceinline__ double mod64(const double* xv) { return fabs(xv[0]); }
  static __device__ __forceinline__ void emit(double* __restrict__ out, int i, int w, const double* xv,
                                              const double* rv, const double* dv, double cf) {
    const double q = xv[0] * rv[0];
    out[i] = dv[0] * rv[0] + cf * q;
  }
  // kp_posttrain_rank_attrib: J_r v = J_r^T v = r * v
  static __device__ __forceinline__ void fwd(const double* v, const double* rv, double* out) { out[0] = v[0] * rv[0]; }
  static __device__ __forceinline__ void bwd(const double* v, const double* rv, double* out) { out[0] = v[0] * rv[0]; }
  // the factor of one coordinate: |x_i| (distmult.py:66, sqrt(x_i^2))
  static __device__ __forceinline__ float mod(const float* xv) { return fabsf(xv[0]); }
  static __device__ __forceinline__ double mod64(const float* xv) { return fabs((double)xv[0]); }
  // J_r^T v = r * v
  static __device__ __forceinline__ void emit(float* __restrict__ out, int i, int w, const double* xv,
                                              const double* rv, const double* dv, double cf) {
    const double q = xv[0] * rv[0];
    out[i] = (float)(dv[0] * rv[0] + cf * q);
  }
};

// the product in the precision of the row it is stored to: fp32 (Prod::q), or fp64 for
// kp_posttrain_rank_f64's double rows (Prod::q64)
template <class Prod, class QT, class LT>
__device__ __forceinline__ QT cx_q_as(const LT* __restrict__ lhs, const float* __restrict__ rel, int d, int w) {
  if constexpr (sizeof(QT) == sizeof(double))
    return Prod::q64(lhs, rel, d, w);
  else
    return Prod::q(lhs, rel, d, w);
}

// qpair[p] = E[h] o R[r] for the frozen-head rows (QT: the stored row's type)
template <class Prod, class QT = float>
__global__ void kp_cx_qpair(const float* __restrict__ E, const float* __restrict__ R, int dp, int half,
                            const int2* __restrict__ pairs, int n_pairs, QT* __restrict__ out) {
  int p = blockIdx.x;
  if (p >= n_pairs) return;
  int2 hr = pairs[p];
  const float* lhs = E + (size_t)hr.x * dp;
  const float* rel = R + (size_t)hr.y * dp;
  for (int d = threadIdx.x; d < dp; d += blockDim.x) out[(size_t)p * dp + d] = cx_q_as<Prod, QT>(lhs, rel, d, half);
}

// the log-sum-exp over the frozen entities from the attention's per-split (kp_attn / kp_attn3,
// ST = float) or per-range (kp_attn64, ST = double) statistics (m, l), in split order: the max
// in ST, the sum of the rescaled l's in fp64.  An empty part (m = -inf) adds nothing.
template <class ST>
__device__ __forceinline__ double lse_ranges64(const ST* __restrict__ am, const ST* __restrict__ al, int n,
                                               int ranges, int item) {
  ST mm = kNegInf;
  for (int s = 0; s < ranges; ++s) mm = fmax(mm, am[(size_t)s * n + item]);
  double ll = 0.0;
  for (int s = 0; s < ranges; ++s) {
    const ST ms = am[(size_t)s * n + item];
    if (ms != kNegInf) ll += (double)al[(size_t)s * n + item] * exp((double)ms - (double)mm);
  }
  return (double)mm + log(ll);
}

// lsef[p] = the frozen-head pair's log-sum-exp over the frozen entities, merged from the
// attention's partial statistics (one thread per pair), rounded once to ST at the store
template <class ST>
__global__ void kp_cx_lse_merge(int npairs, int n_split, const ST* __restrict__ am, const ST* __restrict__ al,
                                ST* __restrict__ lsef) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  lsef[p] = (ST)lse_ranges64(am, al, npairs, n_split, p);
}

// Tsum[q] = sum of frozen target rows of a plan query, in list order (AT: the accumulator's
// and the sums' type)
template <class AT>
__global__ void kp_cx_tsum(const float* __restrict__ E, int dp, const CxQuery* __restrict__ pq, int nq,
                           const int32_t* __restrict__ targets, AT* __restrict__ tsum) {
  int q = blockIdx.x;
  if (q >= nq) return;
  CxQuery Q = pq[q];
  for (int d = threadIdx.x; d < dp; d += blockDim.x) {
    AT acc = 0;
    for (int i = 0; i < Q.tg_count; ++i) acc += (AT)E[(size_t)targets[Q.tg_begin + i] * dp + d];
    tsum[(size_t)q * dp + d] = acc;
  }
}

// ----------------------------------------------------------------------------
// kp_cx_update: one workgroup per active slot at this step.  Assembles the
// single-row gradient of the minibatch loss and applies the
// optimizer with torch's op order (optim/adagrad.py, optim/adam.py).
// ----------------------------------------------------------------------------
// (T: the state's type; CxOpt64 is kp_posttrain_rank_f64's)
template <class T>
struct CxOptT {
  int kind;
  T lr, b1, b2, eps;
  T one_minus_b1, one_minus_b2;
  T step_size;  // Adam: lr / (1 - b1^t)
  T bc2_sqrt;   // Adam: sqrt(1 - b2^t)
  T reg_w;
  int reg_n2;  // KP_REG_N2: N2 on the whole row's L2 norm (regularizers.py:25-35) instead of N3
};
using CxOpt = CxOptT<float>;
using CxOpt64 = CxOptT<double>;

#define UPD_MAXSPLIT 16

// kp_posttrain_rank_trace: the TRACE form of kp_cx_contrib also writes the item's fp64 share
// of the step's summed negative log-likelihood (include/kelpie_hip.h, "Post-training
// trace"); without the flag the argument is an empty struct and the kernel the one it was
template <bool TRACE>
struct CxTraceArgs {};
template <>
struct CxTraceArgs<true> {
  double* term;  // [nq + nt]
};

// One wave per (query or frozen-head row) of this step: its contribution to the
// kelpie row's gradient (un-normalised by the batch size).
//   query (kelpie-head rows sharing relation r, count c, kelpie targets ck):
//     J_r^T (c <E> - Tsum - ck x) + (c p_k - ck) q,   <E> = softmax-weighted entity
//     (frozen part sum_sp w_sp O_sp merged with the kelpie column p_k x)
//   frozen-head row pair (count c, target = kelpie):  c (p_k - 1) q_pair
// (`half` is the policy's extent w: d / 2 for ComplEx, d for DistMult)
// TRACE: item's loss term, from the fp64 values above:
//   query:  c lse - q . Tsum - ck z  (the c rows' lse minus their targets' scores)
//   frozen-head pair:  c (lse - z)
template <int DP, class Prod, bool TRACE = false>
__global__ __launch_bounds__(256) void kp_cx_contrib(int half, const int4* __restrict__ stepq, int nq,
                                                     const int4* __restrict__ stept, int nt,
                                                     const CxQuery* __restrict__ pq, const float* __restrict__ X,
                                                     const float* __restrict__ R, const float* __restrict__ Tsum,
                                                     const float* __restrict__ Qpair, const float* __restrict__ lsef,
                                                     const float* __restrict__ att_m, const float* __restrict__ att_l,
                                                     const float* __restrict__ att_O, int n_split,
                                                     float* __restrict__ contrib, CxTraceArgs<TRACE> tr) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= nq + nt) return;
  float* out = contrib + (size_t)item * DP;
  if (item < nq) {
    const int4 sq = stepq[item];  // slot, rel, plan-query index
    const float* x = X + (size_t)sq.x * DP;
    const float* rel = R + (size_t)sq.y * DP;
    const CxQuery Q = pq[sq.z];
    float z = 0.f;
    for (int d = lane; d < Prod::G * half; d += 64) z += Prod::q(x, rel, d, half) * x[d];
    z = wave_sum(z);
    // The softmax normalisation in fp64 with correctly rounded exp / log.  <E> below is
    // ~5e-4 per coordinate at the reference init and the row contributions cancel to a
    // gradient up to ~100x smaller on the coordinates Adagrad has not saturated, so a
    // one-sided ulp error of a fast exp / log here (every row, every step, the same
    // sign) became a one-sided drift of those coordinates of the kelpie row (measured
    // ~-4e-6 against the fp64 reference, tools/headline_probe.py).
    // The split statistics one split per lane (n_split <= 64): the max, the fp64 sum of
    // the rescaled l's (a butterfly, deterministic) and each split's weight, so a wave
    // makes two fp64 exp per lane instead of 2 n_split in sequence on every lane.
    const bool has = lane < n_split;
    const float ms_l = has ? att_m[(size_t)lane * nq + item] : kNegInf;
    const float ls_l = has ? att_l[(size_t)lane * nq + item] : 0.f;
    const float mm = wave_max(ms_l);
    double e_l = (ms_l == kNegInf) ? 0.0 : (double)ls_l * exp((double)ms_l - (double)mm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e_l += __shfl_xor(e_l, o, 64);
    const double lse_f = (double)mm + log(e_l);
    const double hi = fmax(lse_f, (double)z), lo = fmin(lse_f, (double)z);
    const double lse = hi + log1p(exp(lo - hi));
    const double pk = exp((double)z - lse);
    const double wv_l = (ms_l == kNegInf) ? 0.0 : exp((double)ms_l - lse);
    // merge the partials split by split (increasing split order), one split at a time:
    // 64 registers, so that a wave fits beside a resident kp_attn3 wave on its SIMD (that
    // one leaves 104 of the 512 registers per lane free; with two splits' loads in flight
    // this kernel took 94 and still fitted, the round-4 forms with 150 did not and ran
    // only on the CUs no attention workgroup held: 92 -> 192 us per launch under overlap)
    constexpr int G = Prod::G;
    constexpr int NI = (DP / G + 63) / 64;
    double o_k[NI][G];
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
      for (int h = 0; h < G; ++h) o_k[k][h] = 0.0;
    for (int sp = 0; sp < n_split; ++sp) {
      const double w0 = __shfl(wv_l, sp, 64);
      const float* O0 = att_O + ((size_t)sp * nq + item) * DP;
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        const int i = lane + 64 * k;
        const bool in = i < half;
        float o0[G];
#pragma unroll
        for (int h = 0; h < G; ++h) o0[h] = in ? O0[i + h * half] : 0.f;
#pragma unroll
        for (int h = 0; h < G; ++h) o_k[k][h] += w0 * (double)o0[h];
      }
    }
    const double fc = (double)Q.c, fck = (double)Q.ck;
    const double cf = fc * pk - fck;
    const float* ts = Tsum + (size_t)sq.z * DP;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int i = lane + 64 * k;
      if (i >= half) continue;
      double xv[G], rv[G], dv[G];
#pragma unroll
      for (int h = 0; h < G; ++h) xv[h] = x[i + h * half];
#pragma unroll
      for (int h = 0; h < G; ++h) rv[h] = rel[i + h * half];
#pragma unroll
      for (int h = 0; h < G; ++h) {
        const double e = o_k[k][h] + pk * xv[h];  // <E>: the frozen part and the kelpie column
        dv[h] = fc * e - (double)ts[i + h * half] - fck * xv[h];
      }
      Prod::emit(out, i, half, xv, rv, dv, cf);
    }
    if constexpr (TRACE) {
      // q . Tsum on the step's fp32 query (the q of z and of the attention), summed in fp64:
      // lane-strided, then a butterfly
      double qt = 0.0;
      for (int d = lane; d < Prod::G * half; d += 64) qt += (double)Prod::q(x, rel, d, half) * (double)ts[d];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) qt += __shfl_xor(qt, o, 64);
      if (lane == 0) tr.term[item] = fc * lse - qt - fck * (double)z;
    }
  } else {
    const int4 st = stept[item - nq];  // slot, pair, count
    const float* x = X + (size_t)st.x * DP;
    const float* qp = Qpair + (size_t)st.y * DP;
    float z = 0.f;
    for (int d = lane; d < Prod::G * half; d += 64) z += qp[d] * x[d];
    z = wave_sum(z);
    const double lf = lsef[st.y];
    const double hi = fmax(lf, (double)z), lo = fmin(lf, (double)z);
    const double lse = hi + log1p(exp(lo - hi));
    const double coef = (double)st.z * (exp((double)z - lse) - 1.0);
    for (int d = lane; d < Prod::G * half; d += 64) out[d] = (float)(coef * (double)qp[d]);
    if constexpr (TRACE) {
      if (lane == 0) tr.term[item] = (double)st.z * (lse - (double)z);
    }
  }
}

// kp_posttrain_rank_trace: freg[r] = the regulariser's factor of row r of a frozen table
// (E or R), once per batch: N3 sum_i |f_i|^3, N2 (sum_i |f_i|^2)^(3/2), |f_i| the policy's
// modulus.  One wave per row, fp64, lane-strided then a butterfly (a fixed order).
template <class Prod>
__global__ __launch_bounds__(256) void kp_cx_rowreg(const float* __restrict__ T, int n, int dp, int half, int reg_n2,
                                                    double* __restrict__ freg) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float* row = T + (size_t)r * dp;
  double acc = 0.0;
  for (int i = lane; i < half; i += 64) {
    float xv[Prod::G];
#pragma unroll
    for (int h = 0; h < Prod::G; ++h) xv[h] = row[i + h * half];
    const double f = Prod::mod64(xv);
    acc += reg_n2 ? f * f : f * f * f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) freg[r] = reg_n2 ? acc * sqrt(acc) : acc;
}

// kp_posttrain_rank_trace: one wave per active slot of the step, after kp_cx_contrib<TRACE>
// and before kp_cx_update moves x.  Sums the slot's item terms (its queries, then its
// frozen-head pairs; lane-strided in item order, then a butterfly: a fixed order), divides
// by the batch size and adds the regulariser's value: the frozen rows' factors from freg_e /
// freg_r, the kelpie row's (cnt_l + cnt_r occurrences) from x as it is before the update.
// One fp32 rounding, at the store of step `step` of the slot.
template <int DP, class Prod>
__global__ __launch_bounds__(64) void kp_cx_trace_sum(int half, const int4* __restrict__ act,
                                                      const CxPlan* __restrict__ plans,
                                                      const CxQuery* __restrict__ pq,
                                                      const int32_t* __restrict__ targets,
                                                      const int2* __restrict__ pairs, const int4* __restrict__ stept,
                                                      int nq, const float* __restrict__ X,
                                                      const double* __restrict__ term,
                                                      const double* __restrict__ freg_e,
                                                      const double* __restrict__ freg_r, float reg_w, int reg_n2,
                                                      const int32_t* __restrict__ trace_off, int step,
                                                      float* __restrict__ loss) {
  const int lane = threadIdx.x;
  const int4 a4 = act[blockIdx.x];  // slot, plan, qoff, toff
  const CxPlan P = plans[a4.y];
  const bool reg = reg_w != 0.f;
  double nll = 0.0, fz = 0.0;
  for (int j = lane; j < P.q_count; j += 64) {
    nll += term[a4.z + j];
    if (reg) {
      const CxQuery Q = pq[P.q_begin + j];
      fz += (double)Q.c * freg_r[Q.rel];
      for (int i = 0; i < Q.tg_count; ++i) fz += freg_e[targets[Q.tg_begin + i]];
    }
  }
  for (int j = lane; j < P.t_count; j += 64) {
    nll += term[nq + a4.w + j];
    if (reg) {
      const int4 st = stept[a4.w + j];  // slot, pair, count
      const int2 hr = pairs[st.y];
      fz += (double)st.z * (freg_e[hr.x] + freg_r[hr.y]);
    }
  }
  double fx = 0.0;
  if (reg) {
    const float* x = X + (size_t)a4.x * DP;
    for (int i = lane; i < half; i += 64) {
      float xv[Prod::G];
#pragma unroll
      for (int h = 0; h < Prod::G; ++h) xv[h] = x[i + h * half];
      const double f = Prod::mod64(xv);
      fx += reg_n2 ? f * f : f * f * f;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nll += __shfl_xor(nll, o, 64);
    fz += __shfl_xor(fz, o, 64);
    fx += __shfl_xor(fx, o, 64);
  }
  if (lane == 0) {
    double l = nll / (double)P.b;
    if (reg) {
      if (reg_n2) fx = fx * sqrt(fx);
      l += (double)reg_w * (fz + (double)(P.cnt_l + P.cnt_r) * fx) / (double)P.b;
    }
    loss[trace_off[a4.x] + step] = (float)l;
  }
}

#ifndef KP_CX_UPD64
#define KP_CX_UPD64 0
#endif
// kp_posttrain_rank_marks: per entry of the step's active list the mark row its update also
// stores (-1: none), and the mark rows [slots][marks][DP].  Without the flag the struct is
// empty and kp_cx_update is what it was.
template <bool MARKS>
struct CxMarkArgs {};
template <>
struct CxMarkArgs<true> {
  const int32_t* row;  // [active slots of the step]
  float* rows;
};

// kp_posttrain_rank_attrib: per slot [slots][DP] the step's D_t (the diagonal the update applies
// to the gradient: lr, or Adagrad's lr / (sqrt(s) + eps) in the update's fp32) and the row x_t
// before it moves, and per slot the N2 norm the update used.  Without the flag the struct is
// empty and kp_cx_update is what it was.
template <bool ATTRIB>
struct CxAttribArgs {};
template <>
struct CxAttribArgs<true> {
  float *D, *xprev, *n2;
};

// Sum a slot's contributions, add the N3 term, apply the optimizer (torch op order).
// (`half` is the policy's extent w, as in kp_cx_contrib)
// MARKS: the thread that stores an updated element stores it to the slot's mark row as well
// when the plan marks this (slot, step); a plain vector store, no launch of its own
// ATTRIB: the thread also stores the element's D_t and its value before the update (plain
// vector stores; kp_cx_attrib reads them after this kernel)
template <int DP, class Prod, bool MARKS = false, bool ATTRIB = false>
__global__ __launch_bounds__(256) void kp_cx_update(int half, const int4* __restrict__ act,
                                                    const CxPlan* __restrict__ plans, int nq,
                                                    const float* __restrict__ contrib, float* __restrict__ X,
                                                    float* __restrict__ S1, float* __restrict__ S2, CxOpt opt,
                                                    CxMarkArgs<MARKS> mk, CxAttribArgs<ATTRIB> at) {
  constexpr int G = Prod::G;
  const int tid = threadIdx.x;
  const int4 a4 = act[blockIdx.x];  // slot, plan, qoff, toff
  const int slot = a4.x;
  const CxPlan P = plans[a4.y];
  float* x = X + (size_t)slot * DP;
  const float inv_b = 1.0f / (float)P.b;
  // contribution rows: the slot's queries, then its frozen-head rows
  const int nc = P.q_count + P.t_count;
  auto crow = [&](int j) -> const float* {
    return j < P.q_count ? contrib + (size_t)(a4.z + j) * DP : contrib + (size_t)(nq + a4.w + j - P.q_count) * DP;
  };
  // The rows sum in four wave-strided partials with four chains each, so 16 rows'
  // loads are in flight at once (one sequential chain per dimension was bound by the
  // load latency: ~90 us per step at FB15k-237 sizes); a slot with at most UPD_WIDE
  // rows keeps the sequential chain (the choice is block-uniform).
  constexpr int UPD_WIDE = 4;
#if KP_CX_UPD64
  // the slot's gradient assembled in fp64 (row sums, 1/B, regulariser term) and rounded
  // once to fp32 before the optimizer; the four wave partials meet in two rounds through
  // 2 x DP doubles, the LDS of the fp32 form (6.4 KiB at D = 400: it still fits beside a
  // resident kp_attn3<25> workgroup)
  typedef double acc_t;
  __shared__ double red[2][DP];
  if (nc > UPD_WIDE) {
    const int w = tid >> 6, lane = tid & 63;
    double part[(DP + 63) / 64];
#pragma unroll
    for (int k = 0; k < (DP + 63) / 64; ++k) {
      const int d = lane + 64 * k;
      part[k] = 0.0;
      if (d >= G * half) continue;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      int j = w;
      for (; j + 12 < nc; j += 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += crow(j + 4 * q)[d];
      }
      if (j < nc) acc[0] += crow(j)[d];  // at most three rows are left
      if (j + 4 < nc) acc[1] += crow(j + 4)[d];
      if (j + 8 < nc) acc[2] += crow(j + 8)[d];
      part[k] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
      if (w >= 2) red[w - 2][d] = part[k];
    }
    __syncthreads();
    if (w < 2)
#pragma unroll
      for (int k = 0; k < (DP + 63) / 64; ++k) {
        const int d = lane + 64 * k;
        if (d < G * half) red[w][d] = part[k] + red[w][d];
      }
    __syncthreads();
  }
#else
  typedef float acc_t;
  __shared__ float red[4][DP];
  if (nc > UPD_WIDE) {
    const int w = tid >> 6, lane = tid & 63;
    for (int d = lane; d < G * half; d += 64) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      int j = w;
      for (; j + 12 < nc; j += 16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += crow(j + 4 * k)[d];
      }
      if (j < nc) acc[0] += crow(j)[d];  // at most three rows are left
      if (j + 4 < nc) acc[1] += crow(j + 4)[d];
      if (j + 8 < nc) acc[2] += crow(j + 8)[d];
      red[w][d] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
    __syncthreads();
  }
#endif
  // N2 (regularizers.py:25-35): the factor of each batch row holding the kelpie entity
  // is ||f||^3 with f_i the policy's modulus (complex.py:80-84: |x_i| complex; distmult.py:66:
  // |x_i| real), so its gradient is 3 w / B * ||f|| * x per such row; ||f|| over the whole
  // row, before the update
  float n2 = 0.f;
  if (opt.reg_w != 0.f && opt.reg_n2) {
    __shared__ float n2red[4];
    float ps = 0.f;
    for (int i = tid; i < half; i += 256) {
      float xv[G];
#pragma unroll
      for (int h = 0; h < G; ++h) xv[h] = x[i + h * half];
      const float f = Prod::mod(xv);
      ps += f * f;
    }
    ps = wave_sum(ps);
    if ((tid & 63) == 0) n2red[tid >> 6] = ps;
    __syncthreads();
    n2 = sqrtf((n2red[0] + n2red[1]) + (n2red[2] + n2red[3]));
  }
  if constexpr (ATTRIB) {
    if (tid == 0) at.n2[slot] = n2;
  }
#pragma unroll
  for (int u = 0; u < (DP / G + 255) / 256; ++u) {
    const int i = tid + 256 * u;
    if (i >= half) continue;
    acc_t gv[G];
#pragma unroll
    for (int h = 0; h < G; ++h) gv[h] = 0.f;
    if (nc > UPD_WIDE) {
#pragma unroll
      for (int h = 0; h < G; ++h) {
        const int d = i + h * half;
#if KP_CX_UPD64
        gv[h] = red[0][d] + red[1][d];
#else
        gv[h] = (red[0][d] + red[1][d]) + (red[2][d] + red[3][d]);
#endif
      }
    } else {
      for (int j = 0; j < nc; ++j) {
        const float* c = crow(j);
#pragma unroll
        for (int h = 0; h < G; ++h) gv[h] += c[i + h * half];
      }
    }
#pragma unroll
    for (int h = 0; h < G; ++h) {
#if KP_CX_UPD64
      gv[h] /= (double)P.b;
#else
      gv[h] *= inv_b;
#endif
    }
    float xv[G];
#pragma unroll
    for (int h = 0; h < G; ++h) xv[h] = x[i + h * half];
    if (opt.reg_w != 0.f) {
#if KP_CX_UPD64
      const double mod = opt.reg_n2 ? (double)n2 : Prod::mod64(xv);
      const double k3 = 3.0 * (double)opt.reg_w / (double)P.b * (double)(P.cnt_l + P.cnt_r) * mod;
#else
      const float mod = opt.reg_n2 ? n2 : Prod::mod(xv);
      const float k3 = 3.0f * opt.reg_w * inv_b * (float)(P.cnt_l + P.cnt_r) * mod;
#endif
#pragma unroll
      for (int h = 0; h < G; ++h) gv[h] += k3 * xv[h];
    }
#pragma unroll
    for (int h = 0; h < G; ++h) {
      const int d = i + h * half;
      const float gd = (float)gv[h];
      float xd = xv[h];
      const size_t o = (size_t)slot * DP + d;
      if (opt.kind == KP_OPT_ADAGRAD) {
        float s1 = S1[o];
        s1 = s1 + gd * gd;
        const float stdv = sqrtf(s1) + opt.eps;
        xd = xd + (-opt.lr * gd) / stdv;
        S1[o] = s1;
        if constexpr (ATTRIB) at.D[o] = opt.lr / stdv;
      } else if (opt.kind == KP_OPT_ADAM) {
        float m1 = S1[o], v2 = S2[o];
        m1 = m1 + opt.one_minus_b1 * (gd - m1);
        v2 = v2 * opt.b2;
        v2 = v2 + (opt.one_minus_b2 * gd) * gd;
        const float den = sqrtf(v2) / opt.bc2_sqrt + opt.eps;
        xd = xd + (-opt.step_size * m1) / den;
        S1[o] = m1;
        S2[o] = v2;
      } else {
        xd = xd + (-opt.lr) * gd;
        if constexpr (ATTRIB) at.D[o] = opt.lr;
      }
      x[d] = xd;
      if constexpr (ATTRIB) at.xprev[o] = xv[h];
      if constexpr (MARKS) {
        const int mrow = mk.row[blockIdx.x];  // block-uniform
        if (mrow >= 0) mk.rows[(size_t)mrow * DP + d] = xd;
      }
    }
  }
}

// ----------------------------------------------------------------------------
// kp_posttrain_rank_attrib (include/kelpie_hip.h, "Attributions").  The kernels below run only
// in a call that asks for attributions.
// ----------------------------------------------------------------------------
__device__ __forceinline__ double at_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the device side of the request: the row map (kp_cx_rowmap.hpp), the slots' score gradients,
// what kp_cx_update<ATTRIB> leaves per slot, and the results
struct CxAttribDev {
  const int32_t *tg_row = nullptr, *qk_off = nullptr, *qk_row = nullptr, *t_off = nullptr, *t_row = nullptr;
  double* c = nullptr;  // [ns][DP]
  float *D = nullptr, *xprev = nullptr, *x0 = nullptr, *n2 = nullptr;
  double *fit = nullptr, *reg = nullptr, *delta = nullptr;
  int rows = 0;
};

// c_s = grad_x score(kelpie, p, o) = J_{R_p}^T E_o, once per slot before the loop: exact fp64
// products of the fp32 operands, each sum rounded once; the padding is 0.  rank rows (s, p, o).
template <int DP, class Prod>
__global__ __launch_bounds__(64) void kp_cx_attrib_c(int half, const float* __restrict__ E,
                                                     const float* __restrict__ R, const int32_t* __restrict__ pred,
                                                     int ns, double* __restrict__ C) {
  constexpr int G = Prod::G;
  const int s = blockIdx.x;
  if (s >= ns) return;
  const float* rel = R + (size_t)pred[3 * s + 1] * DP;
  const float* eo = E + (size_t)pred[3 * s + 2] * DP;
  double* c = C + (size_t)s * DP;
  for (int d = threadIdx.x; d < DP; d += 64) c[d] = 0.0;
  __syncthreads();
  for (int i = threadIdx.x; i < half; i += 64) {
    double ev[G], rv[G], out[G];
#pragma unroll
    for (int h = 0; h < G; ++h) ev[h] = eo[i + h * half], rv[h] = rel[i + h * half];
    Prod::bwd(ev, rv, out);
#pragma unroll
    for (int h = 0; h < G; ++h) c[i + h * half] = out[h];
  }
}

// One workgroup per active slot of the step, after kp_cx_update<ATTRIB> and while the step's
// contribution rows are still in the workspace; its four waves take the slot's items (queries,
// then frozen-head pairs) in turn.  With v = c o D_t, u = J_r v and the item's fp32 contribution
// row g (kp_cx_contrib), all dots in fp64 (lane-strided, then a butterfly: a fixed order):
//   query (c rows, ck of them with the kelpie as tail):  every row shares
//       S = (<v, g> + sum_t <u, E_t> + ck kk) / c,   kk = <u, x> + <v, x o r>,
//     a row with the frozen tail t gets S - <u, E_t>, one with the kelpie as tail S - kk, so the
//     rows of a query sum to <v, g> whatever the rounding of the targets' sum was;
//   frozen-head pair (c rows):  every row gets <v, g> / c.
// fit[row] -= value / b; reg[row] -= occ <v, 3 w mod x> / b with the update's own moduli.  A row
// belongs to one item of the step, the item to one wave, and a row's two additions are the same
// lane's: one writer per row, no atomics.
// Nothing of a row is held in registers across a loop: v, x_t and u are re-formed from memory
// (they stay in cache) wherever a dot needs them, so a wave takes few registers and fits beside a
// resident kp_attn3 wave (104 per lane are free, see kp_cx_contrib).
template <int DP, class Prod>
__global__ __launch_bounds__(256) void kp_cx_attrib(int half, const int4* __restrict__ act,
                                                    const CxPlan* __restrict__ plans, const CxQuery* __restrict__ pq,
                                                    const int32_t* __restrict__ targets, const int4* __restrict__ stept,
                                                    int nq, const float* __restrict__ contrib,
                                                    const float* __restrict__ E, const float* __restrict__ R,
                                                    float reg_w, int reg_n2, CxAttribDev at) {
  constexpr int G = Prod::G;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int4 a4 = act[blockIdx.x];  // slot, plan, qoff, toff
  const CxPlan P = plans[a4.y];
  const double* cs = at.c + (size_t)a4.x * DP;
  const float* Ds = at.D + (size_t)a4.x * DP;
  const float* xs = at.xprev + (size_t)a4.x * DP;
  const double fb = (double)P.b;
  const auto load_v = [&](int i, double* vv) {
#pragma unroll
    for (int h = 0; h < G; ++h) vv[h] = cs[i + h * half] * (double)Ds[i + h * half];
  };
  double regu = 0.0;  // <v, 3 w mod x>
  if (reg_w != 0.f) {
    const float n2 = reg_n2 ? at.n2[a4.x] : 0.f;
    for (int i = lane; i < half; i += 64) {
      double vv[G];
      float xf[G];
      load_v(i, vv);
#pragma unroll
      for (int h = 0; h < G; ++h) xf[h] = xs[i + h * half];
      const double mod = reg_n2 ? (double)n2 : (double)Prod::mod(xf);
#pragma unroll
      for (int h = 0; h < G; ++h) regu += vv[h] * (3.0 * (double)reg_w * mod * (double)xf[h]);
    }
    regu = at_wave_sum(regu);
  }
  for (int j = w; j < P.q_count; j += 4) {
    const int qi = P.q_begin + j;
    const CxQuery Q = pq[qi];
    const float* rel = R + (size_t)Q.rel * DP;
    const float* g = contrib + (size_t)(a4.z + j) * DP;
    double a = 0.0, kk = 0.0;
    for (int i = lane; i < half; i += 64) {
      double vv[G], rv[G], xv[G], uv[G], qv[G];
      load_v(i, vv);
#pragma unroll
      for (int h = 0; h < G; ++h) rv[h] = (double)rel[i + h * half], xv[h] = (double)xs[i + h * half];
      Prod::fwd(vv, rv, uv);
      Prod::fwd(xv, rv, qv);
#pragma unroll
      for (int h = 0; h < G; ++h) {
        a += vv[h] * (double)g[i + h * half];
        kk += uv[h] * xv[h] + vv[h] * qv[h];
      }
    }
    a = at_wave_sum(a);
    kk = at_wave_sum(kk);
    double tsum = 0.0;
    for (int t = 0; t < Q.tg_count; ++t) {
      const float* et = E + (size_t)targets[Q.tg_begin + t] * DP;
      double dt = 0.0;
      for (int i = lane; i < half; i += 64) {
        double vv[G], rv[G], uv[G];
        load_v(i, vv);
#pragma unroll
        for (int h = 0; h < G; ++h) rv[h] = (double)rel[i + h * half];
        Prod::fwd(vv, rv, uv);
#pragma unroll
        for (int h = 0; h < G; ++h) dt += uv[h] * (double)et[i + h * half];
      }
      dt = at_wave_sum(dt);
      tsum += dt;
      if (lane == (t & 63)) at.fit[at.tg_row[Q.tg_begin + t]] += dt / fb;
    }
    const double S = (a + tsum + (double)Q.ck * kk) / (double)Q.c;
    for (int t = lane; t < Q.tg_count; t += 64) {
      const int row = at.tg_row[Q.tg_begin + t];
      at.fit[row] -= S / fb;
      at.reg[row] -= regu / fb;
    }
    const int k0 = at.qk_off[qi];
    for (int t = lane; t < Q.ck; t += 64) {
      const int row = at.qk_row[k0 + t];
      at.fit[row] -= (S - kk) / fb;
      at.reg[row] -= 2.0 * regu / fb;
    }
  }
  for (int j = w; j < P.t_count; j += 4) {
    const int cnt = stept[a4.w + j].z;
    const float* g = contrib + (size_t)(nq + a4.w + j) * DP;
    double a = 0.0;
    for (int i = lane; i < half; i += 64) {
      double vv[G];
      load_v(i, vv);
#pragma unroll
      for (int h = 0; h < G; ++h) a += vv[h] * (double)g[i + h * half];
    }
    a = at_wave_sum(a);
    const int t0 = at.t_off[P.t_begin + j];
    for (int t = lane; t < cnt; t += 64) {
      const int row = at.t_row[t0 + t];
      at.fit[row] -= a / (double)cnt / fb;
      at.reg[row] -= regu / fb;
    }
  }
}

// delta_s = <c_s, x_T - x_0> in fp64 from the fp32 rows: one wave per slot, lane-strided, then a
// butterfly
__global__ __launch_bounds__(256) void kp_cx_attrib_delta(int dp, int ns, const double* __restrict__ C,
                                                          const float* __restrict__ X, const float* __restrict__ X0,
                                                          double* __restrict__ delta) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= ns) return;
  const size_t so = (size_t)s * dp;
  double acc = 0.0;
  for (int d = lane; d < dp; d += 64) acc += C[so + d] * ((double)X[so + d] - (double)X0[so + d]);
  acc = at_wave_sum(acc);
  if (lane == 0) delta[s] = acc;
}

// ============================================================================
// kp_posttrain_rank_f64 (include/kelpie_hip.h, "fp64"): the same decomposition with the row,
// the queries, the attention (kp_attn64.hpp), the merge, the gradient, the regulariser term,
// the optimizer state and the update in fp64.  The small kernels are compiled over the row
// type (kp_cx_stepq, kp_cx_qpair, kp_cx_tsum, kp_cx_lse_merge, kp_cx_rankq64) and the host
// side below is written once over it; the merge and the update are the forms below: one
// partial per key range merged in range order where the fp32 form merges one per lane, and
// no trace or mark arguments.  Every sum has a fixed order.
// ============================================================================
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// kp_cx_contrib in fp64: one wave per (query or frozen-head row) of the step.  The formulas
// are kp_cx_contrib's; the ranges' partials O_s merge with the weights exp(m_s - lse), one
// range after the other in range order.
template <int DP, class Prod>
__global__ __launch_bounds__(256) void kp_cx_contrib64(int half, const int4* __restrict__ stepq, int nq,
                                                       const int4* __restrict__ stept, int nt,
                                                       const CxQuery* __restrict__ pq, const double* __restrict__ X,
                                                       const float* __restrict__ R, const double* __restrict__ Tsum,
                                                       const double* __restrict__ Qpair,
                                                       const double* __restrict__ lsef,
                                                       const double* __restrict__ att_m,
                                                       const double* __restrict__ att_l,
                                                       const double* __restrict__ att_O, int ranges,
                                                       double* __restrict__ contrib) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= nq + nt) return;
  double* out = contrib + (size_t)item * DP;
  constexpr int G = Prod::G;
  if (item < nq) {
    const int4 sq = stepq[item];  // slot, rel, plan-query index
    const double* x = X + (size_t)sq.x * DP;
    const float* rel = R + (size_t)sq.y * DP;
    const CxQuery Q = pq[sq.z];
    double z = 0.0;
    for (int d = lane; d < G * half; d += 64) z += Prod::q64(x, rel, d, half) * x[d];
    z = wave_sum64(z);
    const double lse_f = lse_ranges64(att_m, att_l, nq, ranges, item);
    const double hi = fmax(lse_f, z), lo = fmin(lse_f, z);
    const double lse = hi + log1p(exp(lo - hi));
    const double pk = exp(z - lse);
    constexpr int NI = (DP / G + 63) / 64;
    double o_k[NI][G];
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
      for (int h = 0; h < G; ++h) o_k[k][h] = 0.0;
    for (int sp = 0; sp < ranges; ++sp) {
      const double ms = att_m[(size_t)sp * nq + item];
      if (ms == -__builtin_inf()) continue;  // wave-uniform
      const double w0 = exp(ms - lse);
      const double* O0 = att_O + ((size_t)sp * nq + item) * DP;
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        const int i = lane + 64 * k;
        if (i < half) {
#pragma unroll
          for (int h = 0; h < G; ++h) o_k[k][h] += w0 * O0[i + h * half];
        }
      }
    }
    const double fc = (double)Q.c, fck = (double)Q.ck;
    const double cf = fc * pk - fck;
    const double* ts = Tsum + (size_t)sq.z * DP;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      const int i = lane + 64 * k;
      if (i >= half) continue;
      double xv[G], rv[G], dv[G];
#pragma unroll
      for (int h = 0; h < G; ++h) xv[h] = x[i + h * half];
#pragma unroll
      for (int h = 0; h < G; ++h) rv[h] = (double)rel[i + h * half];
#pragma unroll
      for (int h = 0; h < G; ++h) {
        const double e = o_k[k][h] + pk * xv[h];  // <E>: the frozen part and the kelpie column
        dv[h] = fc * e - ts[i + h * half] - fck * xv[h];
      }
      Prod::emit(out, i, half, xv, rv, dv, cf);
    }
  } else {
    const int4 st = stept[item - nq];  // slot, pair, count
    const double* x = X + (size_t)st.x * DP;
    const double* qp = Qpair + (size_t)st.y * DP;
    double z = 0.0;
    for (int d = lane; d < G * half; d += 64) z += qp[d] * x[d];
    z = wave_sum64(z);
    const double lf = lsef[st.y];
    const double hi = fmax(lf, z), lo = fmin(lf, z);
    const double lse = hi + log1p(exp(lo - hi));
    const double coef = (double)st.z * (exp(z - lse) - 1.0);
    for (int d = lane; d < G * half; d += 64) out[d] = coef * qp[d];
  }
}

// kp_cx_update in fp64: one workgroup per active slot; the slot's contribution rows summed in
// row order, 1 / B, the N3 / N2 term, then the optimizer in torch's op order on double state
template <int DP, class Prod>
__global__ __launch_bounds__(256) void kp_cx_update64(int half, const int4* __restrict__ act,
                                                      const CxPlan* __restrict__ plans, int nq,
                                                      const double* __restrict__ contrib, double* __restrict__ X,
                                                      double* __restrict__ S1, double* __restrict__ S2, CxOpt64 opt) {
  constexpr int G = Prod::G;
  const int tid = threadIdx.x;
  const int4 a4 = act[blockIdx.x];  // slot, plan, qoff, toff
  const int slot = a4.x;
  const CxPlan P = plans[a4.y];
  double* x = X + (size_t)slot * DP;
  const int nc = P.q_count + P.t_count;
  auto crow = [&](int j) -> const double* {
    return j < P.q_count ? contrib + (size_t)(a4.z + j) * DP : contrib + (size_t)(nq + a4.w + j - P.q_count) * DP;
  };
  const double fb = (double)P.b;
  double n2 = 0.0;
  if (opt.reg_w != 0.0 && opt.reg_n2) {  // ||f|| over the whole row, before the update
    __shared__ double n2red[4];
    double ps = 0.0;
    for (int i = tid; i < half; i += 256) {
      double xv[G];
#pragma unroll
      for (int h = 0; h < G; ++h) xv[h] = x[i + h * half];
      const double f = Prod::mod64(xv);
      ps += f * f;
    }
    ps = wave_sum64(ps);
    if ((tid & 63) == 0) n2red[tid >> 6] = ps;
    __syncthreads();
    n2 = sqrt((n2red[0] + n2red[1]) + (n2red[2] + n2red[3]));
  }
  double xs[(DP / G + 255) / 256][G], gs[(DP / G + 255) / 256][G];
#pragma unroll
  for (int u = 0; u < (DP / G + 255) / 256; ++u) {
    const int i = tid + 256 * u;
    if (i >= half) continue;
#pragma unroll
    for (int h = 0; h < G; ++h) {
      gs[u][h] = 0.0;
      xs[u][h] = x[i + h * half];
    }
    for (int j = 0; j < nc; ++j) {
      const double* c = crow(j);
#pragma unroll
      for (int h = 0; h < G; ++h) gs[u][h] += c[i + h * half];
    }
#pragma unroll
    for (int h = 0; h < G; ++h) gs[u][h] /= fb;
    if (opt.reg_w != 0.0) {
      const double mod = opt.reg_n2 ? n2 : Prod::mod64(xs[u]);
      const double k3 = 3.0 * opt.reg_w / fb * (double)(P.cnt_l + P.cnt_r) * mod;
#pragma unroll
      for (int h = 0; h < G; ++h) gs[u][h] += k3 * xs[u][h];
    }
  }
  // (the N2 norm above read the whole row: every thread has it before any element moves)
  __syncthreads();
#pragma unroll
  for (int u = 0; u < (DP / G + 255) / 256; ++u) {
    const int i = tid + 256 * u;
    if (i >= half) continue;
#pragma unroll
    for (int h = 0; h < G; ++h) {
      const int d = i + h * half;
      const double gd = gs[u][h];
      double xd = xs[u][h];
      const size_t o = (size_t)slot * DP + d;
      if (opt.kind == KP_OPT_ADAGRAD) {
        double s1 = S1[o];
        s1 = s1 + gd * gd;
        const double stdv = sqrt(s1) + opt.eps;
        xd = xd + (-opt.lr * gd) / stdv;
        S1[o] = s1;
      } else if (opt.kind == KP_OPT_ADAM) {
        double m1 = S1[o], v2 = S2[o];
        m1 = m1 + opt.one_minus_b1 * (gd - m1);
        v2 = v2 * opt.b2;
        v2 = v2 + (opt.one_minus_b2 * gd) * gd;
        const double den = sqrt(v2) / opt.bc2_sqrt + opt.eps;
        xd = xd + (-opt.step_size * m1) / den;
        S1[o] = m1;
        S2[o] = v2;
      } else {
        xd = xd + (-opt.lr) * gd;
      }
      x[d] = xd;
    }
  }
}

// fp64 ranking queries (launch_rank_f64): q_s = x_s o R[p_s] from exact fp64 products of
// the fp32 operands; the target score q_s . E_o and the kelpie column q_s . x_s as one
// sequential fp64 FMA chain over d (the order kp_rank_f64_count scores every entity in).
// Row s of a set of rank rows is pred[3 s ..] = (row, p, o): x is row `row` of X (the slots: s
// itself; a probe: its slot's kelpie row; a mark row: its row of the mark workspace).
// XT: the kelpie rows' type (double: kp_posttrain_rank_f64, whose row is never rounded)
template <int DP, class Prod, class XT = float>
__global__ void kp_cx_rankq64(const XT* __restrict__ X, const float* __restrict__ R, const float* __restrict__ E,
                              int n_ent, int half, const int32_t* __restrict__ pred, int n_slots,
                              double* __restrict__ Q, double* __restrict__ t64, double* __restrict__ kcol64) {
  const int s = blockIdx.x;
  if (s >= n_slots) return;
  const XT* x = X + (size_t)pred[3 * s] * DP;
  const float* rel = R + (size_t)pred[3 * s + 1] * DP;
  double* q = Q + (size_t)s * DP;
  for (int d = threadIdx.x; d < DP; d += blockDim.x) q[d] = Prod::q64(x, rel, d, half);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int o = pred[3 * s + 2];
    double z = 0.0, t = 0.0;
    for (int d = 0; d < DP; ++d) z = __fma_rn(q[d], (double)x[d], z);
    if (o < n_ent) {
      const float* eo = E + (size_t)o * DP;
      for (int d = 0; d < DP; ++d) t = __fma_rn(q[d], (double)eo[d], t);
    } else {
      t = z;  // the kelpie entity is its own object
    }
    kcol64[s] = z;
    t64[s] = t;
  }
}

template <class Prod>
__global__ void kp_cx_scoreq(const float* __restrict__ E, const float* __restrict__ R, int dp, int half,
                             const int32_t* __restrict__ heads, const int32_t* __restrict__ rels, int n,
                             float* __restrict__ Q) {
  int s = blockIdx.x;
  if (s >= n) return;
  const float* lhs = E + (size_t)heads[s] * dp;
  const float* rel = R + (size_t)rels[s] * dp;
  for (int d = threadIdx.x; d < dp; d += blockDim.x) Q[(size_t)s * dp + d] = Prod::q(lhs, rel, d, half);
}

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
// step queries q_j = x_slot o R_rel (complex.py:65-72), one row per step query
// (XT: the rows' and the queries' type; double: kp_posttrain_rank_f64)
template <int DP, class Prod, class XT = float>
__global__ void kp_cx_stepq(const XT* __restrict__ X, const float* __restrict__ R, int half,
                            const int4* __restrict__ stepq, int nq, XT* __restrict__ Q) {
  const int j = blockIdx.x;
  if (j >= nq) return;
  const int4 sq = stepq[j];
  const XT* x = X + (size_t)sq.x * DP;
  const float* rel = R + (size_t)sq.y * DP;
  for (int d = threadIdx.x; d < DP; d += blockDim.x) Q[(size_t)j * DP + d] = cx_q_as<Prod, XT>(x, rel, d, half);
}

template <int DB, class Prod, class XT = float>
void launch_stepq(kp_ctx* c, const int4* stepq, const XT* X, int nq, XT* Q) {
  if (nq <= 0) return;
  hipLaunchKernelGGL((kp_cx_stepq<16 * DB, Prod, XT>), dim3(nq), dim3(64), 0, c->stream, X, c->dR, Prod::extent(c->dim), stepq,
                     nq, Q);
  KP_HIP(hipGetLastError());
}

// co-resident attention workgroups: LDS and registers allow two per CU for rows up
// to 208 floats, one for wider rows
// (kp_attn3: as many as the occupancy API reports)
template <int DB>
int attn_slots_db(kp_ctx* c) {
  if (c->attn_mode == 1) return c->n_cu * attn3_wpc<DB>(c);
  return c->n_cu * (DB <= 13 ? 2 : 1);
}

template <int DB>
void launch_attn(kp_ctx* c, bool with_o, const float* Q, int nq, const AttnPlan& plan, float* m, float* l,
                 float* O) {
  if (nq <= 0) return;
  if (c->attn_mode == 1) {
    if (with_o)
      launch_attn3<DB, ATT_SOFTMAX_O>(c, c->n_ent, Q, nq, plan, m, l, O, nullptr, 0.f);
    else
      launch_attn3<DB, ATT_SOFTMAX>(c, c->n_ent, Q, nq, plan, m, l, O, nullptr, 0.f);
    return;
  }
  const size_t shm = attn_lds_bytes(DB);
  if (with_o)
    hipLaunchKernelGGL((kp_attn<DB, ATT_SOFTMAX_O>), dim3(plan.n_wg), dim3(256), shm, c->stream, c->dE, c->n_ent, Q,
                       nq, plan.wk, m, l, O, nullptr, 0.f);
  else
    hipLaunchKernelGGL((kp_attn<DB, ATT_SOFTMAX>), dim3(plan.n_wg), dim3(256), shm, c->stream, c->dE, c->n_ent, Q,
                       nq, plan.wk, m, l, O, nullptr, 0.f);
  KP_HIP(hipGetLastError());
}

// kp_posttrain_rank_trace's device side (loss == nullptr: no trace): the common part and
// ComplEx's own workspaces
struct CxTraceDev : TraceDev {
  double *term = nullptr, *freg_e = nullptr, *freg_r = nullptr;
  const int32_t* targets = nullptr;
  const int2* pairs = nullptr;
};

template <int DB, class Prod>
void launch_update(kp_ctx* c, int n_act, const int4* act, const CxPlan* plans, const CxQuery* pq,
                   const int4* stepq, int nq, const int4* stept, int nt, const float* tsum, const float* qpair,
                   const float* lsef, const float* am, const float* al, const float* aO, int n_split, float* contrib,
                   float* X, float* S1, float* S2, const CxOpt& opt, const CxTraceDev& tr = {}, int step = 0,
                   const CxMarkArgs<true>* mk = nullptr, const CxAttribDev* at = nullptr,
                   const int32_t* targets = nullptr) {
  if (n_act <= 0) return;
  const int half = Prod::extent(c->dim);
  KP_REQUIRE(n_split >= 1 && n_split <= 64, "cx contrib: one attention split per lane");
  if (nq + nt > 0 && !tr.loss) {
    hipLaunchKernelGGL((kp_cx_contrib<16 * DB, Prod>), dim3((nq + nt + 3) / 4), dim3(256), 0, c->stream, half, stepq, nq,
                       stept, nt, pq, X, c->dR, tsum, qpair, lsef, am, al, aO, n_split, contrib, CxTraceArgs<false>{});
    KP_HIP(hipGetLastError());
  }
  if (tr.loss) {  // kp_posttrain_rank_trace: the items' loss terms, then the slots' losses, before x moves
    if (nq + nt > 0) {
      hipLaunchKernelGGL((kp_cx_contrib<16 * DB, Prod, true>), dim3((nq + nt + 3) / 4), dim3(256), 0, c->stream, half,
                         stepq, nq, stept, nt, pq, X, c->dR, tsum, qpair, lsef, am, al, aO, n_split, contrib,
                         CxTraceArgs<true>{tr.term});
      KP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((kp_cx_trace_sum<16 * DB, Prod>), dim3(n_act), dim3(64), 0, c->stream, half, act, plans, pq,
                       tr.targets, tr.pairs, stept, nq, X, tr.term, tr.freg_e, tr.freg_r, opt.reg_w, opt.reg_n2,
                       tr.off, step, tr.loss);
    KP_HIP(hipGetLastError());
  }
  if (at) {  // kp_posttrain_rank_attrib: the ATTRIB forms, then the step's attributions from what they left
    const CxAttribArgs<true> aa{at->D, at->xprev, at->n2};
    if (mk)
      hipLaunchKernelGGL((kp_cx_update<16 * DB, Prod, true, true>), dim3(n_act), dim3(256), 0, c->stream, half, act,
                         plans, nq, contrib, X, S1, S2, opt, *mk, aa);
    else
      hipLaunchKernelGGL((kp_cx_update<16 * DB, Prod, false, true>), dim3(n_act), dim3(256), 0, c->stream, half, act,
                         plans, nq, contrib, X, S1, S2, opt, CxMarkArgs<false>{}, aa);
    KP_HIP(hipGetLastError());
    hipLaunchKernelGGL((kp_cx_attrib<16 * DB, Prod>), dim3(n_act), dim3(256), 0, c->stream, half, act, plans, pq, targets,
                       stept, nq, contrib, c->dE, c->dR, opt.reg_w, opt.reg_n2, *at);
    KP_HIP(hipGetLastError());
    return;
  }
  if (mk)  // a step that ends a marked epoch of one of its slots: the MARKS form instead, not a further launch
    hipLaunchKernelGGL((kp_cx_update<16 * DB, Prod, true>), dim3(n_act), dim3(256), 0, c->stream, half, act, plans, nq,
                       contrib, X, S1, S2, opt, *mk, CxAttribArgs<false>{});
  else
    hipLaunchKernelGGL((kp_cx_update<16 * DB, Prod>), dim3(n_act), dim3(256), 0, c->stream, half, act, plans, nq, contrib,
                       X, S1, S2, opt, CxMarkArgs<false>{}, CxAttribArgs<false>{});
  KP_HIP(hipGetLastError());
}

// kp_posttrain_rank_f64's: the fp64 forms, any number of key ranges, no trace and no marks
template <int DB, class Prod>
void launch_update(kp_ctx* c, int n_act, const int4* act, const CxPlan* plans, const CxQuery* pq,
                   const int4* stepq, int nq, const int4* stept, int nt, const double* tsum, const double* qpair,
                   const double* lsef, const double* am, const double* al, const double* aO, int ranges,
                   double* contrib, double* X, double* S1, double* S2, const CxOpt64& opt, const CxTraceDev& = {},
                   int = 0, const CxMarkArgs<true>* = nullptr, const CxAttribDev* = nullptr,
                   const int32_t* = nullptr) {
  if (n_act <= 0) return;
  const int half = Prod::extent(c->dim);
  if (nq + nt > 0) {
    hipLaunchKernelGGL((kp_cx_contrib64<16 * DB, Prod>), dim3((nq + nt + 3) / 4), dim3(256), 0, c->stream, half, stepq,
                       nq, stept, nt, pq, X, c->dR, tsum, qpair, lsef, am, al, aO, ranges, contrib);
    KP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((kp_cx_update64<16 * DB, Prod>), dim3(n_act), dim3(256), 0, c->stream, half, act, plans, nq,
                     contrib, X, S1, S2, opt);
  KP_HIP(hipGetLastError());
}

// the fp64 queries of the rows [r0, r0 + m) of a set of rank rows, on the rows X, into the
// set's chunk buffers
template <int DB, class Prod, class XT = float>
void launch_rankq64(kp_ctx* c, const XT* X, const RankSet& rr, int r0, int m) {
  hipLaunchKernelGGL((kp_cx_rankq64<16 * DB, Prod, XT>), dim3(m), dim3(64), 0, c->stream, X, c->dR, c->dE, c->n_ent,
                     Prod::extent(c->dim), rr.rows + 3 * (size_t)r0, m, rr.q, rr.t, rr.kcol);
  KP_HIP(hipGetLastError());
}

#define CX_DISPATCH(DBV, ...) \
  KP_DB_DISPATCH(DBV, 1, "ComplEx / DistMult: unsupported padded dimension", __VA_ARGS__)

// Everything below is written once over the row type T: float, or double for
// kp_posttrain_rank_f64 (rq.f64).  What a precision has of its own is an overload or an
// `if constexpr`: the hyper-parameters' source, x0, the attention (CxAttn), launch_update,
// the downloads.
template <class T>
constexpr bool is_f64 = std::is_same_v<T, double>;

// the optimizer's constants of a call (step_size and bc2_sqrt follow per step): kp_hp's
// floats, or kp_f64's doubles
template <class T>
CxOptT<T> make_opt(const kp_hp* hp, const kp_f64* f) {
  CxOptT<T> opt{};
  opt.kind = hp->optimizer;
  if constexpr (is_f64<T>)
    opt.lr = f->lr, opt.b1 = f->beta1, opt.b2 = f->beta2, opt.eps = f->eps, opt.reg_w = f->reg_weight;
  else
    opt.lr = hp->lr, opt.b1 = hp->beta1, opt.b2 = hp->beta2, opt.eps = hp->eps, opt.reg_w = hp->reg_weight;
  opt.one_minus_b1 = (T)(1.0 - (double)opt.b1);
  opt.one_minus_b2 = (T)(1.0 - (double)opt.b2);
  opt.reg_n2 = hp->reg_kind == KP_REG_N2;
  return opt;
}
// Adam's scalars of step t: adam_step's, or torch's on the double hyper-parameters
inline void set_adam_step(CxOpt& opt, const kp_hp* hp, int t) {
  const AdamStep as = adam_step(hp, t);
  opt.step_size = as.step_size;
  opt.bc2_sqrt = as.bc2_sqrt;
}
inline void set_adam_step(CxOpt64& opt, const kp_hp*, int t) {
  const double step = (double)(t + 1);
  opt.step_size = opt.lr / (1.0 - std::pow(opt.b1, step));
  opt.bc2_sqrt = std::sqrt(1.0 - std::pow(opt.b2, step));
}

// The attention of a call: plan() plans the frozen-head pairs' launch and every step's, notes
// the largest hot one (kp_last_attn_plan) and returns the partial rows (queries x parts) the
// largest launch writes; launch() and parts() take the step t, or -1 for the pairs' launch.
// fp32: a plan per launch for the batches in flight (attn_plan_ctx), kp_attn / kp_attn3
struct CxAttn32 {
  AttnPlan pairs;
  std::vector<AttnPlan> step;  // [T]
  size_t plan(kp_ctx* c, const CxStepPlan& sp, int npairs) {
    int slots = 0;
    CX_DISPATCH(c->dp / 16, slots = attn_slots_db<DB>(c));
    pairs = attn_plan_ctx(c, std::max(npairs, 1), c->n_ent, slots, true);
    size_t rows = (size_t)std::max(npairs, 1) * pairs.wk.n_parts;
    step.resize(sp.T);
    for (int t = 0; t < sp.T; ++t) {
      const int nq = sp.q_off[t + 1] - sp.q_off[t];
      step[t] = attn_plan_ctx(c, std::max(nq, 1), c->n_ent, slots, true);
      if (nq > 0) attn_plan_note(c, step[t], nq, true);
      rows = std::max(rows, (size_t)nq * step[t].wk.n_parts);
    }
    return rows;
  }
  int parts(int t) const { return (t < 0 ? pairs : step[t]).wk.n_parts; }
  template <int DB>
  void launch(kp_ctx* c, int t, bool with_o, const float* Q, int nq, float* m, float* l, float* O) const {
    launch_attn<DB>(c, with_o, Q, nq, t < 0 ? pairs : step[t], m, l, O);
  }
};
// fp64: the key ranges of the call's largest launch for every launch (the planner's S,
// attn_plan_ranges; KP_ATTN_RANGES=S forces S as it does for kp_attn3), in whole 32-key planner
// tiles: one S for the whole call keeps the partials' layout fixed.  kp_attn64, one workgroup
// per (16 queries, range), never shared with a batch in flight
struct CxAttn64 {
  int ranges = 1, keys_per_range = 0;
  size_t plan(kp_ctx* c, const CxStepPlan& sp, int npairs) {
    const int max_nq = std::max(1, std::max(sp.max_nq, npairs));
    const AttnPlan p = c->attn_ranges > 0 ? attn_plan_oneshot(max_nq, c->n_ent, c->attn_ranges)
                                          : attn_plan_ranges(max_nq, c->n_ent, c->n_cu);
    ranges = std::max(1, p.wk.ranges);
    keys_per_range = (p.wk.ktq + ranges - 1) / ranges * 32;
    for (int t = 0; t < sp.T; ++t) {
      const int nq = sp.q_off[t + 1] - sp.q_off[t];
      if (nq > 0 && nq >= c->attn_last.nq) c->attn_last = {nq, 1, ranges, ranges, (nq + A64_QT - 1) / A64_QT * ranges};
    }
    return (size_t)max_nq * ranges;
  }
  int parts(int) const { return ranges; }
  template <int DB>
  void launch(kp_ctx* c, int, bool with_o, const double* Q, int nq, double* m, double* l, double* O) const {
    launch_attn64<DB>(c, with_o, Q, nq, ranges, keys_per_range, m, l, O);
  }
};

// the device side of one call: the plan's uploads and the workspaces (c->cx.step<T>(), c->rank)
template <class T>
struct CxDev {
  T *X, *S1, *S2;  // kelpie rows and optimizer state [ns][dp]
  CxPlan* plans;
  CxQuery* pq;
  int32_t* tg;
  int2* pairs;
  int4 *acts, *stepq, *stept;
  T *contrib, *tsum, *qpair, *lsef;
  // the slots, kp_posttrain_rank_probes; the trace; the marks (fp64: offered none of the three,
  // so the empty ones their upload_* return)
  RankSet rk, probes;
  CxTraceDev trace;
  MarksDev marks;
  int32_t* mark_row = nullptr;  // [acts] the mark row an active entry's update also stores, or -1
  CxAttribDev attrib;           // kp_posttrain_rank_attrib, when with_attrib
  bool with_attrib = false;
  // the attention's: sized and planned by cx_preloop
  T *am = nullptr, *al = nullptr, *ao = nullptr, *qs = nullptr;
  std::conditional_t<is_f64<T>, CxAttn64, CxAttn32> attn;
};

// the plan's element types are the HIP vector types' layout: their arrays are uploaded as such
static_assert(sizeof(CxI2) == sizeof(int2) && alignof(CxI2) == alignof(int2), "CxI2 is int2");
static_assert(sizeof(CxI4) == sizeof(int4) && alignof(CxI4) == alignof(int4), "CxI4 is int4");
inline const int2* as_dev(const CxI2* p) { return reinterpret_cast<const int2*>(p); }
inline const int4* as_dev(const CxI4* p) { return reinterpret_cast<const int4*>(p); }

// x0 zero-padded to [ns][dp] in `xp` and uploaded: the batch's fp32 rows (or the keyed draws,
// upload_x0), or kp_f64's double rows
inline float* cx_upload_x0(kp_ctx* c, DevBuf& b, const kp_batch* bt, const PostReq& rq, std::vector<float>& xp) {
  return upload_x0(c, b, bt, xp, rq.keyed);
}
inline double* cx_upload_x0(kp_ctx* c, DevBuf& b, const kp_batch* bt, const PostReq& rq, std::vector<double>& xp) {
  xp.assign((size_t)bt->n_slots * c->dp, 0.0);
  for (int s = 0; s < bt->n_slots; ++s)
    std::memcpy(&xp[(size_t)s * c->dp], rq.f64->x0 + (size_t)s * c->dim, sizeof(double) * c->dim);
  return upload(c, b, xp.data(), xp.size());
}
// the fp32 rows a set of rank rows names as its X; the fp64 call's sets name none (their
// queries read the double rows)
inline const float* rank_x(const float* X) { return X; }
inline const float* rank_x(const double*) { return nullptr; }
inline const float* query_x(const RankSet& rr, const float*) { return rr.X; }
inline const double* query_x(const RankSet&, const double* X) { return X; }

template <class T>
CxDev<T> cx_workspaces(kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq, const CxStepPlan& sp,
                       std::vector<T>& xp) {
  const int ns = bt->n_slots, DP = c->dp;
  CxStepWs& w = c->cx.step<T>();
  CxDev<T> d;
  d.X = cx_upload_x0(c, w.x, bt, rq, xp);
  d.S1 = ensure_n<T>(w.s1, (size_t)ns * DP);
  d.S2 = ensure_n<T>(w.s2, (size_t)ns * DP);
  KP_HIP(hipMemsetAsync(d.S1, 0, sizeof(T) * (size_t)ns * DP, c->stream));
  KP_HIP(hipMemsetAsync(d.S2, 0, sizeof(T) * (size_t)ns * DP, c->stream));
  d.plans = upload(c, w.plans, sp.plans.data(), sp.plans.size());
  d.pq = upload(c, w.queries, sp.pqs.data(), sp.pqs.size());
  d.tg = upload(c, w.targets, sp.targets.data(), sp.targets.size());
  d.pairs = upload(c, w.pairs, as_dev(sp.pairs.data()), sp.pairs.size());
  d.acts = upload(c, w.acts, as_dev(sp.acts.data()), sp.acts.size());
  // (empty without a step, epochs == 0: upload() then only sizes the buffer)
  d.stepq = upload(c, w.stepq, as_dev(sp.stepq.data()), sp.stepq.size());
  d.stept = upload(c, w.stept, as_dev(sp.stept.data()), sp.stept.size());
  d.contrib = ensure_n<T>(w.contrib, (size_t)std::max(1, sp.max_items) * DP);
  const int npq = (int)sp.pqs.size(), npairs = (int)sp.pairs.size();
  d.tsum = ensure_n<T>(w.tsum, (size_t)std::max(npq, 1) * DP);
  d.qpair = ensure_n<T>(w.qpair, (size_t)std::max(npairs, 1) * DP);
  d.lsef = ensure_n<T>(w.lsef, (size_t)std::max(npairs, 1));

  // the ranking's inputs and buffers now, ahead of the step loop: an upload from pageable
  // memory after the loop waited for the whole loop on the device, so the rank kernels
  // were enqueued only then (a host round trip per batch with the context idle)
  // (the fp64 call's slots are a set of rank rows of its own, c->rank.f64)
  const float* xr = rank_x(d.X);
  d.rk = upload_slots(c, is_f64<T> ? c->rank.f64 : c->rank.slots, bt, rq, xr);
  d.probes = upload_probes(c, bt, rq, xr);
  // kp_posttrain_rank_marks: the mark rows (each the padded x0 until a step captures it)
  d.marks = upload_marks(c, c->cx.marks, hp, bt, rq, xr);
  if (d.marks.nm > 0) {
    const std::vector<int32_t> mr = marks_act_rows(d.marks, sp.act_off, sp.T, [&](int i) { return sp.acts[i].x; });
    d.mark_row = upload(c, c->cx.mark_row, mr.data(), mr.size());
  }
  if constexpr (!is_f64<T>) {
    if (rq.attrib) {  // the row map and the attributions' workspaces, with the call's other uploads
      CxRowMap m;
      if (const char* why = cx_row_map(c->n_ent, hp->batch_size, hp->epochs, bt, sp, m))
        throw KpError{KP_EINVAL, std::string(kp_model_name(c->model)) + ": attributions: " + why};
      // one upload: tg_row | qk_off | qk_row | t_off | t_row
      std::vector<int32_t> pack;
      const auto put = [&pack](const std::vector<int32_t>& v) {
        const size_t at = pack.size();
        pack.insert(pack.end(), v.begin(), v.end());
        return at;
      };
      const size_t o0 = put(m.tg_row), o1 = put(m.qk_off), o2 = put(m.qk_row), o3 = put(m.t_off), o4 = put(m.t_row);
      const int32_t* dm = upload(c, c->cx.at_map, pack.data(), pack.size());
      CxAttribDev& a = d.attrib;
      a.tg_row = dm + o0, a.qk_off = dm + o1, a.qk_row = dm + o2, a.t_off = dm + o3, a.t_row = dm + o4;
      const size_t nx = (size_t)ns * DP;
      a.rows = bt->row_off[ns];
      a.c = ensure_n<double>(c->cx.at_c, nx);
      a.D = ensure_n<float>(c->cx.at_f, 3 * nx + (size_t)ns);
      a.xprev = a.D + nx;
      a.x0 = a.xprev + nx;
      a.n2 = a.x0 + nx;
      a.fit = ensure_n<double>(c->cx.at_out, 2 * (size_t)a.rows + (size_t)ns);
      a.reg = a.fit + a.rows;
      a.delta = a.reg + a.rows;
      KP_HIP(hipMemsetAsync(a.fit, 0, sizeof(double) * (2 * (size_t)a.rows + (size_t)ns), c->stream));
      KP_HIP(hipMemcpyAsync(a.x0, d.X, sizeof(float) * nx, hipMemcpyDeviceToDevice, c->stream));
      d.with_attrib = true;
    }
  }
  if (rq.trace) {  // the trace's offsets and workspaces, with the call's other uploads
    CxTraceDev& t = d.trace;
    static_cast<TraceDev&>(t) = upload_trace(c, bt, rq);
    t.term = ensure_n<double>(c->cx.tr_term, (size_t)std::max(1, sp.max_items));
    t.freg_e = ensure_n<double>(c->cx.tr_fe, (size_t)c->n_ent);
    t.freg_r = ensure_n<double>(c->cx.tr_fr, (size_t)c->n_rel2);
    t.targets = d.tg;
    t.pairs = d.pairs;
  }
  return d;
}

// before the loop: the queries' frozen-target sums, the attention plans and workspaces of
// every step, and the frozen-head pairs' q and frozen log-sum-exp
template <class Prod, class T>
void cx_preloop(kp_ctx* c, const CxStepPlan& sp, CxDev<T>& d, const CxOptT<T>& opt) {
  const int DP = c->dp, DBV = DP / 16;
  const int npq = (int)sp.pqs.size(), npairs = (int)sp.pairs.size();
  CxStepWs& w = c->cx.step<T>();
  KP_HIP(hipEventRecord(c->ev0, c->stream));
  if (npq > 0) {
    hipLaunchKernelGGL(kp_cx_tsum<T>, dim3(npq), dim3(128), 0, c->stream, c->dE, DP, d.pq, npq, d.tg, d.tsum);
    KP_HIP(hipGetLastError());
  }
  if (d.trace.loss && opt.reg_w != 0 && sp.T > 0) {  // the frozen rows' regulariser factors, once per batch
    const int half = Prod::extent(c->dim);
    hipLaunchKernelGGL(kp_cx_rowreg<Prod>, dim3((c->n_ent + 3) / 4), dim3(256), 0, c->stream, c->dE, c->n_ent, DP, half,
                       opt.reg_n2, d.trace.freg_e);
    KP_HIP(hipGetLastError());
    hipLaunchKernelGGL(kp_cx_rowreg<Prod>, dim3((c->n_rel2 + 3) / 4), dim3(256), 0, c->stream, c->dR, c->n_rel2, DP,
                       half, opt.reg_n2, d.trace.freg_r);
    KP_HIP(hipGetLastError());
  }
  if constexpr (!is_f64<T>) {
    if (d.with_attrib) {  // the slots' score gradients, once per batch (the slots' rank rows are (s, p, o))
      const int ns = d.rk.n;
      CX_DISPATCH(DBV, hipLaunchKernelGGL((kp_cx_attrib_c<16 * DB, Prod>), dim3(ns), dim3(64), 0, c->stream,
                                          Prod::extent(c->dim), c->dE, c->dR, d.rk.rows, ns, d.attrib.c));
      KP_HIP(hipGetLastError());
    }
  }
  c->attn_last = {};
  const size_t att_rows = d.attn.plan(c, sp, npairs);
  d.am = ensure_n<T>(w.am, att_rows);
  d.al = ensure_n<T>(w.al, att_rows);
  d.ao = ensure_n<T>(w.ao, att_rows * DP);
  d.qs = ensure_n<T>(w.qs, (size_t)std::max(sp.max_nq, 1) * DP);
  if (npairs > 0) {
    hipLaunchKernelGGL((kp_cx_qpair<Prod, T>), dim3(npairs), dim3(128), 0, c->stream, c->dE, c->dR, DP,
                       Prod::extent(c->dim), d.pairs, npairs, d.qpair);
    KP_HIP(hipGetLastError());
    CX_DISPATCH(DBV, d.attn.template launch<DB>(c, -1, false, d.qpair, npairs, d.am, d.al, nullptr));
    // combine the partials into lsef on the device (no host round trip inside the batch)
    hipLaunchKernelGGL(kp_cx_lse_merge<T>, dim3((npairs + 255) / 256), dim3(256), 0, c->stream, npairs,
                       d.attn.parts(-1), d.am, d.al, d.lsef);
    KP_HIP(hipGetLastError());
  }
}

// the epoch/step loop: per step the queries, their attention over the frozen entities and
// the update of every active slot.  Returns the hot (attention) launches; t_steps: the host
// time after enqueueing steps 0, 1, T/2, T-1 (KP_HOST_TIMES)
template <class Prod, class T>
int64_t cx_step_loop(kp_ctx* c, const kp_hp* hp, const CxStepPlan& sp, const CxDev<T>& d, CxOptT<T> opt,
                     double* t_steps) {
  const int DBV = c->dp / 16, steps = sp.T;
  int64_t hot_launches = 0;
  c->hot_pairs.clear();
  c->hot_iv.clear();
  for (int t = 0; t < steps; ++t) {
    const int nq = sp.q_off[t + 1] - sp.q_off[t];
    const int na = sp.act_off[t + 1] - sp.act_off[t];
    hipEvent_t ea = nullptr, eb = nullptr;
    if (nq > 0 && c->time_hot) {
      ea = c->event(2 * hot_launches);
      eb = c->event(2 * hot_launches + 1);
    }
    CX_DISPATCH(DBV, (launch_stepq<DB, Prod, T>(c, d.stepq + sp.q_off[t], d.X, nq, d.qs)));
    if (nq > 0 && c->time_hot) KP_HIP(hipEventRecord(ea, c->stream));
    CX_DISPATCH(DBV, d.attn.template launch<DB>(c, t, true, d.qs, nq, d.am, d.al, d.ao));
    if (nq > 0) {
      if (c->time_hot) {
        KP_HIP(hipEventRecord(eb, c->stream));
        c->hot_pairs.push_back({(double)nq, 0.0});
      }
      ++hot_launches;
    }
    set_adam_step(opt, hp, t);
    const CxMarkArgs<true> mk{d.mark_row ? d.mark_row + sp.act_off[t] : nullptr, d.marks.X};
    CX_DISPATCH(DBV, launch_update<DB, Prod>(c, na, d.acts + sp.act_off[t], d.plans, d.pq, d.stepq + sp.q_off[t], nq,
                                             d.stept + sp.t_off[t], sp.t_off[t + 1] - sp.t_off[t], d.tsum, d.qpair,
                                             d.lsef, d.am, d.al, d.ao, d.attn.parts(t), d.contrib, d.X, d.S1, d.S2,
                                             opt, d.trace, t, marks_at_step(d.marks, t) ? &mk : nullptr,
                                             d.with_attrib ? &d.attrib : nullptr, d.tg));
    if (g_host_times) {
      if (t == 0) t_steps[0] = host_ms();
      if (t == 1) t_steps[1] = host_ms();
      if (t == steps / 2) t_steps[2] = host_ms();
      if (t == steps - 1) t_steps[3] = host_ms();
    }
  }
  return hot_launches;
}

// the tail of a call (returns the host time at which the wait began, KP_HOST_TIMES): every
// result the fp32 call was asked for (download_results); or the fp64 call's rows (when out_x
// is set), its fp64 target values as out_score and its ranks, one wait, the rows' unpadding
inline double cx_download(kp_ctx* c, const kp_batch* bt, const PostReq& rq, const CxDev<float>& d,
                          std::vector<float>& xp) {
  if (d.with_attrib) {  // delta from the final rows, then the three results with the call's other downloads
    const CxAttribDev& a = d.attrib;
    const int ns = bt->n_slots;
    hipLaunchKernelGGL(kp_cx_attrib_delta, dim3((ns + 3) / 4), dim3(256), 0, c->stream, c->dp, ns, a.c, d.X, a.x0,
                       a.delta);
    KP_HIP(hipGetLastError());
    if (a.rows > 0) {
      KP_HIP(hipMemcpyAsync(rq.attrib->out_fit, a.fit, sizeof(double) * a.rows, hipMemcpyDeviceToHost, c->stream));
      KP_HIP(hipMemcpyAsync(rq.attrib->out_reg, a.reg, sizeof(double) * a.rows, hipMemcpyDeviceToHost, c->stream));
    }
    KP_HIP(hipMemcpyAsync(rq.attrib->out_delta, a.delta, sizeof(double) * ns, hipMemcpyDeviceToHost, c->stream));
  }
  return download_results(c, bt, d.X, d.rk, xp, rq, d.probes, d.trace, d.marks);
}
inline double cx_download(kp_ctx* c, const kp_batch* bt, const PostReq& rq, const CxDev<double>& d,
                          std::vector<double>& xp) {
  const kp_f64& f = *rq.f64;
  const int ns = bt->n_slots;
  if (f.out_x) KP_HIP(hipMemcpyAsync(xp.data(), d.X, sizeof(double) * xp.size(), hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipMemcpyAsync(f.out_score, d.rk.t, sizeof(double) * ns, hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipMemcpyAsync(bt->out_rank, d.rk.rank, sizeof(int64_t) * ns, hipMemcpyDeviceToHost, c->stream));
  const double t_wait = g_host_times ? host_ms() : 0.0;
  KP_HIP(hipStreamSynchronize(c->stream));
  if (f.out_x)
    for (int s = 0; s < ns; ++s)
      std::memcpy(f.out_x + (size_t)s * c->dim, &xp[(size_t)s * c->dp], sizeof(double) * c->dim);
  return t_wait;
}

// loop-interval events, destroyed on every exit path (a KP_HIP / KP_REQUIRE throws)
struct LoopEvents {
  hipEvent_t a = nullptr, b = nullptr;
  ~LoopEvents() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// a checked and planned call on the device, in the row type T: workspaces, the step loop, the
// ranks, the downloads and the timing
template <class Prod, class T>
void cx_run(kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq, const CxStepPlan& sp, double t_in,
            double t_plan) {
  const CxOptT<T> opt = make_opt<T>(hp, rq.f64);
  std::vector<T> xp;
  CxDev<T> d = cx_workspaces<T>(c, hp, bt, rq, sp, xp);
  cx_preloop<Prod>(c, sp, d, opt);

  LoopEvents lev;
  KP_HIP(hipEventCreate(&lev.a));
  KP_HIP(hipEventCreate(&lev.b));
  KP_HIP(hipEventRecord(lev.a, c->stream));
  const double t_loop0 = g_host_times ? host_ms() : 0.0;
  double t_steps[4] = {0, 0, 0, 0};
  const int64_t hot_launches = cx_step_loop<Prod>(c, hp, sp, d, opt, t_steps);
  KP_HIP(hipEventRecord(lev.b, c->stream));

  // ---- ranking: scores of (kelpie, p, .) over E plus the kelpie column, in fp64
  // (launch_rank_f64: at the reference init the target's neighbours are ~1e-5 relative away)
  // the slots, then the probes on the slots' rows, then the marks on the mark workspace; the
  // fp64 call's slots on its double rows (its out_score is the set's fp64 target value itself)
  const auto queries = [c, X = d.X](const RankSet& rr, int r0, int m) {
    CX_DISPATCH(c->dp / 16, (launch_rankq64<DB, Prod, T>(c, query_x(rr, X), rr, r0, m)));
  };
  for (const RankSet* set : {&d.rk, &d.probes, &d.marks.rows}) rank_rows(c, *set, RANK64_DOT, queries);
  KP_HIP(hipEventRecord(c->ev1, c->stream));

  const double t_enq = cx_download(c, bt, rq, d, xp);
  const double t_done = g_host_times ? host_ms() : 0.0;
  if (g_host_times)
    std::fprintf(stderr,
                 "[kp_cx] slots %d steps %d: plan %.2f ms, enqueue %.2f ms (uploads+pairs %.2f, step 0 %.2f, step 1 "
                 "%.2f, to T/2 %.2f, to T-1 %.2f), wait %.2f ms\n",
                 bt->n_slots, sp.T, t_plan - t_in, t_enq - t_plan, t_loop0 - t_plan, t_steps[0] - t_loop0,
                 t_steps[1] - t_steps[0], t_steps[2] - t_steps[1], t_steps[3] - t_steps[2], t_done - t_enq);
  record_hot_timing(c, hot_launches, lev.a, lev.b);
}

// The batched post-training and rank of a model whose step is a 1-vs-all softmax over
// q = lhs o rel (product policy Prod): planning (kp_cx_plan.hpp), workspaces, attention
// planning and timing are the model's only through Prod, and the precision's
// (kp_posttrain_rank_f64: rq.f64) only through cx_run's row type.
// KP_HOST_TIMES=1 (kp_posttrain.hpp) prints the host time before the first upload (checks
// and planning), up to the last launch enqueued, and waiting for the device
template <class Prod>
void posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq) {
  const std::string who = kp_model_name(c->model);
  const double t_in = g_host_times ? host_ms() : 0.0;
  const int ns = bt->n_slots;
  KP_REQUIRE(hp->batch_size > 0 && hp->epochs >= 0, who + ": bad batch_size/epochs");
  // every id is checked before it indexes a host vector or a device table, as in every
  // model family (kp_batch_check.hpp)
  require_request(c, hp, bt, rq, true, kp_model_name(c->model));
  KP_REQUIRE(hp->reg_kind == KP_REG_N3 || hp->reg_kind == KP_REG_N2, who + ": unknown regulariser");

  // an armed call (kp_ctx_arm_keyed): the step plan is host work, so the permutations of the
  // multi-step slots (R > batch_size; none in most batches) are generated on the device and
  // brought back for it; the rows are generated in place by cx_workspaces
  kp_batch keyed_bt;
  std::vector<int64_t> keyed_off;
  std::vector<int32_t> keyed_perm;
  if (rq.keyed) {
    keyed_off.resize((size_t)ns + 1);
    (void)kp_keyed_words_host(c->model, hp, ns, bt->row_off, nullptr, keyed_off.data());  // require_request checked it
    const int64_t total = keyed_off[ns];
    keyed_perm.resize((size_t)std::max<int64_t>(1, total));
    if (total > 0) {
      int32_t* dPerm = ensure_n<int32_t>(c->kd.rng, (size_t)total);
      keyed_rng_dev(c, hp, rq.keyed, ns, bt->row_off, keyed_off.data(), dPerm);
      KP_HIP(hipMemcpyAsync(keyed_perm.data(), dPerm, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
      KP_HIP(hipStreamSynchronize(c->stream));
    }
    keyed_bt = *bt;
    keyed_bt.rng_off = keyed_off.data();
    keyed_bt.rng = keyed_perm.data();
    bt = &keyed_bt;
  }

  CxStepPlan sp;
  if (const char* why = cx_step_plan(c->n_ent, c->n_rel2, hp->batch_size, hp->epochs, bt, sp))
    throw KpError{KP_EINVAL, who + ": " + why};
  const double t_plan = g_host_times ? host_ms() : 0.0;
  if (rq.f64)
    cx_run<Prod, double>(c, hp, bt, rq, sp, t_in, t_plan);
  else
    cx_run<Prod, float>(c, hp, bt, rq, sp, t_in, t_plan);
}


}  // namespace

int cx_pick_db(int dim) {
  static const int dbs[] = {1, 2, 4, 8, 13, 16, 25};
  for (int db : dbs)
    if (16 * db >= dim) return db;
  return -1;
}

void complex_posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq) {
  posttrain_rank<CxProd>(c, hp, bt, rq);
}
void distmult_posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq) {
  posttrain_rank<DmProd>(c, hp, bt, rq);
}

// scores of (head, relation) pairs against every entity; ComplEx and DistMult contexts
void complex_scores_dev(kp_ctx* c, int n, const int32_t* dh, const int32_t* dr, float* dS, int ld) {
  if (n <= 0) return;
  const int DP = c->dp;
  float* dQ = ensure_n<float>(c->cx.score_q, (size_t)n * DP);
  if (c->model == KP_MODEL_DISTMULT)
    hipLaunchKernelGGL(kp_cx_scoreq<DmProd>, dim3(n), dim3(128), 0, c->stream, c->dE, c->dR, DP,
                       DmProd::extent(c->dim), dh, dr, n, dQ);
  else
    hipLaunchKernelGGL(kp_cx_scoreq<CxProd>, dim3(n), dim3(128), 0, c->stream, c->dE, c->dR, DP,
                       CxProd::extent(c->dim), dh, dr, n, dQ);
  KP_HIP(hipGetLastError());
  launch_score_gemm(c, dQ, n, dS, ld, 0);
}

void complex_all_scores(kp_ctx* c, int n, const int32_t* heads, const int32_t* rels, float* out) {
  if (n <= 0) return;
  // the pairs go through the rank's two id buffers (idle outside complex_posttrain_rank)
  // rather than two of their own, which keeps the context's device allocations as they were
  int32_t* dh = upload(c, c->rank.slots.trip, heads, (size_t)n);
  int32_t* dr = upload(c, c->rank.slots.po, rels, (size_t)n);
  float* dS = ensure_n<float>(c->cx.score_out, (size_t)n * c->n_ent);
  complex_scores_dev(c, n, dh, dr, dS, c->n_ent);
  KP_HIP(hipMemcpyAsync(out, dS, sizeof(float) * (size_t)n * c->n_ent, hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipStreamSynchronize(c->stream));
}

#ifdef KP_ATTN_STAMPS
extern "C" int kp_debug_attn_stamps(unsigned long long* out, int reset) {
  KP_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(kpattn::g_attn_stamps), sizeof(unsigned long long) * 8));
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    KP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(kpattn::g_attn_stamps), z, sizeof(z)));
  }
  return 0;
}
#endif
