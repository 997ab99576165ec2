// kp_conve.hip -- ConvE batched post-training (KelpieConvE + KelpieBCEOptimizer)
// and ranking, for gfx950.
//
// Reference semantics (src/link_prediction/models/conve.py:133-158,193-237,
// src/link_prediction/optimization/bce_optimizer.py:92-112,161-208):
//   rows = kelpie triples + inverses -> er_vocab (h, r) -> tails, insertion
//   order, NOT shuffled; minibatches of batch_size pairs; targets one-hot over
//   N = |E|+1 entities, smoothed (1-ls) y + 1/N; BCELoss(sigmoid(x . E_all^T));
//   encoder: BN1 -> input dropout -> conv 3x3 (32) -> BN2 -> ReLU -> feature-map
//   Dropout2d -> FC -> hidden dropout -> BN3 -> ReLU, with every layer frozen and BN in
//   eval mode, but the three dropouts in TRAIN mode (model.py:114-125): their masks are
//   drawn on the host (RNG as input, packed keep bits: per slot and step one word-aligned
//   run per dropout, in the forward's draw order); Adam(lr = 1e-3) on the kelpie row.
//   With an input or feature-map dropout the frozen-head pairs' encodings change every
//   step, so they are encoded per step with the kelpie pairs (else once per batch).
//
// Per step, for the pairs whose head is the kelpie ("kelpie pairs"):
//   conv forward (kp_cv_conv_fwd) -> FC (fp32 MFMA GEMM, split-K) -> dropout/BN3/ReLU
//   (kp_cv_post_fc) -> O = sum_e G(x . E_e) E_e over the frozen entities
//   (kpattn::kp_attn<.., ATT_BCE_O>, the same MFMA pass as ComplEx) -> target and
//   kelpie-column corrections and the encoder backward (kp_cv_dx, FC^T GEMM,
//   kp_cv_conv_bwd) -> kp_cv_update (+ the kelpie-column gradient of every pair;
//   pairs with a frozen head reuse their precomputed FC output) -> Adam.
#include <cstdio>
#include <cmath>

#include "kp_attn.hpp"
#include "kp_attn3.hpp"
#include "kp_cv_fused.hpp"
#include "kp_cv_plan.hpp"
#include "kp_posttrain.hpp"

int cx_pick_db(int dim);

namespace {
using namespace kpattn;

struct CvConst {
  int n_ent, dim, dp, H, hid;
  float scale;  // hidden dropout: 1/(1-p) as float32 (the noise value of a kept element)
  float ylo, yhi;
  int has_mask;             // hidden dropout drawn
  int has_in, has_fm;       // input / feature-map dropout drawn
  float scale_in, scale_fm;
  int fr_step;              // frozen-head pairs encoded every step (has_in || has_fm)
};

__device__ __forceinline__ float bce_g(float s, float y, float gs) {
  // BCELoss backward (grad = gs) followed by sigmoid backward, torch op order
#if KP_CV_EXACT_BCE & 1
  const float p = 1.0f / (1.0f + expf(-s));
#else
  const float p = 1.0f / (1.0f + __expf(-s));
#endif
  const float w = (1.0f - p) * p;
#if KP_CV_EXACT_BCE & 2
  if (w >= 1e-12f) return (p - y) * gs;
#endif
  return ((p - y) / fmaxf(w, 1e-12f) * gs) * w;
}

// the dropout multiplier of element idx of a pair's run starting at bit base (ATen's
// noise: bernoulli(keep) / keep, i.e. 1/(1-p) or 0); 1 when that dropout is not drawn
__device__ __forceinline__ float noise_at(const int32_t* __restrict__ bits, long long base, int idx, float scale) {
  if (base < 0) return 1.0f;
  const long long b = base + idx;
  const uint32_t w = (uint32_t)bits[b >> 5];
  return ((w >> (b & 31)) & 1u) ? scale : 0.0f;
}

// image (BN1) -> conv 3x3 + bias -> BN2 -> ReLU -> flat (conve.py:134-146).
// src[i] = (lhs, rel): lhs >= 0 a frozen entity row, lhs < 0 the kelpie row X[-lhs-1].
// W2C > 0: the feature-map width H - 2 as a compile-time constant (d = 200: 8), so the
// per-output index divisions become multiplies; 0: read from k.H
template <int W2C>
__global__ __launch_bounds__(256) void kp_cv_conv_fwd(int M, const int2* __restrict__ src,
                                                      const float* __restrict__ E, const float* __restrict__ X,
                                                      const float* __restrict__ R, CvConst k,
                                                      const float* __restrict__ cw, const float* __restrict__ cb,
                                                      const float* __restrict__ bna, const float* __restrict__ bnb,
                                                      const CvBits* __restrict__ mb, const int32_t* __restrict__ bits,
                                                      float* __restrict__ flat) {
  __shared__ float img[40 * 32];
  __shared__ float w[288], bias[32], a2[32], b2[32];
  const int i = blockIdx.x;
  if (i >= M) return;
  const int tid = threadIdx.x;
  const int2 sr = src[i];
  const float* lhs = sr.x >= 0 ? E + (size_t)sr.x * k.dp : X + (size_t)(-sr.x - 1) * k.dp;
  const float* rel = R + (size_t)sr.y * k.dp;
  const float a1 = bna[0], b1 = bnb[0];
  const long long in_b = mb ? mb[i].in : -1, fm_b = mb ? mb[i].fm : -1;
  for (int j = tid; j < 20 * k.H; j += 256) {
    img[j] = lhs[j] * a1 + b1;
    img[20 * k.H + j] = rel[j] * a1 + b1;
    if (in_b >= 0) {  // input dropout on the BN1 image (conve.py:141-142)
      img[j] *= noise_at(bits, in_b, j, k.scale_in);
      img[20 * k.H + j] *= noise_at(bits, in_b, 20 * k.H + j, k.scale_in);
    }
  }
  for (int j = tid; j < 288; j += 256) w[j] = cw[j];
  if (tid < 32) {
    bias[tid] = cb[tid];
    a2[tid] = bna[1 + tid];
    b2[tid] = bnb[1 + tid];
  }
  __syncthreads();
  const int W2 = W2C > 0 ? W2C : k.H - 2;
  const int per_c = 38 * W2;
  for (int o = tid; o < k.hid; o += 256) {
    const int c = o / per_c, rem = o - c * per_c;
    const int y = rem / W2, xx = rem - y * W2;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) acc += w[c * 9 + ky * 3 + kx] * img[(y + ky) * k.H + xx + kx];
    acc += bias[c];
    const float v = acc * a2[c] + b2[c];
    float f = fmaxf(v, 0.f);
    if (fm_b >= 0) f *= noise_at(bits, fm_b, c, k.scale_fm);  // feature-map Dropout2d (conve.py:147)
    flat[(size_t)i * k.hid + o] = f;
  }
}

// x = ReLU(BN3(dropout(FC))) from the split-K FC slabs; writes dp-padded rows
__global__ void kp_cv_post_fc(int M, const float* __restrict__ slabs, int ksplit, CvConst k,
                              const CvBits* __restrict__ mb, const int32_t* __restrict__ bits,
                              const float* __restrict__ bna, const float* __restrict__ bnb, float* __restrict__ Q) {
  const int i = blockIdx.x;
  if (i >= M) return;
  const float* a3 = bna + 33;
  const float* b3 = bnb + 33;
  for (int d = threadIdx.x; d < k.dp; d += blockDim.x) {
    float v = 0.f;
    if (d < k.dim) {
      float fc = 0.f;
      for (int z = 0; z < ksplit; ++z) fc += slabs[((size_t)z * M + i) * k.dim + d];
      float nz = 1.0f;
      if (mb && k.has_mask) nz = noise_at(bits, mb[i].hid, d, k.scale);
      const float dr = (mb && k.has_mask) ? fc * nz : fc;
      v = fmaxf(dr * a3[d] + b3[d], 0.f);
    }
    Q[(size_t)i * k.dp + d] = v;
  }
}

// the shared-encoder path (kp_cv_fused.hpp): fc_i = (the kelpie row's band slabs, FC bias
// in band 0) + (the pair's map-row-18-19 slabs) + trel[relation], then as kp_cv_post_fc
__global__ void kp_cv_post_fc3(int M, const float* __restrict__ sl, int nzl, int nl, const float* __restrict__ sm,
                               int nzm, const float* __restrict__ trel, const int2* __restrict__ src,
                               const int2* __restrict__ psr, CvConst k, const CvBits* __restrict__ mb,
                               const int32_t* __restrict__ bits, const float* __restrict__ bna,
                               const float* __restrict__ bnb, float* __restrict__ Q) {
  const int i = blockIdx.x;
  if (i >= M) return;
  const int kr = psr[i].x, rel = src[i].y;
  const float* a3 = bna + 33;
  const float* b3 = bnb + 33;
  for (int d = threadIdx.x; d < k.dp; d += blockDim.x) {
    float v = 0.f;
    if (d < k.dim) {
      float fl = 0.f, fm = 0.f;
      for (int z = 0; z < nzl; ++z) fl += sl[((size_t)z * nl + kr) * k.dim + d];
      for (int z = 0; z < nzm; ++z) fm += sm[((size_t)z * M + i) * k.dim + d];
      const float fc = (fl + fm) + trel[(size_t)rel * k.dim + d];
      float nz = 1.0f;
      if (mb && k.has_mask) nz = noise_at(bits, mb[i].hid, d, k.scale);
      const float dr = (mb && k.has_mask) ? fc * nz : fc;
      v = fmaxf(dr * a3[d] + b3[d], 0.f);
    }
    Q[(size_t)i * k.dp + d] = v;
  }
}

// block-wide sum (256 threads)
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// kp_cv_dx's dot products in its summation order: a 256-thread block_sum of per-thread
// partials over d = tid + 256 m, i.e. four wave sums (old wave w: d mod 256 in [64 w,
// 64 w + 64)) added in wave order.  One wave holding d = l + 64 j (lane l) keeps one
// partial per j mod 4 -- partial w is old wave w's lane l, accumulated in the same m
// order -- and adds the four wave sums in old-wave order: bitwise the block's result,
// with no LDS.
template <int NJ>
__device__ __forceinline__ float dot256_order1(const float* a, const float* b) {
  float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NJ; ++j) p[j & 3] += a[j] * b[j];
  return ((wave_sum(p[0]) + wave_sum(p[1])) + wave_sum(p[2])) + wave_sum(p[3]);
}

// kp_cv_dx on one wave per pair (NJ = ceil(dp / 64) row values per lane, in registers),
// bitwise the same as the 256-thread form below.  No LDS and <= 32 VGPRs, so it runs beside
// the other batch's attention workgroups: two kp_attn3<13> workgroups (asm form, 80 KiB
// each) fill a CU's LDS, and the round-5 two-wave form's 16 bytes of LDS then kept it off
// every CU they held (354 us per launch against 65 us, profiles/r06/r06y)
template <int NJ>
__global__ __launch_bounds__(64) void kp_cv_dx1(int M, CvConst k, const CvInst* __restrict__ inst,
                                                const float* __restrict__ Q, const float* __restrict__ O, int n_split,
                                                const int32_t* __restrict__ tails, const float* __restrict__ E,
                                                const float* __restrict__ X, const int32_t* __restrict__ bits,
                                                const float* __restrict__ bna, float* __restrict__ dfc,
                                                float* __restrict__ gk, __bf16* __restrict__ g3) {
  const int i = blockIdx.x;
  if (i >= M) return;
  const int t = threadIdx.x;
  const CvInst I = inst[i];
  float xi[NJ], xk[NJ], dx[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int d = t + 64 * j;
    const bool in = d < k.dim;
    xi[j] = in ? Q[(size_t)i * k.dp + d] : 0.f;
    xk[j] = in ? X[(size_t)I.slot * k.dp + d] : 0.f;
  }
  const float gs = 1.0f / (float)((long long)I.b * (long long)(k.n_ent + 1));
  const float sk = dot256_order1<NJ>(xi, xk);  // kelpie column
  bool k_is_tail = false;
  for (int u = 0; u < I.tail_count; ++u) k_is_tail |= (tails[I.tail_begin + u] == k.n_ent);
  const float Gk = bce_g(sk, k_is_tail ? k.yhi : k.ylo, gs);
  if (t == 0) gk[i] = Gk;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int d = t + 64 * j;
    float v = 0.f;
    if (d < k.dim)
      for (int sp = 0; sp < n_split; ++sp) v += O[((size_t)sp * M + i) * k.dp + d];
    dx[j] = v + Gk * xk[j];
  }
  // target corrections: G(s, yhi) - G(s, ylo) for the frozen tails
  for (int u = 0; u < I.tail_count; ++u) {
    const int e = tails[I.tail_begin + u];
    if (e == k.n_ent) continue;
    float er[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int d = t + 64 * j;
      er[j] = d < k.dim ? E[(size_t)e * k.dp + d] : 0.f;
    }
    const float st = dot256_order1<NJ>(xi, er);
    const float corr = bce_g(st, k.yhi, gs) - bce_g(st, k.ylo, gs);
#pragma unroll
    for (int j = 0; j < NJ; ++j) dx[j] += corr * er[j];
  }
  const float* a3 = bna + 33;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int d = t + 64 * j;
    if (d < k.dim) {
      const float nz = k.has_mask ? noise_at(bits, I.mb.hid, d, k.scale) : 1.0f;
      const float relu = xi[j] > 0.f ? 1.0f : 0.0f;
      const float v = dx[j] * relu * a3[d] * nz;
      dfc[(size_t)i * k.dim + d] = v;
      if (g3) {  // kp_cv_bwd_fused's A operand: [3][M][KB] bf16 pieces
        __bf16 h, m, l;
        split3(v, h, m, l);
        const size_t o = (size_t)i * kpcvf::KB + d, ps = (size_t)M * kpcvf::KB;
        g3[o] = h;
        g3[ps + o] = m;
        g3[2 * ps + o] = l;
      }
    }
  }
  if (g3)
    for (int d = k.dim + t; d < kpcvf::KB; d += 64) {
      const size_t o = (size_t)i * kpcvf::KB + d, ps = (size_t)M * kpcvf::KB;
      g3[o] = g3[ps + o] = g3[2 * ps + o] = (__bf16)0.f;
    }
}

// dL/dx_i (encoder output) -> dL/dfc_i; also G at the kelpie column
__global__ __launch_bounds__(256) void kp_cv_dx(int M, CvConst k, const CvInst* __restrict__ inst,
                                                const float* __restrict__ Q, const float* __restrict__ O, int n_split,
                                                const int32_t* __restrict__ tails, const float* __restrict__ E,
                                                const float* __restrict__ X, const int32_t* __restrict__ bits,
                                                const float* __restrict__ bna, float* __restrict__ dfc,
                                                float* __restrict__ gk, __bf16* __restrict__ g3) {
  __shared__ float red[4];
  __shared__ float xi[640], xk[640];
  const int i = blockIdx.x;
  if (i >= M) return;
  const int tid = threadIdx.x;
  const CvInst I = inst[i];
  for (int d = tid; d < k.dp; d += 256) {
    xi[d] = Q[(size_t)i * k.dp + d];
    xk[d] = X[(size_t)I.slot * k.dp + d];
  }
  __syncthreads();
  const float gs = 1.0f / (float)((long long)I.b * (long long)(k.n_ent + 1));
  // kelpie column
  float part = 0.f;
  for (int d = tid; d < k.dim; d += 256) part += xi[d] * xk[d];
  const float sk = block_sum(part, red);
  bool k_is_tail = false;
  for (int t = 0; t < I.tail_count; ++t) k_is_tail |= (tails[I.tail_begin + t] == k.n_ent);
  const float Gk = bce_g(sk, k_is_tail ? k.yhi : k.ylo, gs);
  if (tid == 0) gk[i] = Gk;
  const float* a3 = bna + 33;
  for (int d0 = 0; d0 < k.dim; d0 += 256) {
    const int d = d0 + tid;
    float dx = 0.f;
    if (d < k.dim) {
      for (int sp = 0; sp < n_split; ++sp) dx += O[((size_t)sp * M + i) * k.dp + d];
      dx += Gk * xk[d];
    }
    // target corrections: G(s, yhi) - G(s, ylo) for the frozen tails
    for (int t = 0; t < I.tail_count; ++t) {
      const int e = tails[I.tail_begin + t];
      if (e == k.n_ent) continue;
      float pp = 0.f;
      for (int dd = tid; dd < k.dim; dd += 256) pp += xi[dd] * E[(size_t)e * k.dp + dd];
      const float st = block_sum(pp, red);
      const float corr = bce_g(st, k.yhi, gs) - bce_g(st, k.ylo, gs);
      if (d < k.dim) dx += corr * E[(size_t)e * k.dp + d];
    }
    if (d < k.dim) {
      const float nz = k.has_mask ? noise_at(bits, I.mb.hid, d, k.scale) : 1.0f;
      const float relu = xi[d] > 0.f ? 1.0f : 0.0f;
      const float v = dx * relu * a3[d] * nz;
      dfc[(size_t)i * k.dim + d] = v;
      if (g3) {  // kp_cv_bwd_fused's A operand: [3][M][KB] bf16 pieces
        __bf16 h, m, l;
        split3(v, h, m, l);
        const size_t o = (size_t)i * kpcvf::KB + d, ps = (size_t)M * kpcvf::KB;
        g3[o] = h;
        g3[ps + o] = m;
        g3[2 * ps + o] = l;
      }
    }
  }
  if (g3)
    for (int d = k.dim + tid; d < kpcvf::KB; d += 256) {
      const size_t o = (size_t)i * kpcvf::KB + d, ps = (size_t)M * kpcvf::KB;
      g3[o] = g3[ps + o] = g3[2 * ps + o] = (__bf16)0.f;
    }
}

// dL/dflat -> ReLU / BN2 -> transposed 3x3 conv -> BN1 -> the lhs half of the image
// (feature-map dropout: flat holds the dropped map, so flat > 0 is the ReLU mask of a
// kept channel, and a kept channel's gradient carries its 1/(1-p); input dropout: the
// image gradient times the input mask)
__global__ __launch_bounds__(256) void kp_cv_conv_bwd(int M, CvConst k, const float* __restrict__ dflat,
                                                      const float* __restrict__ flat,
                                                      const float* __restrict__ cw, const float* __restrict__ bna,
                                                      const CvBits* __restrict__ mb,
                                                      const int32_t* __restrict__ bits, float* __restrict__ dl) {
  extern __shared__ __attribute__((aligned(16))) float dc[];  // [32][20][W2]
  __shared__ float w[288];
  const int i = blockIdx.x;
  if (i >= M) return;
  const int tid = threadIdx.x;
  const int W2 = k.H - 2;
  const int per_c = 38 * W2;
  for (int j = tid; j < 288; j += 256) w[j] = cw[j];
  for (int j = tid; j < 32 * 20 * W2; j += 256) {
    const int c = j / (20 * W2), rem = j - c * 20 * W2;
    const int o = c * per_c + rem;  // rows 0..19 of channel c
    const float f = flat[(size_t)i * k.hid + o];
    const float g = dflat[(size_t)i * k.hid + o];
    dc[j] = (f > 0.f) ? (k.has_fm ? g * k.scale_fm : g) * bna[1 + c] : 0.f;
  }
  __syncthreads();
  const float a1 = bna[0];
  for (int j = tid; j < 20 * k.H; j += 256) {
    const int yy = j / k.H, xx = j - yy * k.H;
    float acc = 0.f;
    for (int c = 0; c < 32; ++c) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int y = yy - ky;
        if (y < 0 || y >= 20) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int x = xx - kx;
          if (x < 0 || x >= W2) continue;
          acc += dc[(c * 20 + y) * W2 + x] * w[c * 9 + ky * 3 + kx];
        }
      }
    }
    if (k.has_in) acc *= noise_at(bits, mb[i].in, j, k.scale_in);
    dl[(size_t)i * k.dp + j] = acc * a1;
  }
}

// kp_cv_conv_fwd with the width specialised for d = 200 (H = 10)
#define KP_CONV_FWD(grid, block, shm, stream, M, src, E, X, R, kk, ...)                                      \
  do {                                                                                                      \
    if ((kk).H == 10)                                                                                       \
      hipLaunchKernelGGL(kp_cv_conv_fwd<8>, grid, block, shm, stream, M, src, E, X, R, kk, __VA_ARGS__);    \
    else                                                                                                    \
      hipLaunchKernelGGL(kp_cv_conv_fwd<0>, grid, block, shm, stream, M, src, E, X, R, kk, __VA_ARGS__);    \
  } while (0)

struct CvOpt {
  float lr, b1, b2, eps, one_minus_b1, one_minus_b2, step_size, bc2_sqrt;
};

// the frozen-head pairs' part of a slot's gradient (o, r_inv, kelpie): the kelpie
// column's BCE gradient G * x_fc, in chunks of up to FCH pairs of one slot, one workgroup per
// chunk (a hub slot's hundreds of pairs no longer run as one workgroup's serial loop);
// ch = (slot's act index in the step, first pair, pair count); fpart[chunk][d]
__global__ __launch_bounds__(256) void kp_cv_fgrad(CvConst k, const int4* __restrict__ chunks,
                                                   const CvAct* __restrict__ act, const CvFInst* __restrict__ fi,
                                                   const float* __restrict__ fcf, const int32_t* __restrict__ bits,
                                                   const float* __restrict__ bna, const float* __restrict__ bnb,
                                                   const float* __restrict__ X, float* __restrict__ fpart) {
  __shared__ float xs[640];
  __shared__ float gw_s[4][640];  // per-wave partial sums
  const int4 ch = chunks[blockIdx.x];
  const CvAct A = act[ch.x];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const float* x = X + (size_t)A.slot * k.dp;
  for (int d = tid; d < k.dp; d += 256) xs[d] = x[d];
  __syncthreads();
  const float* a3 = bna + 33;
  const float* b3 = bnb + 33;
  float gw[10];
#pragma unroll
  for (int u = 0; u < 10; ++u) gw[u] = 0.f;
  auto load_pair = [&](const CvFInst& F, float (&v)[10]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 10; ++u) {
      const int d = lane + 64 * u;
      v[u] = 0.f;
      if (d < k.dim) {
        if (k.fr_step) {  // encoded this step with its own masks (kp_cv_post_fc)
          v[u] = fcf[(size_t)F.fp * k.dp + d];
        } else {
          const float fc = fcf[(size_t)F.fp * k.dim + d];
          const float nz = k.has_mask ? noise_at(bits, F.mb.hid, d, k.scale) : 1.0f;
          const float dr = k.has_mask ? fc * nz : fc;
          v[u] = fmaxf(dr * a3[d] + b3[d], 0.f);
        }
      }
    }
  };
  auto add_pair = [&](const CvFInst& F, const float (&v)[10]) __attribute__((always_inline)) {
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < 10; ++u) {
      const int d = lane + 64 * u;
      if (d < k.dim) part += v[u] * xs[d];
    }
    const float s = wave_sum(part);
    const float gs = 1.0f / (float)((long long)F.b * (long long)(k.n_ent + 1));
    const float G = bce_g(s, k.yhi, gs);
#pragma unroll
    for (int u = 0; u < 10; ++u) gw[u] += G * v[u];
  };
  // a wave's pairs (wave, wave + 4, ...) two at a time: both rows loaded before either
  // reduction
  const int f0 = A.f_begin + ch.y;
  int j = wave;
  for (; j + 4 < ch.z; j += 8) {
    const CvFInst F0 = fi[f0 + j], F1 = fi[f0 + j + 4];
    float v0[10], v1[10];
    load_pair(F0, v0);
    load_pair(F1, v1);
    add_pair(F0, v0);
    add_pair(F1, v1);
  }
  if (j < ch.z) {
    const CvFInst F0 = fi[f0 + j];
    float v0[10];
    load_pair(F0, v0);
    add_pair(F0, v0);
  }
#pragma unroll
  for (int u = 0; u < 10; ++u) {
    const int d = lane + 64 * u;
    if (d < k.dim) gw_s[wave][d] = gw[u];
  }
  __syncthreads();
  for (int d = tid; d < k.dim; d += 256)
    fpart[(size_t)blockIdx.x * k.dim + d] = (gw_s[0][d] + gw_s[1][d]) + (gw_s[2][d] + gw_s[3][d]);
}

// kp_posttrain_rank_marks: per entry of the step's active list the mark row its update also
// stores (-1: none), and the mark rows [slots][marks][dp].  Without the flag the struct is
// empty and kp_cv_update is what it was.
template <bool MARKS>
struct CvMarkArgs {};
template <>
struct CvMarkArgs<true> {
  const int32_t* row;  // [active slots of the step]
  float* rows;
};

// gradient assembly + Adam, one workgroup per active slot; its frozen-head pairs' part is
// the sum of its kp_cv_fgrad chunks (A.pad0: first chunk of the step, A.pad1: count)
// MARKS: the thread that stores an updated element stores it to the slot's mark row as well
// when the plan marks this (slot, step); a plain vector store, no launch of its own
template <bool MARKS = false>
__global__ __launch_bounds__(256) void kp_cv_update(CvConst k, const CvAct* __restrict__ act,
                                                    const float* __restrict__ Q, const float* __restrict__ gk,
                                                    const float* __restrict__ dl, const float* __restrict__ fpart,
                                                    float* __restrict__ X, float* __restrict__ S1,
                                                    float* __restrict__ S2, CvOpt opt, CvMarkArgs<MARKS> mk) {
  __shared__ float xs[640];
  const CvAct A = act[blockIdx.x];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  float* x = X + (size_t)A.slot * k.dp;
  for (int d = tid; d < k.dp; d += 256) xs[d] = x[d];
  __syncthreads();
  float g[3] = {0.f, 0.f, 0.f};
  // kelpie-head pair rows: a slot with more than 4 sums them in four wave-strided
  // partials with two chains each (one chain per dimension was bound by load latency);
  // the choice is block-uniform
  __shared__ float gk_s[4][640];
  const bool wide = A.k_count > 4;
  if (wide) {
    for (int d = lane; d < k.dim; d += 64) {
      float a0 = 0.f, a1 = 0.f;
      int j = wave;
      for (; j + 4 < A.k_count; j += 8) {
        const int i0 = A.k_begin + j, i1 = i0 + 4;
        a0 += gk[i0] * Q[(size_t)i0 * k.dp + d] + dl[(size_t)i0 * k.dp + d];
        a1 += gk[i1] * Q[(size_t)i1 * k.dp + d] + dl[(size_t)i1 * k.dp + d];
      }
      if (j < A.k_count) {
        const int i0 = A.k_begin + j;
        a0 += gk[i0] * Q[(size_t)i0 * k.dp + d] + dl[(size_t)i0 * k.dp + d];
      }
      gk_s[wave][d] = a0 + a1;
    }
  } else {
    for (int j = 0; j < A.k_count; ++j) {
      const int ii = A.k_begin + j;
      const float G = gk[ii];
      for (int u = 0; u < 3; ++u) {
        const int d = tid + 256 * u;
        if (d < k.dim) g[u] += G * Q[(size_t)ii * k.dp + d] + dl[(size_t)ii * k.dp + d];
      }
    }
  }
  __syncthreads();
  for (int u = 0; u < 3; ++u) {
    const int d = tid + 256 * u;
    if (d >= k.dim) continue;
    if (wide) g[u] = (gk_s[0][d] + gk_s[1][d]) + (gk_s[2][d] + gk_s[3][d]);
    float fw = 0.f;
    for (int c = 0; c < A.pad1; ++c) fw += fpart[(size_t)(A.pad0 + c) * k.dim + d];
    g[u] += fw;
  }
  for (int u = 0; u < 3; ++u) {
    const int d = tid + 256 * u;
    if (d >= k.dim) continue;
    const size_t o = (size_t)A.slot * k.dp + d;
    float m1 = S1[o], v2 = S2[o];
    const float gd = g[u];
    m1 = m1 + opt.one_minus_b1 * (gd - m1);
    v2 = v2 * opt.b2;
    v2 = v2 + (opt.one_minus_b2 * gd) * gd;
    const float den = sqrtf(v2) / opt.bc2_sqrt + opt.eps;
    const float xd = xs[d] + (-opt.step_size * m1) / den;
    x[d] = xd;
    if constexpr (MARKS) {
      const int mrow = mk.row[blockIdx.x];  // block-uniform
      if (mrow >= 0) mk.rows[(size_t)mrow * k.dp + d] = xd;
    }
    S1[o] = m1;
    S2[o] = v2;
  }
}

// fp64 ranking queries (launch_rank_f64, act 1): the encoder output of the post-trained
// row (fp32, eval mode) widened to fp64; its logit against the target and against the
// kelpie row as one sequential fp64 FMA chain over d (exact products of fp32 operands),
// the order kp_rank_f64_count scores every entity in.  At the reference init the sigmoid
// scores of ~10^5 entities lie within ~0.005 of 0.5, a few per fp32 ulp there, so fp32
// scores tie and their rounding moves the rank; the logits order them as a fp64 run does.
// Row s of a set of rank rows is po[3 s ..] = (row, p, o) and Qr[s] its encoder output
// (encode_eval on (-row - 1, p)): x is row `row` of X (the slots: s itself; a probe: its slot's
// kelpie row; a mark row: its row of the mark workspace).
__global__ void kp_cv_rankq64(const float* __restrict__ Qr, const float* __restrict__ X,
                              const float* __restrict__ E, int n_ent, int dp, const int32_t* __restrict__ po,
                              int n_slots, double* __restrict__ Q, double* __restrict__ t64,
                              double* __restrict__ kcol64) {
  const int s = blockIdx.x;
  if (s >= n_slots) return;
  double* q = Q + (size_t)s * dp;
  for (int d = threadIdx.x; d < dp; d += blockDim.x) q[d] = (double)Qr[(size_t)s * dp + d];
  __syncthreads();
  if (threadIdx.x == 0) {
    const float* x = X + (size_t)po[3 * s] * dp;
    const int o = po[3 * s + 2];
    double z = 0.0, t = 0.0;
    for (int d = 0; d < dp; ++d) z = __fma_rn(q[d], (double)x[d], z);
    if (o < n_ent) {
      const float* eo = E + (size_t)o * dp;
      for (int d = 0; d < dp; ++d) t = __fma_rn(q[d], (double)eo[d], t);
    } else {
      t = z;  // the kelpie entity is its own object
    }
    kcol64[s] = z;
    t64[s] = t;
  }
}

// kelpie column of the rank scores: sigmoid(q_s . x_s)
__global__ void kp_cv_kcol(int n, CvConst k, const float* __restrict__ Q, const float* __restrict__ X,
                           float* __restrict__ scores, int ld) {
  const int s = blockIdx.x;
  if (s >= n) return;
  float z = 0.f;
  for (int d = threadIdx.x; d < k.dim; d += 64) z += Q[(size_t)s * k.dp + d] * X[(size_t)s * k.dp + d];
  z = wave_sum(z);
  if (threadIdx.x == 0) scores[(size_t)s * ld + k.n_ent] = 1.0f / (1.0f + expf(-z));
}

// ---- kp_posttrain_rank_trace (include/kelpie_hip.h, "Post-training trace") ----------------
// The step loop evaluates no loss: the attention forms G(s_e), and the frozen-head pairs never
// meet the frozen entities.  So the trace scores every row of a step -- the kelpie pairs and
// the frozen-head pairs, encoded with the step's masks as the step encodes them -- against all
// n_ent + 1 columns (one fp32 MFMA pass over E per chunk of rows, kp_gemm_abt) and reduces
// the BCE terms in fp64.

// the step's rows [nk + nf][dp]: the kelpie pairs' encoder outputs (copied from Q), then the
// frozen-head pairs' rows from their batch-wide FC rows with this step's hidden mask, as
// kp_cv_fgrad forms them (with an input or feature-map dropout Q holds them all already)
__global__ void kp_cv_trace_rows(int nk, int nf, CvConst k, const float* __restrict__ Q,
                                 const CvFInst* __restrict__ fi, const float* __restrict__ fcf,
                                 const int32_t* __restrict__ bits, const float* __restrict__ bna,
                                 const float* __restrict__ bnb, float* __restrict__ TQ) {
  const int i = blockIdx.x;
  if (i >= nk + nf) return;
  float* out = TQ + (size_t)i * k.dp;
  if (i < nk) {
    for (int d = threadIdx.x; d < k.dp; d += blockDim.x) out[d] = Q[(size_t)i * k.dp + d];
    return;
  }
  const CvFInst F = fi[i - nk];
  const float* a3 = bna + 33;
  const float* b3 = bnb + 33;
  for (int d = threadIdx.x; d < k.dp; d += blockDim.x) {
    float v = 0.f;
    if (d < k.dim) {
      const float fc = fcf[(size_t)F.fp * k.dim + d];
      const float nz = k.has_mask ? noise_at(bits, F.mb.hid, d, k.scale) : 1.0f;
      const float dr = k.has_mask ? fc * nz : fc;
      v = fmaxf(dr * a3[d] + b3[d], 0.f);
    }
    out[d] = v;
  }
}

// one BCELoss term on the logit s with target y, in fp64: -(y log p + (1 - y) log(1 - p)),
// p = sigmoid(s), each log clamped at -100 as torch clamps it
__device__ __forceinline__ double cv_bce_term(double s, double y) {
  const double lp = fmin(s, 0.0) - log1p(exp(-fabs(s)));  // log sigmoid(s); log(1 - sigmoid(s)) = lp - s
  return -(y * fmax(lp, -100.0) + (1.0 - y) * fmax(lp - s, -100.0));
}

// the summed BCE terms of one row over all n_ent + 1 columns; one workgroup per row of the
// chunk [r0, r0 + gridDim.x).  Every frozen column first counts with the smoothed zero target,
// thread-strided partials, a butterfly per wave and the four wave sums in wave order (a fixed
// order); then the kelpie column (its logit the row's fp64 dot with the slot's x) and the
// pair's own tails are put right
__global__ __launch_bounds__(256) void kp_cv_trace_row(int r0, int nk, CvConst k, const float* __restrict__ S, int ld,
                                                       const float* __restrict__ TQ, const CvInst* __restrict__ ki,
                                                       const CvFInst* __restrict__ fi,
                                                       const int32_t* __restrict__ tails,
                                                       const float* __restrict__ X, double* __restrict__ rowloss) {
  __shared__ double part[2][4];
  const int row = r0 + blockIdx.x, tid = threadIdx.x;
  const float* srow = S + (size_t)blockIdx.x * ld;
  const bool kelpie = row < nk;
  const int slot = kelpie ? ki[row].slot : fi[row - nk].slot;
  const float* q = TQ + (size_t)row * k.dp;
  const float* x = X + (size_t)slot * k.dp;
  const double ylo = (double)k.ylo, yhi = (double)k.yhi;
  double acc = 0.0, z = 0.0;
  for (int e = tid; e < k.n_ent; e += 256) acc += cv_bce_term((double)srow[e], ylo);
  for (int d = tid; d < k.dim; d += 256) z += (double)q[d] * (double)x[d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    z += __shfl_xor(z, o, 64);
  }
  if ((tid & 63) == 0) {
    part[0][tid >> 6] = acc;
    part[1][tid >> 6] = z;
  }
  __syncthreads();
  if (tid != 0) return;
  double total = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
  const double zk = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
  bool k_is_tail = !kelpie;  // a frozen-head pair's only tail is the kelpie entity
  if (kelpie) {
    const CvInst I = ki[row];
    for (int u = 0; u < I.tail_count; ++u) {
      const int e = tails[I.tail_begin + u];
      if (e == k.n_ent) {
        k_is_tail = true;
      } else {
        const double st = (double)srow[e];
        total += cv_bce_term(st, yhi) - cv_bce_term(st, ylo);
      }
    }
  }
  rowloss[row] = total + cv_bce_term(zk, k_is_tail ? yhi : ylo);
}

// one thread per active slot: its rows' sums in row order (kelpie pairs, then frozen-head
// pairs), the mean over b x (n_ent + 1), one fp32 rounding at the store of step `step`
__global__ void kp_cv_trace_slot(int na, int nk, CvConst k, const CvAct* __restrict__ act,
                                 const CvInst* __restrict__ ki, const CvFInst* __restrict__ fi,
                                 const double* __restrict__ rowloss, const int32_t* __restrict__ trace_off, int step,
                                 float* __restrict__ loss) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= na) return;
  const CvAct A = act[a];
  double sum = 0.0;
  for (int j = 0; j < A.k_count; ++j) sum += rowloss[A.k_begin + j];
  for (int j = 0; j < A.f_count; ++j) sum += rowloss[nk + A.f_begin + j];
  const int b = A.k_count > 0 ? ki[A.k_begin].b : fi[A.f_begin].b;
  loss[trace_off[A.slot] + step] = (float)(sum / ((double)b * (double)(k.n_ent + 1)));
}

CvConst make_const(kp_ctx* c, const kp_hp* hp) {
  CvConst k{};
  k.n_ent = c->n_ent;
  k.dim = c->dim;
  k.dp = c->dp;
  k.H = c->dim / 20;
  k.hid = c->hidden;
  // ATen's noise value: 1 / (1 - p) in float32 (the dropout's div_ of the bernoulli mask);
  // p == 1 ships zero keep bits, so its infinite scale is never selected
  auto scale_of = [](double p) { return (p > 0.0 && p < 1.0) ? (1.0f / (float)(1.0 - p)) : 1.0f; };
  const double p = hp ? hp->hidden_dropout : 0.0;
  k.has_mask = (p > 0.0) ? 1 : 0;
  k.scale = scale_of(p);
  const double pin = hp ? hp->input_dropout : 0.0, pfm = hp ? hp->fmap_dropout : 0.0;
  k.has_in = (pin > 0.0) ? 1 : 0;
  k.has_fm = (pfm > 0.0) ? 1 : 0;
  k.scale_in = scale_of(pin);
  k.scale_fm = scale_of(pfm);
  k.fr_step = (k.has_in || k.has_fm) ? 1 : 0;
  const double ls = hp ? hp->label_smoothing : 0.0;
  if (ls != 0.0) {
    const float inv_n = (float)(1.0 / (double)(c->n_ent + 1));
    k.ylo = inv_n;
    k.yhi = (float)(1.0 - ls) * 1.0f + inv_n;
  } else {
    k.ylo = 0.f;
    k.yhi = 1.f;
  }
  return k;
}

// encoder (eval mode) for n (lhs, rel) sources -> Q [n][dp]
void encode_eval(kp_ctx* c, int n, const int2* dsrc, const float* dX, float* dQ) {
  if (n <= 0) return;
  CvConst k = make_const(c, nullptr);
  float* dflat = ensure_n<float>(c->cv.flat, (size_t)n * c->hidden);
  float* dfc = ensure_n<float>(c->cv.slab, (size_t)n * c->dim);
  KP_CONV_FWD(dim3(n), dim3(256), 0, c->stream, n, dsrc, c->dE, dX, c->dR, k, c->d_conv_w,
                     c->d_conv_b, c->d_bn_a, c->d_bn_b, nullptr, nullptr, dflat);
  KP_HIP(hipGetLastError());
  launch_gemm_abt(c, dflat, c->hidden, n, c->d_fc_w, c->hidden, c->dim, c->hidden, dfc, c->dim, c->d_fc_b, 0, 1);
  hipLaunchKernelGGL(kp_cv_post_fc, dim3(n), dim3(256), 0, c->stream, n, dfc, 1, k, nullptr, nullptr, c->d_bn_a,
                     c->d_bn_b, dQ);
  KP_HIP(hipGetLastError());
}

}  // namespace

float* conve_fc_wt(kp_ctx* c);

// kp_cv_fused.hpp's weight images (built once per context; the FC layer is frozen)
static void conve_fused_images(kp_ctx* c, const __bf16** fw, const __bf16** bw) {
  if (!c->cvf_ready) {
    const long long n1 = (long long)kpcvf::NR * kpcvf::HID, n2 = (long long)kpcvf::NBL * kpcvf::KB;
    __bf16* a = reinterpret_cast<__bf16*>(c->cvf_fw3.ensure(3 * sizeof(__bf16) * (size_t)n1));
    __bf16* b = reinterpret_cast<__bf16*>(c->cvf_bw3.ensure(3 * sizeof(__bf16) * (size_t)n2));
    hipLaunchKernelGGL(kpcvf::kp_cv_fwd_image, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_fc_w, c->dim, a);
    KP_HIP(hipGetLastError());
    hipLaunchKernelGGL(kpcvf::kp_cv_bwd_image, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_fc_w, c->dim, b);
    KP_HIP(hipGetLastError());
    c->cvf_ready = true;
  }
  *fw = c->cvf_fw3.as<__bf16>();
  *bw = c->cvf_bw3.as<__bf16>();
}

// the shared-encoder split's frozen terms (kp_cv_fused.hpp), once per context: the FC
// weight's map-row slices and the relations' FC terms (map rows 20-37, the relation half
// only, no bias) summed over NB_L bands.  dX / dBits: any valid kelpie rows / keep bits,
// the relation sources read neither
static void conve_shared_setup(kp_ctx* c, const __bf16* cvf_fw, const float* dX, const int32_t* dBits) {
  if (c->cv_shared_ready) return;
  constexpr int NB_L = 24;
  float* wtm = ensure_n<float>(c->cv_wtm, (size_t)c->dim * kpcvf::NMID);
  hipLaunchKernelGGL(kpcvf::kp_cv_mid_wt, dim3((c->dim * kpcvf::NMID + 255) / 256), dim3(256), 0, c->stream,
                     c->d_fc_w, c->dim, wtm);
  KP_HIP(hipGetLastError());
  float* wtl = ensure_n<float>(c->cv_wtl, (size_t)c->dim * kpcvf::NLHS);
  float* wlc = ensure_n<float>(c->cv_wlc, (size_t)c->dim * kpcvf::NLHS);
  float* wfm = ensure_n<float>(c->cv_wfm, (size_t)c->dim * kpcvf::NMID);
  const int nw = (kpcvf::NLHS + kpcvf::NMID) * c->dim;
  hipLaunchKernelGGL(kpcvf::kp_cv_lhs_wt, dim3((nw + 255) / 256), dim3(256), 0, c->stream, c->d_fc_w, c->dim, wlc,
                     wtl, wfm);
  KP_HIP(hipGetLastError());
  const int nr = c->n_rel2;
  std::vector<int2> rs(nr);
  for (int r = 0; r < nr; ++r) rs[r] = make_int2(0, r);
  DevBuf bs, bo;
  int2* dRs = upload(c, bs, rs.data(), rs.size());
  float* sl = ensure_n<float>(bo, (size_t)NB_L * nr * c->dim);
  const int g = NB_L * ((nr + kpcvf::MT - 1) / kpcvf::MT);
  hipLaunchKernelGGL(kpcvf::kp_cv_fwd_fused<false>, dim3(g), dim3(512), kpcvf::FWD_LDS, c->stream, nr, dRs, c->dE,
                     dX, c->dR, c->dp, c->d_conv_w, c->d_conv_b, c->d_bn_a, c->d_bn_b, cvf_fw, nullptr, c->dim,
                     nullptr, dBits, 1.0f, 1.0f, sl, nullptr, 8 * (kpcvf::MID_Y + 2),
                     8 * (kpcvf::FR - kpcvf::MID_Y - 2), NB_L, 2);
  KP_HIP(hipGetLastError());
  float* tr = ensure_n<float>(c->cv_trel, (size_t)nr * c->dim);
  hipLaunchKernelGGL(kpcvf::kp_cv_slab_sum, dim3((nr * c->dim + 255) / 256), dim3(256), 0, c->stream, nr, NB_L,
                     c->dim, sl, tr);
  KP_HIP(hipGetLastError());
  KP_HIP(hipStreamSynchronize(c->stream));
  bs.release();
  bo.release();
  c->cv_shared_ready = true;
}

void conve_encode_dev(kp_ctx* c, int n, const int2* d_src, float* d_out) { encode_eval(c, n, d_src, nullptr, d_out); }

namespace {

// the plan's element types are the HIP vector types' layout: their arrays are uploaded as such
static_assert(sizeof(CvI2) == sizeof(int2) && alignof(CvI2) == alignof(int2), "CvI2 is int2");
static_assert(sizeof(CvI4) == sizeof(int4) && alignof(CvI4) == alignof(int4), "CvI4 is int4");
// a plan list on the device, at least one element long (an empty list sizes the buffer only:
// a call without a step, hp.epochs == 0 or no slot with rows, has nothing to copy)
template <class D, class T>
D* upload_list(kp_ctx* c, DevBuf& b, const std::vector<T>& v) {
  static_assert(sizeof(D) == sizeof(T), "the list's device type has the host type's layout");
  D* d = ensure_n<D>(b, std::max<size_t>(1, v.size()));
  if (!v.empty()) KP_HIP(hipMemcpyAsync(d, v.data(), sizeof(D) * v.size(), hipMemcpyHostToDevice, c->stream));
  return d;
}
template <class T>
T* upload1(kp_ctx* c, DevBuf& b, const std::vector<T>& v) {
  return upload_list<T>(c, b, v);
}
int2* upload1(kp_ctx* c, DevBuf& b, const std::vector<CvI2>& v) { return upload_list<int2>(c, b, v); }
int4* upload1(kp_ctx* c, DevBuf& b, const std::vector<CvI4>& v) { return upload_list<int4>(c, b, v); }

// the device side of one call (c->cv): the plan's uploads (cv_workspaces), the frozen-head
// pairs' FC rows (cv_frozen_fc) and the step workspaces (cv_step_workspaces)
struct CvDev {
  float *X, *S1, *S2;  // kelpie rows and Adam state [ns][dp]
  CvInst* KI;
  CvFInst* FI;
  CvAct* act;
  int32_t *tails, *bits;
  float* fcf = nullptr;  // frozen-head pairs' FC output (pre-dropout), once per batch
  bool fused = false;    // fused encoder kernels (kp_cv_fused.hpp) for d = 200: the feature map stays on chip
  bool shared = false;   // the shared-encoder split: kelpie rows' map rows 0-17, the pairs' rows 18-19
  int KS, mk, me, msr;   // FC forward split-K; kelpie pairs, encoder rows, shared rows per step (>= 1)
  float *flat, *slab, *Q;
  const __bf16 *fw = nullptr, *bw = nullptr;
  uint8_t* relu = nullptr;
  __bf16* g3 = nullptr;
  int2 *sr_src = nullptr, *sr_rng = nullptr, *psr = nullptr;
  uint8_t* relu_s = nullptr;
  float* slab_l = nullptr;  // kelpie rows' FC split-K slabs [KSL][rows][dim]
  float* mid = nullptr;     // pairs' map-row-18-19 FC terms [pairs][dim]
  float* map_l = nullptr;   // kelpie rows' map rows 0-17, then (backward) g W_lhs
  float* map_m = nullptr;   // pairs' map rows 18-19, then (backward) dfc W_mid [pairs][512]
  float* gs = nullptr;      // kelpie rows' summed pair dfc
  float* dls = nullptr;     // kelpie rows' lhs image gradient [rows][DP]
  int2* src;
  int4* fch;
  float* fpart;
  CvBits* enc_bits;
  float* gscale;
  std::vector<AttnPlan> step_plan;  // [T]
  RankSet probes;               // kp_posttrain_rank_probes
  MarksDev marks;               // kp_posttrain_rank_marks
  int32_t* mark_row = nullptr;  // [acts] the mark row an active entry's update also stores, or -1
  float *O, *dfc, *gk, *dflat, *dl, *wt;
  float s_in, s_fm;  // the masks' multipliers as the fused kernels take them (1: not drawn)
};

CvDev cv_workspaces(kp_ctx* c, const kp_batch* bt, const CvStepPlan& sp, std::vector<float>& xp) {
  CvDev d;
  d.X = upload_x0(c, c->cv.x, bt, xp);
  d.S1 = ensure_n<float>(c->cv.s1, xp.size());
  d.S2 = ensure_n<float>(c->cv.s2, xp.size());
  KP_HIP(hipMemsetAsync(d.S1, 0, sizeof(float) * xp.size(), c->stream));
  KP_HIP(hipMemsetAsync(d.S2, 0, sizeof(float) * xp.size(), c->stream));
  d.KI = upload1(c, c->cv.kinst, sp.kinst);
  d.FI = upload1(c, c->cv.finst, sp.finst);
  d.act = upload1(c, c->cv.acts, sp.acts);
  d.tails = upload1(c, c->cv.tails, sp.tails);
  const int64_t nbits = bt->rng_off[bt->n_slots];
  // the keep bits, plus one zero guard word (kp_cv_fwd_fused reads a row's input bits as
  // a 64-bit window)
  d.bits = ensure_n<int32_t>(c->cv.keep_bits, (size_t)(nbits + 2));
  if (nbits > 0)
    KP_HIP(hipMemcpyAsync(d.bits, bt->rng, sizeof(int32_t) * (size_t)nbits, hipMemcpyHostToDevice, c->stream));
  KP_HIP(hipMemsetAsync(d.bits + nbits, 0, 2 * sizeof(int32_t), c->stream));
  return d;
}

// frozen-head pairs without an input / feature-map dropout: FC output (pre-dropout) once
// per batch.  Returns the rows it encoded
int cv_frozen_fc(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, CvDev& d) {
  const int nfp = kc.fr_step ? 0 : (int)sp.fpairs.size();
  d.fcf = ensure_n<float>(c->cv.fcf, (size_t)std::max(1, nfp) * c->dim);
  if (nfp > 0) {
    int2* dFp = upload(c, c->cv.fpairs, reinterpret_cast<const int2*>(sp.fpairs.data()), sp.fpairs.size());
    float* dflat = ensure_n<float>(c->cv.flat, (size_t)nfp * c->hidden);
    KP_CONV_FWD(dim3(nfp), dim3(256), 0, c->stream, nfp, dFp, c->dE, d.X, c->dR, kc, c->d_conv_w, c->d_conv_b,
                c->d_bn_a, c->d_bn_b, nullptr, nullptr, dflat);
    KP_HIP(hipGetLastError());
    launch_gemm_abt(c, dflat, c->hidden, nfp, c->d_fc_w, c->hidden, c->dim, c->hidden, d.fcf, c->dim, c->d_fc_b, 0, 1);
  }
  return nfp;
}

// the attention plan of every step and its O rows
void cv_attn_plans(kp_ctx* c, const CvStepPlan& sp, CvDev& d) {
  const int DBV = c->dp / 16;
  int attn_slots = c->n_cu * (DBV <= 13 ? 2 : 1);  // co-resident attention workgroups
  if (c->attn_mode == 1) {
    KP_DB_DISPATCH(DBV, 4, "ConvE: unsupported padded dimension",
                   attn_slots = c->n_cu * attn3_wpc<DB, ATT_BCE_O>(c));
  }
  d.step_plan.resize(sp.T);
  size_t o_rows = 1;
  c->attn_last = {};
  for (int t = 0; t < sp.T; ++t) {
    const int nk = sp.kin_off[t + 1] - sp.kin_off[t];
    // the ConvE attention (ATT_BCE_O, two workgroups per CU) keeps the plan of a launch that
    // runs alone whatever the context's in-flight hint says
    d.step_plan[t] = attn_plan_ctx(c, std::max(nk, 1), c->n_ent, attn_slots, KP_CV_ATTN_INFLIGHT != 0);
    if (nk > 0) attn_plan_note(c, d.step_plan[t], nk, KP_CV_ATTN_INFLIGHT != 0);
    o_rows = std::max(o_rows, (size_t)nk * d.step_plan[t].wk.n_parts);
  }
  d.O = ensure_n<float>(c->cv.o, o_rows * c->dp);
}

// the step loop's workspaces and the rest of the plan's uploads; nfp: cv_frozen_fc's rows
// (c->cv.flat still holds them)
void cv_step_workspaces(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, int nfp, CvDev& d) {
  const int DP = c->dp, K = c->n_ent;
  d.fused = c->cv_fused && c->dim == 200 && c->hidden == kpcvf::HID;
  d.KS = d.fused ? kpcvf::NSPLIT : 8;
  d.mk = std::max(1, sp.max_k);
  d.me = std::max(1, sp.max_enc);  // encoder rows per step (kelpie pairs + per-step frozen pairs)
  d.msr = std::max(1, sp.max_sr);
  const int mk = d.mk, me = d.me, msr = d.msr;
  d.flat = ensure_n<float>(c->cv.flat, (size_t)std::max(d.fused ? 1 : me, nfp) * c->hidden);
  d.slab = ensure_n<float>(c->cv.slab, (size_t)d.KS * me * c->dim);
  if (d.fused) {
    conve_fused_images(c, &d.fw, &d.bw);
    d.relu = reinterpret_cast<uint8_t*>(c->cv.relu.ensure((size_t)me * kpcvf::MASK_B));
    d.g3 = ensure_n<__bf16>(c->cv.g3, 3 * (size_t)mk * kpcvf::KB);
  }
  // the shared-encoder split (kp_cv_fused.hpp): kelpie rows' map rows 0-17 in NB_L bands,
  // the pairs' rows 18-19 in NB_M, the relations' rows 20-37 (once per context) in NB_L
  d.shared = d.fused && c->cv_shared && !kc.has_in && !kc.has_fm;
  if (d.shared) {
    conve_shared_setup(c, d.fw, d.X, d.bits);
    d.sr_src = upload1(c, c->cv.sr_src, sp.sr_src);
    d.sr_rng = upload1(c, c->cv.sr_rng, sp.sr_rng);
    d.psr = upload1(c, c->cv.psr, sp.psr);
    d.relu_s = reinterpret_cast<uint8_t*>(c->cv.relu_s.ensure((size_t)msr * kpcvf::MASK_B));
    KP_HIP(hipMemsetAsync(d.relu_s, 0, (size_t)msr * kpcvf::MASK_B, c->stream));  // rows 18-19 stay 0
    d.slab_l = ensure_n<float>(c->cv.slab_l, (size_t)kpcvf::KSL * msr * c->dim);
    d.map_m = ensure_n<float>(c->cv.map_m, (size_t)mk * kpcvf::NMID);
    d.mid = ensure_n<float>(c->cv.mid, (size_t)mk * c->dim);
    d.map_l = ensure_n<float>(c->cv.map_l, (size_t)msr * kpcvf::NLHS);
    d.gs = ensure_n<float>(c->cv.gs, (size_t)msr * c->dim);
    d.dls = ensure_n<float>(c->cv.dls, (size_t)msr * DP);
  }
  const int n_dl = d.fused ? kpcvf::NSPLIT : 1;  // lhs image-gradient slabs per pair (kp_cv_bwd_fused, reduced in slab 0)
  d.Q = ensure_n<float>(c->cv.q, (size_t)me * DP);
  d.src = upload1(c, c->cv.enc_src, sp.enc_src);
  d.fch = upload1(c, c->cv.fchunks, sp.fchunks);
  d.fpart = ensure_n<float>(c->cv.fpart, (size_t)std::max(1, sp.max_fch) * c->dim);
  d.enc_bits = upload1(c, c->cv.enc_bits, sp.enc_bits);
  d.gscale = ensure_n<float>(c->cv.gscale, std::max<size_t>(1, sp.kinst.size()));
  {
    std::vector<float> gsv(sp.kinst.size());
    for (size_t i = 0; i < gsv.size(); ++i) gsv[i] = 1.0f / (float)((long long)sp.kinst[i].b * (long long)(K + 1));
    if (!gsv.empty())
      KP_HIP(hipMemcpyAsync(d.gscale, gsv.data(), sizeof(float) * gsv.size(), hipMemcpyHostToDevice, c->stream));
  }
  cv_attn_plans(c, sp, d);
  d.dfc = ensure_n<float>(c->cv.dfc, (size_t)mk * c->dim);
  d.gk = ensure_n<float>(c->cv.gk, (size_t)mk);
  d.dflat = ensure_n<float>(c->cv.dflat, (size_t)(d.fused ? 1 : mk) * c->hidden);
  d.dl = ensure_n<float>(c->cv.dl, (size_t)n_dl * mk * DP);
  d.wt = conve_fc_wt(c);
  d.s_in = kc.has_in ? kc.scale_in : 1.0f;
  d.s_fm = kc.has_fm ? kc.scale_fm : 1.0f;
}

// step t's slices of the plan's device lists
struct CvStep {
  int t, nk, ne, na, nsr;  // kelpie pairs, encoder rows (the nk kelpie rows first), active slots, shared rows
  const CvInst* KI;
  const int2* ES;
  const CvBits* EB;
};
CvStep cv_step(const CvStepPlan& sp, const CvDev& d, int t) {
  return CvStep{t,
                sp.kin_off[t + 1] - sp.kin_off[t],
                sp.enc_off[t + 1] - sp.enc_off[t],
                sp.act_off[t + 1] - sp.act_off[t],
                sp.sr_off[t + 1] - sp.sr_off[t],
                d.KI + sp.kin_off[t],
                d.src + sp.enc_off[t],
                d.enc_bits + sp.enc_off[t]};
}

// encoder forward, shared split (kp_cv_fused.hpp); ne == nk here
void cv_fwd_shared(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, const CvDev& d, const CvStep& st) {
  const int DP = c->dp, ne = st.ne, nsr = st.nsr;
  hipLaunchKernelGGL(kpcvf::kp_cv_lhs_map, dim3(nsr), dim3(256), 0, c->stream, nsr, d.sr_src + sp.sr_off[st.t], d.X, DP,
                     c->d_conv_w, c->d_conv_b, c->d_bn_a, c->d_bn_b, d.map_l, d.relu_s);
  KP_HIP(hipGetLastError());
  launch_gemm_abt(c, d.map_l, kpcvf::NLHS, nsr, c->cv_wlc.as<float>(), kpcvf::NLHS, c->dim, kpcvf::NLHS, d.slab_l,
                  c->dim, c->d_fc_b, 0, kpcvf::KSL);
  hipLaunchKernelGGL(kpcvf::kp_cv_mid_map, dim3((ne * kpcvf::CH * 2 + 255) / 256), dim3(256), 0, c->stream, ne, st.ES,
                     c->dE, d.X, c->dR, DP, c->d_conv_w, c->d_conv_b, c->d_bn_a, c->d_bn_b, d.map_m, d.relu);
  KP_HIP(hipGetLastError());
  launch_gemm_abt(c, d.map_m, kpcvf::NMID, ne, c->cv_wtm.as<float>(), kpcvf::NMID, c->dim, kpcvf::NMID, d.mid, c->dim,
                  nullptr, 0, 1);
  hipLaunchKernelGGL(kp_cv_post_fc3, dim3(ne), dim3(256), 0, c->stream, ne, d.slab_l, kpcvf::KSL, nsr, d.mid, 1,
                     c->cv_trel.as<float>(), st.ES, d.psr + sp.kin_off[st.t], kc, st.EB, d.bits, c->d_bn_a, c->d_bn_b,
                     d.Q);
  KP_HIP(hipGetLastError());
}

// conv + FC forward in one kernel (kp_cv_fused.hpp) -> the FC split-K slabs
void cv_fwd_fused(kp_ctx* c, const CvConst& kc, const CvDev& d, const CvStep& st) {
  const int ne = st.ne;
  const int fgrid = kpcvf::NSPLIT * ((ne + kpcvf::MT - 1) / kpcvf::MT);
  if (kc.fr_step)
    hipLaunchKernelGGL(kpcvf::kp_cv_fwd_fused<true>, dim3(fgrid), dim3(512), kpcvf::FWD_LDS, c->stream, ne, st.ES,
                       c->dE, d.X, c->dR, c->dp, c->d_conv_w, c->d_conv_b, c->d_bn_a, c->d_bn_b, d.fw, c->d_fc_b,
                       c->dim, st.EB, d.bits, d.s_in, d.s_fm, d.slab, d.relu, 0, kpcvf::FR * 8, kpcvf::NSPLIT, 8);
  else
    hipLaunchKernelGGL(kpcvf::kp_cv_fwd_fused<false>, dim3(fgrid), dim3(512), kpcvf::FWD_LDS, c->stream, ne, st.ES,
                       c->dE, d.X, c->dR, c->dp, c->d_conv_w, c->d_conv_b, c->d_bn_a, c->d_bn_b, d.fw, c->d_fc_b,
                       c->dim, st.EB, d.bits, d.s_in, d.s_fm, d.slab, d.relu, 0, kpcvf::FR * 8, kpcvf::NSPLIT, 8);
  KP_HIP(hipGetLastError());
}

// conv forward, then the FC as a split-K GEMM -> the FC split-K slabs
void cv_fwd_plain(kp_ctx* c, const CvConst& kc, const CvDev& d, const CvStep& st) {
  KP_CONV_FWD(dim3(st.ne), dim3(256), 0, c->stream, st.ne, st.ES, c->dE, d.X, c->dR, kc, c->d_conv_w, c->d_conv_b,
              c->d_bn_a, c->d_bn_b, st.EB, d.bits, d.flat);
  KP_HIP(hipGetLastError());
  launch_gemm_abt(c, d.flat, c->hidden, st.ne, c->d_fc_w, c->hidden, c->dim, c->hidden, d.slab, c->dim, c->d_fc_b, 0,
                  d.KS);
}

// encoder forward of the step's rows -> Q (conve.py:133-153, train-mode dropouts)
void cv_forward(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, const CvDev& d, const CvStep& st) {
  if (st.ne <= 0) return;
  if (d.shared) return cv_fwd_shared(c, kc, sp, d, st);
  if (d.fused)
    cv_fwd_fused(c, kc, d, st);
  else
    cv_fwd_plain(c, kc, d, st);
  hipLaunchKernelGGL(kp_cv_post_fc, dim3(st.ne), dim3(256), 0, c->stream, st.ne, d.slab, d.KS, kc, st.EB, d.bits,
                     c->d_bn_a, c->d_bn_b, d.Q);
  KP_HIP(hipGetLastError());
}

// O = sum_e G(x . E_e) E_e of the step's kelpie pairs over the frozen entities
template <int DB>
void launch_cv_attn(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, const CvDev& d, const CvStep& st) {
  const AttnPlan& plan = d.step_plan[st.t];
  const float* gscale = d.gscale + sp.kin_off[st.t];
  if (c->attn_mode == 1)
    launch_attn3<DB, ATT_BCE_O>(c, c->n_ent, d.Q, st.nk, plan, nullptr, nullptr, d.O, gscale, kc.ylo);
  else
    hipLaunchKernelGGL((kp_attn<DB, ATT_BCE_O>), dim3(plan.n_wg), dim3(256), attn_lds_bytes(c->dp / 16), c->stream,
                       c->dE, c->n_ent, d.Q, st.nk, plan.wk, nullptr, nullptr, d.O, gscale, kc.ylo);
}

// the step's hot launch, bracketed by the context's event pair `launch` when timed
void cv_attention(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, const CvDev& d, const CvStep& st,
                  int64_t launch) {
  if (c->time_hot) KP_HIP(hipEventRecord(c->event(2 * launch), c->stream));
  KP_DB_DISPATCH(c->dp / 16, 4, "ConvE: unsupported padded dimension", launch_cv_attn<DB>(c, kc, sp, d, st));
  KP_HIP(hipGetLastError());
  if (c->time_hot) {
    KP_HIP(hipEventRecord(c->event(2 * launch + 1), c->stream));
    c->hot_pairs.push_back({(double)st.nk, 0.0});
  }
}

// dL/dx -> dL/dfc of the step's kelpie pairs, and G at the kelpie column
void cv_dx(kp_ctx* c, const CvConst& kc, const CvDev& d, const CvStep& st) {
  const int nk = st.nk, n_split = d.step_plan[st.t].wk.n_parts;
  __bf16* g3p = d.shared ? nullptr : d.g3;
  const int nj = (c->dp + 63) / 64;
#define CV_DX1(J)                                                                                                \
  hipLaunchKernelGGL(kp_cv_dx1<J>, dim3(nk), dim3(64), 0, c->stream, nk, kc, st.KI, d.Q, d.O, n_split, d.tails, \
                     c->dE, d.X, d.bits, c->d_bn_a, d.dfc, d.gk, g3p)
  if (!c->cv_dx_block && nj <= 2)
    CV_DX1(2);
  else if (!c->cv_dx_block && nj <= 4)
    CV_DX1(4);
  else if (!c->cv_dx_block && nj <= 6)
    CV_DX1(6);
  else if (!c->cv_dx_block && nj <= 8)
    CV_DX1(8);
  else
    hipLaunchKernelGGL(kp_cv_dx, dim3(nk), dim3(256), 0, c->stream, nk, kc, st.KI, d.Q, d.O, n_split, d.tails, c->dE,
                       d.X, d.bits, c->d_bn_a, d.dfc, d.gk, g3p);
#undef CV_DX1
  KP_HIP(hipGetLastError());
}

// encoder backward, shared split: map rows 0-17 once per kelpie row (the sum of its pairs'
// dfc; rows 18-19 of its ReLU bytes are 0), then rows 18-19 per pair, assembled into the
// pairs' dl rows
void cv_bwd_shared(kp_ctx* c, const CvStepPlan& sp, const CvDev& d, const CvStep& st) {
  const int DP = c->dp, nk = st.nk, nsr = st.nsr;
  hipLaunchKernelGGL(kpcvf::kp_cv_slot_g, dim3(nsr), dim3(256), 0, c->stream, nsr, d.sr_rng + sp.sr_off[st.t], d.dfc,
                     c->dim, d.gs);
  KP_HIP(hipGetLastError());
  launch_gemm_abt(c, d.gs, c->dim, nsr, c->cv_wtl.as<float>(), c->dim, kpcvf::NLHS, c->dim, d.map_l, kpcvf::NLHS,
                  nullptr, 0, 1);
  hipLaunchKernelGGL(kpcvf::kp_cv_lhs_convt, dim3(nsr), dim3(256), 0, c->stream, nsr, d.map_l, d.relu_s, c->d_conv_w,
                     c->d_bn_a, DP, d.dls);
  KP_HIP(hipGetLastError());
  launch_gemm_abt(c, d.dfc, c->dim, nk, c->cv_wfm.as<float>(), c->dim, kpcvf::NMID, c->dim, d.map_m, kpcvf::NMID,
                  nullptr, 0, 1);
  hipLaunchKernelGGL(kpcvf::kp_cv_mid_convt, dim3((nk + kpcvf::MPW - 1) / kpcvf::MPW), dim3(256), 0, c->stream, nk,
                     d.map_m, d.relu, c->d_conv_w, c->d_bn_a, d.psr + sp.kin_off[st.t], d.dls, DP, d.dl);
  KP_HIP(hipGetLastError());
}

// FC^T and transposed conv in one kernel (kp_cv_fused.hpp), its slabs reduced into slab 0
void cv_bwd_fused(kp_ctx* c, const CvConst& kc, const CvDev& d, const CvStep& st) {
  const int DP = c->dp, nk = st.nk;
  const int bgrid = kpcvf::NSPLIT * ((nk + kpcvf::MT - 1) / kpcvf::MT);
  hipLaunchKernelGGL(kpcvf::kp_cv_bwd_fused, dim3(bgrid), dim3(512), kpcvf::BWD_LDS, c->stream, nk, d.g3, d.bw, d.relu,
                     c->d_conv_w, c->d_bn_a, d.s_fm, DP, d.dl);
  KP_HIP(hipGetLastError());
  const long long nr = (long long)nk * kpcvf::LR * kpcvf::IW;
  hipLaunchKernelGGL(kpcvf::kp_cv_dl_reduce, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c->stream, nk, DP,
                     kc.has_in ? st.EB : nullptr, d.bits, d.s_in, d.dl);
  KP_HIP(hipGetLastError());
}

// FC^T as a GEMM, then the transposed conv
void cv_bwd_plain(kp_ctx* c, const CvConst& kc, const CvDev& d, const CvStep& st) {
  const int nk = st.nk;
  launch_gemm_abt(c, d.dfc, c->dim, nk, d.wt, c->dim, c->hidden, c->dim, d.dflat, c->hidden, nullptr, 0, 1);
  const size_t shm_cbwd = sizeof(float) * 32 * 20 * (c->dim / 20 - 2);
  hipLaunchKernelGGL(kp_cv_conv_bwd, dim3(nk), dim3(256), shm_cbwd, c->stream, nk, kc, d.dflat, d.flat, c->d_conv_w,
                     c->d_bn_a, st.EB, d.bits, d.dl);
  KP_HIP(hipGetLastError());
}

// gradient assembly + Adam of the step's active slots.  d.act entries index kinst / finst
// relative to this step's lists; the frozen-head pairs read their encodings from Q (fr_step)
// or the batch's FC rows
void cv_update(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, const CvDev& d, const CvStep& st,
               const CvOpt& opt) {
  if (st.na <= 0) return;
  const int t = st.t, nch = sp.fch_off[t + 1] - sp.fch_off[t];
  if (nch > 0) {
    hipLaunchKernelGGL(kp_cv_fgrad, dim3(nch), dim3(256), 0, c->stream, kc, d.fch + sp.fch_off[t],
                       d.act + sp.act_off[t], d.FI + sp.fin_off[t], kc.fr_step ? d.Q : d.fcf, d.bits, c->d_bn_a,
                       c->d_bn_b, d.X, d.fpart);
    KP_HIP(hipGetLastError());
  }
  if (marks_at_step(d.marks, t))  // the step ends a marked epoch of one of its slots: the MARKS form instead
    hipLaunchKernelGGL(kp_cv_update<true>, dim3(st.na), dim3(256), 0, c->stream, kc, d.act + sp.act_off[t], d.Q, d.gk,
                       d.dl, d.fpart, d.X, d.S1, d.S2, opt, CvMarkArgs<true>{d.mark_row + sp.act_off[t], d.marks.X});
  else
    hipLaunchKernelGGL(kp_cv_update<false>, dim3(st.na), dim3(256), 0, c->stream, kc, d.act + sp.act_off[t], d.Q, d.gk,
                       d.dl, d.fpart, d.X, d.S1, d.S2, opt, CvMarkArgs<false>{});
  KP_HIP(hipGetLastError());
}

// kp_posttrain_rank_trace's device side (loss == nullptr: no trace): the common part, and
// ConvE's own: the step's rows, one chunk's logits [chunk][ld] and the rows' summed terms
constexpr size_t TRACE_WS_BYTES = (size_t)64 << 20;  // a chunk's logits, as TOPK_WS_BYTES
struct CvTraceDev : TraceDev {
  float *rows = nullptr, *scores = nullptr;
  double* rowloss = nullptr;
  int chunk = 0, ld = 0;
};

CvTraceDev cv_trace_workspaces(kp_ctx* c, const kp_batch* bt, const PostReq& rq, const CvStepPlan& sp) {
  CvTraceDev t;
  if (!rq.trace) return t;
  int max_rows = 1;
  for (int s = 0; s < sp.T; ++s)
    max_rows = std::max(max_rows, (sp.kin_off[s + 1] - sp.kin_off[s]) + (sp.fin_off[s + 1] - sp.fin_off[s]));
  t.ld = round_up(c->n_ent, 4);
  t.chunk = (int)std::min<size_t>((size_t)max_rows, std::max<size_t>(1, TRACE_WS_BYTES / (sizeof(float) * t.ld)));
  if (const char* e = std::getenv("KP_TRACE_CHUNK"))  // diagnostic: n rows per chunk, as KP_PROBE_CHUNK
    t.chunk = std::min(max_rows, std::max(1, std::atoi(e)));
  static_cast<TraceDev&>(t) = upload_trace(c, bt, rq);
  t.rows = ensure_n<float>(c->cv.tr_rows, (size_t)max_rows * c->dp);
  t.scores = ensure_n<float>(c->cv.tr_scores, (size_t)t.chunk * t.ld);
  t.rowloss = ensure_n<double>(c->cv.tr_rowloss, (size_t)max_rows);
  return t;
}

// the losses of step t's active slots, after the forward and before the update moves x
void cv_trace_step(kp_ctx* c, const CvConst& kc, const CvStepPlan& sp, const CvDev& d, const CvStep& st,
                   const CvTraceDev& tr) {
  if (!tr.loss || st.na <= 0) return;
  const int t = st.t, nk = st.nk, nf = sp.fin_off[t + 1] - sp.fin_off[t], n = nk + nf;
  const CvFInst* FI = d.FI + sp.fin_off[t];
  const float* TQ = d.Q;  // fr_step: the step's encoder rows, kelpie pairs first
  if (!kc.fr_step) {
    hipLaunchKernelGGL(kp_cv_trace_rows, dim3(n), dim3(256), 0, c->stream, nk, nf, kc, d.Q, FI, d.fcf, d.bits, c->d_bn_a,
                       c->d_bn_b, tr.rows);
    KP_HIP(hipGetLastError());
    TQ = tr.rows;
  }
  for (int r0 = 0; r0 < n; r0 += tr.chunk) {  // E streams once per chunk of rows, not once per row
    const int m = std::min(tr.chunk, n - r0);
    launch_gemm_abt(c, TQ + (size_t)r0 * c->dp, c->dp, m, c->dE, c->dp, c->n_ent, c->dp, tr.scores, tr.ld, nullptr, 0, 1);
    hipLaunchKernelGGL(kp_cv_trace_row, dim3(m), dim3(256), 0, c->stream, r0, nk, kc, tr.scores, tr.ld, TQ, st.KI, FI,
                       d.tails, d.X, tr.rowloss);
    KP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(kp_cv_trace_slot, dim3((st.na + 63) / 64), dim3(64), 0, c->stream, st.na, nk, kc,
                     d.act + sp.act_off[t], st.KI, FI, tr.rowloss, tr.off, t, tr.loss);
  KP_HIP(hipGetLastError());
}

// the epoch/step loop; returns the hot (attention) launches
int64_t cv_step_loop(kp_ctx* c, const kp_hp* hp, const CvConst& kc, const CvStepPlan& sp, const CvDev& d,
                     const CvTraceDev& tr) {
  CvOpt opt{};
  opt.lr = hp->lr;
  opt.b1 = hp->beta1;
  opt.b2 = hp->beta2;
  opt.eps = hp->eps;
  opt.one_minus_b1 = (float)(1.0 - (double)hp->beta1);
  opt.one_minus_b2 = (float)(1.0 - (double)hp->beta2);
  int64_t launches = 0;
  c->hot_pairs.clear();
  c->hot_iv.clear();
  for (int t = 0; t < sp.T; ++t) {
    const CvStep st = cv_step(sp, d, t);
    cv_forward(c, kc, sp, d, st);
    if (st.nk > 0) {
      cv_attention(c, kc, sp, d, st, launches++);
      cv_dx(c, kc, d, st);
      if (d.shared)
        cv_bwd_shared(c, sp, d, st);
      else if (d.fused)
        cv_bwd_fused(c, kc, d, st);
      else
        cv_bwd_plain(c, kc, d, st);
    }
    const AdamStep as = adam_step(hp, t);
    opt.step_size = as.step_size;
    opt.bc2_sqrt = as.bc2_sqrt;
    cv_trace_step(c, kc, sp, d, st, tr);
    cv_update(c, kc, sp, d, st, opt);
  }
  return launches;
}

// what a rank row's pass through encode_eval holds: its feature maps, FC output and encoder output
size_t cv_enc_row_bytes(const kp_ctx* c) { return sizeof(float) * ((size_t)c->hidden + c->dim + c->dp); }

// the optional requests' uploads and buffers (ahead of the step loop), in the order the stream
// has always seen them: the probes, the trace, the marks.  A chunk's rank rows also pass
// through encode_eval's feature maps and FC output, counted into the chunk's budget (which
// makes upload_rank_rows upload the rows' encoder sources as well); with the marks, per entry
// of the active lists the mark row its update also stores
CvTraceDev cv_request_workspaces(kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq,
                                 const CvStepPlan& sp, CvDev& d) {
  const size_t enc_row = cv_enc_row_bytes(c);
  d.probes = upload_probes(c, bt, rq, d.X, enc_row);
  const CvTraceDev tr = cv_trace_workspaces(c, bt, rq, sp);
  d.marks = upload_marks(c, c->cv.marks, hp, bt, rq, d.X, enc_row);
  if (d.marks.nm > 0) {
    const std::vector<int32_t> mr = marks_act_rows(d.marks, sp.act_off, sp.T, [&](int i) { return sp.acts[i].slot; });
    d.mark_row = upload(c, c->cv.mark_row, mr.data(), mr.size());
  }
  return tr;
}

// rank: sigmoid(enc(x, R_p) . E_e), kelpie column, maximizer.  The slots' encoder output is
// c->cv.q (the step's rows in the loop), not a buffer of the set's own.
RankSet cv_rank(kp_ctx* c, const CvConst& kc, const kp_batch* bt, const PostReq& rq, const CvDev& d) {
  const int ns = bt->n_slots, K = c->n_ent, DP = c->dp;
  RankSetReq sr;
  sr.rank64 = c->cv_rank64 != 0;
  sr.enc_row_bytes = cv_enc_row_bytes(c);
  sr.enc_q = ensure_n<float>(c->cv.q, (size_t)std::max(ns, d.mk) * DP);
  const RankSet rk = upload_slots(c, c->rank.slots, bt, rq, d.X, sr);
  if (c->cv_rank64) {
    // the slots, then the probes on the slots' rows, then the marks on the mark workspace: a
    // chunk's rows through the encoder (eval mode) on the set's rows, then the queries and the count
    const auto queries = [c, K, DP](const RankSet& rr, int r0, int m) {
      encode_eval(c, m, rr.enc_src + r0, rr.X, rr.enc_q);
      hipLaunchKernelGGL(kp_cv_rankq64, dim3(m), dim3(64), 0, c->stream, rr.enc_q, rr.X, c->dE, K, DP,
                         rr.rows + 3 * (size_t)r0, m, rr.q, rr.t, rr.kcol);
      KP_HIP(hipGetLastError());
    };
    for (const RankSet* set : {&rk, &d.probes, &d.marks.rows}) rank_rows(c, *set, RANK64_SIGMOID, queries);
  } else {
    const int ld = round_up(K + 1, 4);
    float* dScores = ensure_n<float>(c->rank.scores, (size_t)ns * ld);
    encode_eval(c, ns, rk.enc_src, d.X, rk.enc_q);
    launch_score_gemm(c, rk.enc_q, ns, dScores, ld, 1);
    hipLaunchKernelGGL(kp_cv_kcol, dim3(ns), dim3(64), 0, c->stream, ns, kc, rk.enc_q, d.X, dScores, ld);
    KP_HIP(hipGetLastError());
    launch_rank_count(c, ns, dScores, ld, K + 1, rk.po, rk.filt_off, rk.filt, 0, rk.target, rk.rank);
  }
  return rk;
}

}  // namespace

// KP_HOST_TIMES=1 (kp_posttrain.hpp) prints the host time of the planning (kp_cv_plan.hpp),
// the uploads, enqueueing the step loop, and the rank with the final wait
void conve_posttrain_rank(kp_ctx* c, const kp_hp* hp, const kp_batch* bt, const PostReq& rq) {
  const double t_in = g_host_times ? host_ms() : 0.0;
  // (with ConvE's hyper-parameter check at its place among the request's)
  require_request(c, hp, bt, rq, c->cv_rank64 != 0, kp_model_name(c->model));
  const CvConst kc = make_const(c, hp);

  CvStepPlan sp;
  if (const char* why = cv_step_plan(c->n_ent, c->n_rel2, c->dim, hp->batch_size, hp->epochs, kc.has_in != 0,
                                     kc.has_fm != 0, kc.has_mask != 0, kc.fr_step != 0, bt, sp))
    throw KpError{KP_EINVAL, std::string("ConvE: ") + why};
  const double t_plan = g_host_times ? host_ms() : 0.0;

  std::vector<float> xp;
  CvDev d = cv_workspaces(c, bt, sp, xp);
  const CvTraceDev tr = cv_request_workspaces(c, hp, bt, rq, sp, d);
  const double t_up = g_host_times ? host_ms() : 0.0;
  KP_HIP(hipEventRecord(c->ev0, c->stream));
  const int nfp = cv_frozen_fc(c, kc, sp, d);
  cv_step_workspaces(c, kc, sp, nfp, d);

  const int64_t launches = cv_step_loop(c, hp, kc, sp, d, tr);
  const double t_loop = g_host_times ? host_ms() : 0.0;

  const RankSet rk = cv_rank(c, kc, bt, rq, d);
  KP_HIP(hipEventRecord(c->ev1, c->stream));
  download_results(c, bt, d.X, rk, xp, rq, d.probes, tr, d.marks);
  if (g_host_times)
    std::fprintf(stderr, "[kp_cv] slots %d steps %d pairs %zu: plan %.2f ms, uploads %.2f ms, loop enqueue %.2f ms, "
                 "rank + wait %.2f ms\n", bt->n_slots, sp.T, sp.kinst.size(), t_plan - t_in, t_up - t_plan,
                 t_loop - t_up, host_ms() - t_loop);
  record_hot_timing(c, launches, c->ev0, c->ev1);  // the whole call counts as its loop
}

float* conve_fc_wt(kp_ctx* c) {
  // FC weight transposed [hidden][dim] for the backward GEMM (built once, kept in the context)
  if (!c->d_fc_wt) {
    std::vector<float> w((size_t)c->dim * c->hidden), wt((size_t)c->dim * c->hidden);
    KP_HIP(hipMemcpy(w.data(), c->d_fc_w, sizeof(float) * w.size(), hipMemcpyDeviceToHost));
    for (int o = 0; o < c->dim; ++o)
      for (int j = 0; j < c->hidden; ++j) wt[(size_t)j * c->dim + o] = w[(size_t)o * c->hidden + j];
    KP_HIP(hipMalloc(&c->d_fc_wt, sizeof(float) * wt.size()));
    KP_HIP(hipMemcpy(c->d_fc_wt, wt.data(), sizeof(float) * wt.size(), hipMemcpyHostToDevice));
  }
  return c->d_fc_wt;
}

void conve_scores_dev(kp_ctx* c, int n, const int32_t* d_heads, const int32_t* d_rels, float* d_out, int ld) {
  if (n <= 0) return;
  std::vector<int32_t> h(n), r(n);
  KP_HIP(hipMemcpyAsync(h.data(), d_heads, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipMemcpyAsync(r.data(), d_rels, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipStreamSynchronize(c->stream));
  std::vector<int2> src(n);
  for (int i = 0; i < n; ++i) src[i] = make_int2(h[i], r[i]);
  DevBuf bs, bq;
  int2* dsrc = upload(c, bs, src.data(), src.size());
  float* dQ = ensure_n<float>(bq, (size_t)n * c->dp);
  encode_eval(c, n, dsrc, nullptr, dQ);
  launch_gemm_abt(c, dQ, c->dp, n, c->dE, c->dp, c->n_ent, c->dp, d_out, ld, nullptr, 1, 1);
  KP_HIP(hipStreamSynchronize(c->stream));
  bs.release();
  bq.release();
}

void conve_all_scores(kp_ctx* c, int n, const int32_t* heads, const int32_t* rels, float* out) {
  if (n <= 0) return;
  DevBuf bh, br, bs;
  int32_t* dh = upload(c, bh, heads, (size_t)n);
  int32_t* dr = upload(c, br, rels, (size_t)n);
  float* dS = ensure_n<float>(bs, (size_t)n * c->n_ent);
  conve_scores_dev(c, n, dh, dr, dS, c->n_ent);
  KP_HIP(hipMemcpyAsync(out, dS, sizeof(float) * (size_t)n * c->n_ent, hipMemcpyDeviceToHost, c->stream));
  KP_HIP(hipStreamSynchronize(c->stream));
  for (DevBuf* b : {&bh, &br, &bs}) b->release();
}

#ifdef KP_ATTN_STAMPS
// the ConvE translation unit's copy of kpattn::g_attn_stamps (device globals are per code object)
extern "C" int kp_debug_attn_stamps_conve(unsigned long long* out, int reset) {
  KP_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(kpattn::g_attn_stamps), sizeof(unsigned long long) * 8));
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    KP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(kpattn::g_attn_stamps), z, sizeof(z)));
  }
  return 0;
}
#endif
