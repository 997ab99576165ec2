// kp_attn64.hpp -- the fp64 attention of kp_posttrain_rank_f64 (include/kelpie_hip.h, "fp64"):
// for a launch's query rows in fp64 and a key range of the fp32 entity table, the running max
// m, l = sum_e exp(s_e - m) and O = sum_e exp(s_e - m) E_e with s_e = q . E_e, everything in
// fp64 and both contractions on v_mfma_f64_16x16x4_f64.  E stays fp32 in HBM and in LDS and is
// upcast at the operand read (exact), so no second image of the table is kept.
//
// Work: one workgroup of four waves per (16-query tile, key range); the grid is (query tiles,
// ranges).  Per 16-key tile:
//   1. the tile's rows go to LDS (fp32, rows past the range's end as zeros);
//   2. S^T = E_tile . Q^T (keys x queries): the D columns are cut into four equal runs, wave w
//      contracts run w (DB MFMAs, its slice of Q held in registers for the whole range) and
//      leaves its partial in LDS; every wave then adds the four partials in wave order, so all
//      four hold the same S^T bit for bit;
//   3. the online softmax per query (a query is an MFMA column: lane & 15): the tile's max and
//      sum meet over a lane's four rows and the lanes 16, 32 apart, a fixed order;
//   4. O^T += E_tile^T . P^T: the sixteen-column blocks of D are dealt to the waves (block b to
//      wave b % 4), four MFMAs per block.  S^T's C layout (row = key = (lane >> 4) + 4 reg) is
//      the B operand of step reg as it stands: the keys of step reg are (lane >> 4) + 4 reg on
//      both operands, so P never moves between lanes.
// Keys past the range's end are masked (p = 0 and the row of zeros), a range without keys
// writes the empty partial (m = -inf, l = 0, O = 0).  No atomics: a rerun is bitwise equal.
// The partials of the ranges are merged by log-sum-exp in range order by the consumers
// (kp_complex.hip: kp_cx_contrib64, kp_cx_lse_merge<double>).
// LDS: 16 (16 DB + 1) floats + 8 KiB of partials (33.7 KiB at DB = 25); registers: DB doubles
// of Q and 4 ceil(DB / 4) doubles of O per lane; no scratch.
#pragma once

#include "kp_common.hpp"

namespace kpattn {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int A64_QT = 16;  // queries per workgroup
constexpr int A64_KT = 16;  // keys per tile

template <int DB, bool WITH_O>
__global__ __launch_bounds__(256) void kp_attn64(const float* __restrict__ E, int n_ent, const double* __restrict__ Q,
                                                 int nq, int keys_per_range, double* __restrict__ out_m,
                                                 double* __restrict__ out_l, double* __restrict__ out_O) {
  constexpr int DP = 16 * DB;
  constexpr int ES = DP + 1;         // LDS row stride (odd: the sixteen keys of a read fall on sixteen banks)
  constexpr int NB = (DB + 3) / 4;   // O blocks per wave
  __shared__ float Es[A64_KT * ES];
  __shared__ double Sp[4][4][64];  // [wave][register][lane] partial S^T
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int c16 = lane & 15, g4 = lane >> 4;
  const int q0 = blockIdx.x * A64_QT;
  const int r = blockIdx.y;
  const long long kb = (long long)r * keys_per_range;
  const int k0 = (int)(kb < n_ent ? kb : n_ent);
  const int k1 = (int)(kb + keys_per_range < n_ent ? kb + keys_per_range : n_ent);
  const int qi = q0 + c16;
  const double kInf = __builtin_inf();

  // the wave's slice of Q^T as B operands: step j holds Q[qi][4 (w DB + j) + g4]
  double qv[DB];
#pragma unroll
  for (int j = 0; j < DB; ++j) qv[j] = qi < nq ? Q[(size_t)qi * DP + 4 * (w * DB + j) + g4] : 0.0;
  f64x4 oacc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) oacc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
  double m = -kInf, l = 0.0;

  for (int kt = k0; kt < k1; kt += A64_KT) {
    const int nk = min(A64_KT, k1 - kt);
    // 1. the tile (rows kt .. kt + 15 are contiguous in the table)
    for (int e = tid; e < A64_KT * DP; e += 256) {
      const int kr = e / DP, d = e - kr * DP;
      Es[kr * ES + d] = kr < nk ? E[(size_t)(kt + kr) * DP + d] : 0.f;
    }
    __syncthreads();
    // 2. the wave's run of D
    f64x4 s = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < DB; ++j) {
      const double a = (double)Es[c16 * ES + 4 * (w * DB + j) + g4];
      s = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qv[j], s, 0, 0, 0);
    }
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) Sp[w][rg][lane] = s[rg];
    __syncthreads();
    // 3. S^T (row = key g4 + 4 rg, column = query c16) and the online softmax
    double sv[4], p[4];
    double tmax = -kInf;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      sv[rg] = ((Sp[0][rg][lane] + Sp[1][rg][lane]) + Sp[2][rg][lane]) + Sp[3][rg][lane];
      if (g4 + 4 * rg < nk) tmax = fmax(tmax, sv[rg]);
    }
    tmax = fmax(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmax(tmax, __shfl_xor(tmax, 32, 64));
    const double m_new = fmax(m, tmax);  // finite: the tile has a key
    const double scale = exp(m - m_new);  // 0 at the first tile
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) p[rg] = g4 + 4 * rg < nk ? exp(sv[rg] - m_new) : 0.0;
    double ps = (p[0] + p[1]) + (p[2] + p[3]);
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * scale + ps;
    m = m_new;
    // 4. the wave's blocks of O^T (row = column 16 blk + g4 + 4 rg of D, column = query c16)
    if constexpr (WITH_O) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int blk = w + 4 * b;
        if (blk < DB) {
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) oacc[b][rg] *= scale;
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const double a = (double)Es[(g4 + 4 * rg) * ES + 16 * blk + c16];
            oacc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, p[rg], oacc[b], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // the next tile overwrites Es and Sp
  }

  if (qi < nq) {
    const size_t row = (size_t)r * nq + qi;
    if (w == 0 && g4 == 0) {
      out_m[row] = m;
      out_l[row] = l;
    }
    if constexpr (WITH_O) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int blk = w + 4 * b;
        if (blk < DB) {
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) out_O[row * DP + 16 * blk + g4 + 4 * rg] = oacc[b][rg];
        }
      }
    }
  }
}

// Host: nq queries over the context's table in `ranges` key ranges of keys_per_range keys
// (a multiple of the planner's 32-key tile); out_m / out_l [ranges][nq], out_O [ranges][nq][dp]
template <int DB>
void launch_attn64(kp_ctx* c, bool with_o, const double* Q, int nq, int ranges, int keys_per_range, double* m,
                   double* l, double* O) {
  if (nq <= 0) return;
  const dim3 grid((nq + A64_QT - 1) / A64_QT, ranges);
  if (with_o)
    hipLaunchKernelGGL((kp_attn64<DB, true>), grid, dim3(256), 0, c->stream, c->dE, c->n_ent, Q, nq, keys_per_range, m,
                       l, O);
  else
    hipLaunchKernelGGL((kp_attn64<DB, false>), grid, dim3(256), 0, c->stream, c->dE, c->n_ent, Q, nq, keys_per_range,
                       m, l, O);
  KP_HIP(hipGetLastError());
}

}  // namespace kpattn
