// attn_micro.hip -- standalone timing + fp64 check of kp_attn3 (the ComplEx / ConvE
// attention pass) on one synthetic problem, for A/B of kernel variants built with
// different defines (tools/attn_micro.sh).  Not part of the product library.
//
//   attn_micro <DB 25|13> <mode 0|2> <n_ent> <nq> <iters> [scale] [part 0|1|2]
//              [--ranges S] [--inflight N] [--streams K]
//
// --ranges S: S key ranges per query tile, one workgroup per unit (the library's
// KP_ATTN_RANGES); --inflight N: the planner's in-flight hint (kp_ctx_set_inflight).
// --streams K: K contexts, each on its own stream with its own partials, launch the kernel
// back to back, each launch followed by a short dependent kernel that reads the partials
// once (it stands in for the merge, its work proportional to the ranges like the merge's);
// "ms" is then the union time per launch, host time over all launches / (K x iters).
//
// Prints one JSON line: per-launch ms (HIP events around `iters` back-to-back launches),
// fp32-equivalent TF/s (4 D per (query, entity) with O, 2 D without), and the largest
// relative error of the merged (m, l, O) of 16 sampled queries against fp64.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <random>

#include "kp_attn3.hpp"  // -I selects the source tree under test (tools/attn_micro.sh)
#if __has_include("kp_attn5.hpp")
#include "kp_attn5.hpp"
#define KP_MICRO_HAS_ATTN5 1
#endif
#if __has_include("kp_attn6.hpp")
#include "kp_attn6.hpp"
#define KP_MICRO_HAS_ATTN6 1
#endif
#if __has_include("kp_attn4.hpp")
#include "kp_attn4.hpp"
#define KP_MICRO_HAS_ATTN4 1
#endif

using namespace kpattn;

// s_memrealtime calibration (KP_MICRO_RTCAL=1): one wave spins until the counter has
// advanced by `ticks` (bounded by an iteration cap), timed by HIP events on the host side
__global__ void kp_rtcal(unsigned long long ticks, unsigned long long* out) {
  unsigned long long r0, t0, r1 = 0, t1 = 0;
  asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(r0), "=s"(t0)::"memory");
  for (long long it = 0; it < (1LL << 32); ++it) {
    asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1), "=s"(t1)::"memory");
    if (r1 - r0 >= ticks) break;
  }
  if (threadIdx.x == 0) {
    out[0] = r1 - r0;
    out[1] = t1 - t0;
  }
}

// a pure-MFMA kernel (KP_MICRO_MFMA=1): every wave runs `iters` dependent chains of
// v_mfma_f32_16x16x32_bf16 on register operands, no memory traffic but the final store;
// thread 0 of each workgroup stamps its start and end (100 MHz realtime) like the clock build
__global__ __launch_bounds__(256, 1) void kp_mfma_spin(int iters, float* out, unsigned long long* st) {
  unsigned long long r0;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r0)::"memory");
  typedef __bf16 b8 __attribute__((ext_vector_type(8)));
  b8 a, b;
  for (int j = 0; j < 8; ++j) {
    a[j] = (__bf16)(0.001f * (threadIdx.x + j));
    b[j] = (__bf16)(0.002f * (blockIdx.x + j));
  }
  f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, c2 = c0, c3 = c0;
  for (int i = 0; i < iters; ++i) {
    c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c3, 0, 0, 0);
  }
  out[blockIdx.x * 256 + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3];
  unsigned long long r1;
  asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1)::"memory");
  if (threadIdx.x == 0) {
    st[2 * blockIdx.x] = r0;
    st[2 * blockIdx.x + 1] = r1;
  }
}

// the pure-MFMA kernel plus the attention's other traffic (KP_MICRO_MFMA2=1): MODE bit 0 =
// two ds_read_b128 of the dynamic LDS per four MFMAs, bit 1 = one 16-B global load per four
// MFMAs streaming through a 35 MB buffer; the loaded values feed the next MFMA operands
template <int MODE>
__global__ __launch_bounds__(256, 1) void kp_mfma_spin2(int iters, const uint4* __restrict__ buf, long long nbuf,
                                                         float* out, unsigned long long* st) {
  extern __shared__ uint4 lds_s[];
  unsigned long long r0;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r0)::"memory");
  typedef __bf16 b8 __attribute__((ext_vector_type(8)));
  b8 a, b;
  for (int j = 0; j < 8; ++j) {
    a[j] = (__bf16)(0.001f * (threadIdx.x + j));
    b[j] = (__bf16)(0.002f * (blockIdx.x + j));
  }
  for (int i = threadIdx.x; i < 9728; i += 256) lds_s[i] = make_uint4(i, i + 1, i + 2, i + 3);
  __syncthreads();
  f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, c2 = c0, c3 = c0;
  long long g = (long long)blockIdx.x * 4096 + threadIdx.x;
  for (int i = 0; i < iters; ++i) {
    if (MODE & 1) {
      const uint4 x = lds_s[(threadIdx.x + 64 * (i & 127)) % 9728];
      const uint4 y = lds_s[(threadIdx.x + 64 * ((i + 37) & 127) + 4800) % 9728];
      a = __builtin_bit_cast(b8, x);
      b = __builtin_bit_cast(b8, y);
    }
    if (MODE & 2) {
      const uint4 z = buf[g % nbuf];
      g += 256 * 248;
      a = __builtin_bit_cast(b8, __builtin_bit_cast(uint4, a) ^ z);
    }
    c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c3, 0, 0, 0);
  }
  out[blockIdx.x * 256 + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3];
  unsigned long long r1;
  asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1)::"memory");
  if (threadIdx.x == 0) {
    st[2 * blockIdx.x] = r0;
    st[2 * blockIdx.x + 1] = r1;
  }
}

// an empty kernel with kp_attn3's launch shape (KP_MICRO_EMPTY=1): the dispatch cost alone
__global__ __launch_bounds__(256, 1) void kp_empty(int* sink) {
  extern __shared__ int lds_e[];
  if (threadIdx.x == 1023) sink[blockIdx.x] = lds_e[0];
}

// --streams: the merge's stand-in, one thread per four dimensions of a query sums the
// launch's `parts` O partials ([parts][nq][dp]) into out ([nq][dp])
__global__ void kp_micro_merge(const float* __restrict__ O, long long n4, int parts, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = 0; p < parts; ++p) {
    const float4 v = reinterpret_cast<const float4*>(O)[(size_t)p * n4 + i];
    a.x += v.x;
    a.y += v.y;
    a.z += v.z;
    a.w += v.w;
  }
  reinterpret_cast<float4*>(out)[i] = a;
}

struct MicroOpt {
  int ranges = 0, inflight = 1, streams = 0;
};

template <int DB, int MODE>
static int run(int n_ent, int nq, int iters, float scale, int part, MicroOpt opt) {
  constexpr int DP = 16 * DB;
  kp_ctx c;
  KP_HIP(hipStreamCreate(&c.stream));
  hipDeviceProp_t prop;
  KP_HIP(hipGetDeviceProperties(&prop, 0));
  c.n_cu = prop.multiProcessorCount;
  c.n_ent = n_ent;
  c.dp = DP;
  c.attn_mode = 1;
  c.attn_part = part;
  c.attn_ranges = opt.ranges;
  c.attn_inflight = opt.inflight;
  std::mt19937 gen(1234);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> E((size_t)n_ent * DP, 0.f), Q((size_t)nq * DP, 0.f), qs(nq);
  for (int e = 0; e < n_ent; ++e)
    for (int d = 0; d < DP; ++d) E[(size_t)e * DP + d] = scale * nd(gen);
  for (int q = 0; q < nq; ++q) {
    for (int d = 0; d < DP; ++d) Q[(size_t)q * DP + d] = scale * nd(gen);
    qs[q] = 1.0f / (float)n_ent;
  }
  KP_HIP(hipMalloc(&c.dE, E.size() * 4));
  KP_HIP(hipMemcpy(c.dE, E.data(), E.size() * 4, hipMemcpyHostToDevice));
  float *dQ, *dqs;
  KP_HIP(hipMalloc(&dQ, Q.size() * 4));
  KP_HIP(hipMalloc(&dqs, nq * 4));
  KP_HIP(hipMemcpy(dQ, Q.data(), Q.size() * 4, hipMemcpyHostToDevice));
  KP_HIP(hipMemcpy(dqs, qs.data(), nq * 4, hipMemcpyHostToDevice));
  // KP_MICRO_ATTN5=1: the wave-pair kernel (kp_attn5.hpp) for the D = 400 softmax modes
  bool use5 = std::getenv("KP_MICRO_ATTN5") && std::atoi(std::getenv("KP_MICRO_ATTN5")) == 1;
#ifdef KP_MICRO_HAS_ATTN5
  use5 = use5 && DB == 25 && MODE != ATT_BCE_O;
  const int slots = c.n_cu * (use5 ? attn5_wpc(&c) : attn3_wpc<DB, MODE == ATT_BCE_O ? ATT_BCE_O : ATT_SOFTMAX_O>(&c));
#else
  use5 = false;
  const int slots = c.n_cu * attn3_wpc<DB, MODE == ATT_BCE_O ? ATT_BCE_O : ATT_SOFTMAX_O>(&c);
#endif
  const AttnPlan plan = attn_plan_ctx(&c, nq, n_ent, slots, true);
  const int parts = plan.wk.n_parts;
  float *dm, *dl, *dO;
  KP_HIP(hipMalloc(&dm, (size_t)parts * nq * 4));
  KP_HIP(hipMalloc(&dl, (size_t)parts * nq * 4));
  KP_HIP(hipMalloc(&dO, (size_t)parts * nq * DP * 4));
  const float ylo = 0.05f;
  // KP_MICRO_ATTN4=1: the pipelined kernel (kp_attn4.hpp) where it exists
  const bool use4 = std::getenv("KP_MICRO_ATTN4") && std::atoi(std::getenv("KP_MICRO_ATTN4")) == 1;
  // KP_MICRO_ATTN6=1: the pair-shared O phase (kp_attn6.hpp) for the D = 400 softmax step
  const bool use6 = std::getenv("KP_MICRO_ATTN6") && std::atoi(std::getenv("KP_MICRO_ATTN6")) == 1;
  auto launch = [&]() {
#ifdef KP_MICRO_HAS_ATTN6
    if constexpr (DB == 25 && MODE == ATT_SOFTMAX_O) {
      if (use6) {
        launch_attn6<DB>(&c, n_ent, dQ, nq, plan, dm, dl, dO);
        return;
      }
    }
#endif
    (void)use6;
#ifdef KP_MICRO_HAS_ATTN4
    if constexpr (attn4_supported(DB) && MODE == ATT_SOFTMAX_O) {
      if (use4) {
        launch_attn4<DB>(&c, n_ent, dQ, nq, plan, dm, dl, dO);
        return;
      }
    }
#endif
    (void)use4;
#ifdef KP_MICRO_HAS_ATTN5
    if constexpr (DB == 25 && MODE != ATT_BCE_O) {
      if (use5) {
        launch_attn5<MODE>(&c, n_ent, dQ, nq, plan, dm, dl, dO);
        return;
      }
    }
#endif
    launch_attn3<DB, MODE>(&c, n_ent, dQ, nq, plan, dm, dl, dO, dqs, ylo);
  };
  if (std::getenv("KP_MICRO_RTCAL")) {
    unsigned long long* dout;
    KP_HIP(hipMalloc(&dout, 16));
    for (unsigned long long ticks : {1000000ull, 10000000ull}) {
      hipEvent_t a, b;
      KP_HIP(hipEventCreate(&a));
      KP_HIP(hipEventCreate(&b));
      KP_HIP(hipEventRecord(a, c.stream));
      hipLaunchKernelGGL(kp_rtcal, dim3(1), dim3(64), 0, c.stream, ticks, dout);
      KP_HIP(hipEventRecord(b, c.stream));
      KP_HIP(hipEventSynchronize(b));
      float ems = 0.f;
      KP_HIP(hipEventElapsedTime(&ems, a, b));
      unsigned long long h[2];
      KP_HIP(hipMemcpy(h, dout, 16, hipMemcpyDeviceToHost));
      printf("{\"rtcal_ticks\": %llu, \"memtime_ticks\": %llu, \"event_ms\": %.4f, \"realtime_mhz\": %.3f, "
             "\"idle_wave_clock_ghz\": %.4f}\n", h[0], h[1], ems, h[0] / (ems * 1e3), h[1] / (ems * 1e6));
    }
  }
  if (std::getenv("KP_MICRO_MFMA")) {
    float* dout;
    unsigned long long* dst;
    KP_HIP(hipMalloc(&dout, 4 * 256 * 256));
    KP_HIP(hipMalloc(&dst, 16 * 256));
    for (int it : {4000, 8000, 16000}) {
      for (int w = 0; w < 20; ++w) hipLaunchKernelGGL(kp_mfma_spin, dim3(256), dim3(256), 0, c.stream, it, dout, dst);
      hipEvent_t a, b;
      KP_HIP(hipEventCreate(&a));
      KP_HIP(hipEventCreate(&b));
      KP_HIP(hipEventRecord(a, c.stream));
      for (int i = 0; i < 30; ++i) hipLaunchKernelGGL(kp_mfma_spin, dim3(256), dim3(256), 0, c.stream, it, dout, dst);
      KP_HIP(hipEventRecord(b, c.stream));
      KP_HIP(hipEventSynchronize(b));
      float ems = 0.f;
      KP_HIP(hipEventElapsedTime(&ems, a, b));
      std::vector<unsigned long long> h(512);
      KP_HIP(hipMemcpy(h.data(), dst, 16 * 256, hipMemcpyDeviceToHost));
      unsigned long long t0 = ~0ull, t1 = 0;
      for (int i = 0; i < 256; ++i) {
        t0 = std::min(t0, h[2 * i]);
        t1 = std::max(t1, h[2 * i + 1]);
      }
      printf("{\"mfma_spin_iters\": %d, \"us_per_launch\": %.1f, \"wg_span_us\": %.1f}\n", it, 1e3 * ems / 30,
             (t1 - t0) * 0.01);
    }
  }
  if (std::getenv("KP_MICRO_MFMA2")) {
    float* dout;
    unsigned long long* dst;
    uint4* dbuf;
    const long long nbuf = 35LL * 1024 * 1024 / 16;
    KP_HIP(hipMalloc(&dout, 4 * 256 * 256));
    KP_HIP(hipMalloc(&dst, 16 * 256));
    KP_HIP(hipMalloc(&dbuf, 16 * nbuf));
    KP_HIP(hipMemset(dbuf, 1, 16 * nbuf));
    for (int mode = 0; mode < 4; ++mode) {
      auto go = [&](int it) {
        if (mode == 0) hipLaunchKernelGGL(kp_mfma_spin2<0>, dim3(248), dim3(256), 155648, c.stream, it, dbuf, nbuf, dout, dst);
        if (mode == 1) hipLaunchKernelGGL(kp_mfma_spin2<1>, dim3(248), dim3(256), 155648, c.stream, it, dbuf, nbuf, dout, dst);
        if (mode == 2) hipLaunchKernelGGL(kp_mfma_spin2<2>, dim3(248), dim3(256), 155648, c.stream, it, dbuf, nbuf, dout, dst);
        if (mode == 3) hipLaunchKernelGGL(kp_mfma_spin2<3>, dim3(248), dim3(256), 155648, c.stream, it, dbuf, nbuf, dout, dst);
      };
      const int it = 8000;
      for (int w = 0; w < 20; ++w) go(it);
      hipEvent_t a, b;
      KP_HIP(hipEventCreate(&a));
      KP_HIP(hipEventCreate(&b));
      KP_HIP(hipEventRecord(a, c.stream));
      for (int i = 0; i < 30; ++i) go(it);
      KP_HIP(hipEventRecord(b, c.stream));
      KP_HIP(hipEventSynchronize(b));
      float ems = 0.f;
      KP_HIP(hipEventElapsedTime(&ems, a, b));
      std::vector<unsigned long long> h(512);
      KP_HIP(hipMemcpy(h.data(), dst, 16 * 248, hipMemcpyDeviceToHost));
      unsigned long long t0 = ~0ull, t1 = 0;
      for (int i = 0; i < 248; ++i) {
        t0 = std::min(t0, h[2 * i]);
        t1 = std::max(t1, h[2 * i + 1]);
      }
      printf("{\"mfma_spin2_mode\": %d, \"iters\": %d, \"us_per_launch\": %.1f, \"wg_span_us\": %.1f}\n", mode, it,
             1e3 * ems / 30, (t1 - t0) * 0.01);
    }
  }
  if (std::getenv("KP_MICRO_EMPTY")) {
    int* sink;
    KP_HIP(hipMalloc(&sink, 4 * 4096));
    for (int rep = 0; rep < 2; ++rep) {
      hipEvent_t a, b;
      KP_HIP(hipEventCreate(&a));
      KP_HIP(hipEventCreate(&b));
      KP_HIP(hipEventRecord(a, c.stream));
      for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(kp_empty, dim3(plan.n_wg), dim3(256), attn3_lds_bytes(DB), c.stream, sink);
      KP_HIP(hipEventRecord(b, c.stream));
      KP_HIP(hipEventSynchronize(b));
      float ems = 0.f;
      KP_HIP(hipEventElapsedTime(&ems, a, b));
      printf("{\"empty_kernel_us_per_launch\": %.2f, \"n_wg\": %d, \"lds\": %zu}\n", 1e3 * ems / iters, plan.n_wg,
             attn3_lds_bytes(DB));
    }
  }
  launch();
  KP_HIP(hipStreamSynchronize(c.stream));
  float ms = 0.f;
  if (opt.streams > 0) {
    // K contexts as the pipeline has them: own stream, own image of the table, own partials
    const int K = opt.streams;
    const long long n4 = (long long)nq * DP / 4;
    std::vector<kp_ctx> cs(K);
    std::vector<float*> sm(K), sl(K), sO(K), sout(K);
    for (int k = 0; k < K; ++k) {
      KP_HIP(hipStreamCreateWithFlags(&cs[k].stream, hipStreamNonBlocking));
      cs[k].n_cu = c.n_cu;
      cs[k].n_ent = n_ent;
      cs[k].dp = DP;
      cs[k].attn_mode = 1;
      cs[k].dE = c.dE;
      KP_HIP(hipMalloc(&sm[k], (size_t)parts * nq * 4));
      KP_HIP(hipMalloc(&sl[k], (size_t)parts * nq * 4));
      KP_HIP(hipMalloc(&sO[k], (size_t)parts * nq * DP * 4));
      KP_HIP(hipMalloc(&sout[k], (size_t)nq * DP * 4));
    }
    auto round = [&]() {
      for (int k = 0; k < K; ++k) {
        launch_attn3<DB, MODE>(&cs[k], n_ent, dQ, nq, plan, sm[k], sl[k], sO[k], dqs, ylo);
        hipLaunchKernelGGL(kp_micro_merge, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, cs[k].stream, sO[k], n4,
                           parts, sout[k]);
      }
    };
    auto sync_all = [&]() {
      for (int k = 0; k < K; ++k) KP_HIP(hipStreamSynchronize(cs[k].stream));
    };
    {
      const auto w0 = std::chrono::steady_clock::now();
      while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 1.0) {
        for (int i = 0; i < 10; ++i) round();
        sync_all();
      }
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters; ++i) round();
    sync_all();
    ms = (float)(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / ((double)iters * K));
    // the checked and hashed outputs below: stream 0's partials
    KP_HIP(hipMemcpy(dm, sm[0], (size_t)parts * nq * 4, hipMemcpyDeviceToDevice));
    KP_HIP(hipMemcpy(dl, sl[0], (size_t)parts * nq * 4, hipMemcpyDeviceToDevice));
    KP_HIP(hipMemcpy(dO, sO[0], (size_t)parts * nq * DP * 4, hipMemcpyDeviceToDevice));
  } else {
    hipEvent_t e0, e1;
    KP_HIP(hipEventCreate(&e0));
    KP_HIP(hipEventCreate(&e1));
    // >= 1 s of back-to-back launches first: the first ~10 ms of work after the GPU leaves
    // idle run below the settled clock (profiles/r03zx_attn_warm_vs_spans.jsonl)
    {
      const auto w0 = std::chrono::steady_clock::now();
      while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < 1.0) {
        for (int i = 0; i < 20; ++i) launch();
        KP_HIP(hipStreamSynchronize(c.stream));
      }
    }
    KP_HIP(hipEventRecord(e0, c.stream));
    for (int i = 0; i < iters; ++i) launch();
    KP_HIP(hipEventRecord(e1, c.stream));
    KP_HIP(hipEventSynchronize(e1));
    KP_HIP(hipEventElapsedTime(&ms, e0, e1));
    ms /= iters;
  }
  std::vector<float> hm((size_t)parts * nq), hl((size_t)parts * nq), hO((size_t)parts * nq * DP);
  if (MODE != ATT_BCE_O) {
    KP_HIP(hipMemcpy(hm.data(), dm, hm.size() * 4, hipMemcpyDeviceToHost));
    KP_HIP(hipMemcpy(hl.data(), dl, hl.size() * 4, hipMemcpyDeviceToHost));
  }
  KP_HIP(hipMemcpy(hO.data(), dO, hO.size() * 4, hipMemcpyDeviceToHost));
  // fp64 check of 16 sampled queries
  double err_l = 0, err_o = 0;
  for (int k = 0; k < 16; ++k) {
    const int q = (int)((long long)k * 7919 % nq);
    std::vector<double> s(n_ent);
    double M = -1e300;
    for (int e = 0; e < n_ent; ++e) {
      double a = 0;
      for (int d = 0; d < DP; ++d) a += (double)Q[(size_t)q * DP + d] * E[(size_t)e * DP + d];
      s[e] = a;
      M = std::max(M, a);
    }
    std::vector<double> O(DP, 0.0);
    double L = 0;
    double onorm = 0;
    for (int e = 0; e < n_ent; ++e) {
      double w;
      if (MODE == ATT_BCE_O) {
        const double p = 1.0 / (1.0 + std::exp(-s[e]));
        const double w0 = (1 - p) * p;
        w = ((p - ylo) / std::max(w0, 1e-12) * qs[q]) * w0;
      } else {
        w = std::exp(s[e] - M);
      }
      L += w;
      for (int d = 0; d < DP; ++d) O[d] += w * E[(size_t)e * DP + d];
    }
    for (int d = 0; d < DP; ++d) onorm = std::max(onorm, std::fabs(O[d]));
    // merge the GPU partials
    double gM = -1e300;
    if (MODE != ATT_BCE_O)
      for (int p = 0; p < parts; ++p) gM = std::max(gM, (double)hm[(size_t)p * nq + q]);
    double gL = 0;
    std::vector<double> gO(DP, 0.0);
    for (int p = 0; p < parts; ++p) {
      const double f = MODE == ATT_BCE_O ? 1.0 : std::exp((double)hm[(size_t)p * nq + q] - gM);
      if (MODE != ATT_BCE_O) gL += f * hl[(size_t)p * nq + q];
      for (int d = 0; d < DP; ++d) gO[d] += f * hO[((size_t)p * nq + q) * DP + d];
    }
    if (MODE != ATT_BCE_O) {
      const double sc = std::exp(gM - M);  // GPU stats relative to its own max
      err_l = std::max(err_l, std::fabs(gL * sc - L) / L);
      for (int d = 0; d < DP; ++d) err_o = std::max(err_o, std::fabs(gO[d] * sc - O[d]) / onorm);
    } else {
      for (int d = 0; d < DP; ++d) err_o = std::max(err_o, std::fabs(gO[d] - O[d]) / onorm);
    }
  }
  // FNV-1a over the output bits: variants meant to be bitwise identical print the same hash
  unsigned long long bits = 1469598103934665603ull;
  auto fnv = [&](const std::vector<float>& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * 4; ++i) bits = (bits ^ p[i]) * 1099511628211ull;
  };
  if (MODE != ATT_BCE_O) {
    fnv(hm);
    fnv(hl);
  }
  fnv(hO);
  const double flops = (MODE == ATT_SOFTMAX ? 2.0 : 4.0) * DP * (double)nq * n_ent;
#ifdef KP_ATTN3_STAMPS
  {
    // one more launch with zeroed counters: cycles per (wave, tile) of each phase
    unsigned long long z[8] = {0}, st[8];
    KP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_attn3_stamps), z, sizeof(z)));
    launch();
    KP_HIP(hipStreamSynchronize(c.stream));
    KP_HIP(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_attn3_stamps), sizeof(st)));
    const double n = (double)(st[4] ? st[4] : 1);
    printf("{\"stamps\": {\"S\": %.0f, \"softmax\": %.0f, \"O\": %.0f, \"tile_end\": %.0f, \"wave_tiles\": %llu}}\n",
           st[0] / n, st[1] / n, st[2] / n, st[3] / n, st[4]);
  }
#endif
#ifdef KP_ATTN3_CLOCK
  {
    // >= 2 s of back-to-back launches on the random inputs, then one stamped launch:
    // median over workgroups of the in-kernel clock = d(memtime) / d(realtime) x 100 MHz
    const int warm = std::max(1, (int)(2000.0 / std::max(ms, 1e-3f)));
    for (int i = 0; i < warm; ++i) launch();
    KP_HIP(hipStreamSynchronize(c.stream));
    {
      // the per-launch time again, now with the clock settled (the first timing above
      // starts a few launches after the GPU left idle)
      hipEvent_t a, b;
      KP_HIP(hipEventCreate(&a));
      KP_HIP(hipEventCreate(&b));
      KP_HIP(hipEventRecord(a, c.stream));
      for (int i = 0; i < iters; ++i) launch();
      KP_HIP(hipEventRecord(b, c.stream));
      KP_HIP(hipEventSynchronize(b));
      float wms = 0.f;
      KP_HIP(hipEventElapsedTime(&wms, a, b));
      printf("{\"ms_after_warmup\": %.5f, \"tflops_after_warmup\": %.2f}\n", wms / iters, flops / (wms / iters) / 1e9);
      launch();  // the stamped launch
      KP_HIP(hipStreamSynchronize(c.stream));
    }
    static unsigned long long ck[4096][4];
    KP_HIP(hipMemcpyFromSymbol(ck, HIP_SYMBOL(g_attn3_clock), sizeof(ck)));
    std::vector<double> f;
    for (int b = 0; b < std::min(plan.n_wg, 4096); ++b)
      if (ck[b][3] > ck[b][1]) f.push_back((double)(ck[b][2] - ck[b][0]) / (double)(ck[b][3] - ck[b][1]) * 0.1);
    std::sort(f.begin(), f.end());
    const double med = f.empty() ? 0.0 : f[f.size() / 2];
    // workgroup spans on the 100 MHz clock: when they start and end relative to the first
    // start, and how long each runs (the launch's ms covers all of it plus the launch)
    unsigned long long t0 = ~0ull, t1 = 0;
    std::vector<double> dur, st;
    for (int b = 0; b < std::min(plan.n_wg, 4096); ++b)
      if (ck[b][3] > ck[b][1]) {
        t0 = std::min(t0, ck[b][1]);
        t1 = std::max(t1, ck[b][3]);
        dur.push_back((ck[b][3] - ck[b][1]) * 0.01);
      }
    for (int b = 0; b < std::min(plan.n_wg, 4096); ++b)
      if (ck[b][3] > ck[b][1]) st.push_back((ck[b][1] - t0) * 0.01);
    std::sort(dur.begin(), dur.end());
    std::sort(st.begin(), st.end());
    if (!dur.empty())
      printf("{\"wg_us_min\": %.1f, \"wg_us_median\": %.1f, \"wg_us_max\": %.1f, \"start_spread_us\": %.1f, "
             "\"first_start_to_last_end_us\": %.1f}\n", dur.front(), dur[dur.size() / 2], dur.back(), st.back(),
             (t1 - t0) * 0.01);
    printf("{\"clock_ghz_median\": %.4f, \"clock_ghz_min\": %.4f, \"clock_ghz_max\": %.4f, \"workgroups\": %zu, "
           "\"warm_launches\": %d}\n", med, f.empty() ? 0.0 : f.front(), f.empty() ? 0.0 : f.back(), f.size(), warm);
  }
#endif
  printf("{\"kernel\": \"%s\", \"DB\": %d, \"mode\": %d, \"n_ent\": %d, \"nq\": %d, \"parts\": %d, \"ranges\": %d, \"n_wg\": %d, \"streams\": %d, "
         "\"ms\": %.5f, \"tflops\": %.2f, \"frac_bf16x6\": %.4f, \"err_l\": %.3e, \"err_o\": %.3e, \"bits\": \"%016llx\"}\n",
         use5 ? "kp_attn5" : "kp_attn3", DB, MODE, n_ent, nq, parts, plan.wk.ranges, plan.n_wg, opt.streams, ms, flops / ms / 1e9, flops / ms / 1e9 / 419.43,
         err_l, err_o, bits);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: attn_micro DB mode n_ent nq iters [scale] [part] [--ranges S] [--inflight N] [--streams K]\n");
    return 2;
  }
  const int DB = atoi(argv[1]), mode = atoi(argv[2]), n_ent = atoi(argv[3]), nq = atoi(argv[4]), iters = atoi(argv[5]);
  MicroOpt opt;
  int npos = argc;
  for (int i = 6; i < argc; ++i)
    if (argv[i][0] == '-' && argv[i][1] == '-') {
      npos = std::min(npos, i);
      const int v = i + 1 < argc ? atoi(argv[i + 1]) : 0;
      if (!strcmp(argv[i], "--ranges")) opt.ranges = std::max(0, std::min(16, v));
      else if (!strcmp(argv[i], "--inflight")) opt.inflight = std::max(1, v);
      else if (!strcmp(argv[i], "--streams")) opt.streams = std::max(0, std::min(8, v));
      else {
        fprintf(stderr, "unknown option %s\n", argv[i]);
        return 2;
      }
      ++i;
    }
  const float scale = npos > 6 ? (float)atof(argv[6]) : 0.05f;
  const int part = npos > 7 ? atoi(argv[7]) : 0;
  try {
    if (DB == 25 && mode == 0) return run<25, ATT_SOFTMAX_O>(n_ent, nq, iters, scale, part, opt);
    if (DB == 13 && mode == 2) return run<13, ATT_BCE_O>(n_ent, nq, iters, scale, part, opt);
    fprintf(stderr, "unsupported DB/mode\n");
    return 2;
  } catch (const KpError& e) {
    fprintf(stderr, "error: %s\n", e.msg.c_str());
    return 1;
  }
}
