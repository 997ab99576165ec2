// kp_keyed.hip -- keyed draws on the device (include/kelpie_hip.h, "Keyed draws"): the kernels
// that generate a batch's kelpie inits, epoch permutations, negatives and head-or-tail words
// from the slots' keys, straight into the buffers the step kernels read; kp_ctx_arm_keyed,
// kp_keyed_draws and kp_keyed_rng_words.  The definitions are kp_keyed.hpp's scalar functions.
// Every store is a plain vector store and every value depends on its own index alone: a rerun
// gives the same bits.
#include "kp_keyed.hpp"
#include "kp_posttrain.hpp"

namespace {

constexpr int KK_NT = 256;          // threads per workgroup, every kernel here (4 waves of 64)
constexpr int KK_PERM_LDS = 4096;   // (key word, row) pairs of the LDS network: 32 KiB
constexpr size_t KK_SCRATCH_BYTES = (size_t)64 << 20;  // the global network's scratch, at most

// kp_key_x0: the slots' initial rows [ns][dp], the zero padding [dim, dp) included.
//   uniform (ComplEx / DistMult): one thread per four elements (one Philox block), one float4 store
//   normal (TransE): one thread per element (its two words are lanes of one block)
template <bool NORMAL>
__global__ __launch_bounds__(KK_NT) void kp_key_x0(const uint64_t* __restrict__ init_key, int ns, int dim, int dp,
                                                    float scale, float* __restrict__ X) {
  const int per_row = NORMAL ? dp : dp / 4;
  const long long n = (long long)ns * per_row;
  for (long long g = (long long)blockIdx.x * KK_NT + threadIdx.x; g < n; g += (long long)gridDim.x * KK_NT) {
    const int s = (int)(g / per_row), j = (int)(g % per_row);
    const uint64_t key = init_key[s];
    if (NORMAL) {
      float v = 0.f;
      if (j < dim) {
        const KpPhilox4 w = kp_keyed_quad(key, KP_KS_X0, 0u, (uint32_t)j >> 1);
        v = kp_keyed_normal(w.v[(2 * j) & 3], w.v[((2 * j) & 3) + 1], scale);
      }
      X[(size_t)s * dp + j] = v;
    } else {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * j < dim) {
        const KpPhilox4 w = kp_keyed_quad(key, KP_KS_X0, 0u, (uint32_t)j);
        v.x = kp_keyed_uniform(w.v[0], scale);
        if (4 * j + 1 < dim) v.y = kp_keyed_uniform(w.v[1], scale);
        if (4 * j + 2 < dim) v.z = kp_keyed_uniform(w.v[2], scale);
        if (4 * j + 3 < dim) v.w = kp_keyed_uniform(w.v[3], scale);
      }
      *reinterpret_cast<float4*>(X + (size_t)s * dp + 4 * (size_t)j) = v;  // dp is a multiple of 16
    }
  }
}

// kp_key_words: TransE's negatives and head-or-tail words, elementwise: one thread per four
// rows of an epoch (one Philox block per stream).  blockIdx.y strides the slots.
__global__ __launch_bounds__(KK_NT) void kp_key_words(const uint64_t* __restrict__ slot_key, int ns, int epochs,
                                                       const int32_t* __restrict__ row_off,
                                                       const int64_t* __restrict__ rng_off, uint64_t neg_bound,
                                                       int32_t* __restrict__ out) {
  for (int s = blockIdx.y; s < ns; s += gridDim.y) {
    const int R = row_off[s + 1] - row_off[s];
    const long long QR = (R + 3) / 4, items = QR * epochs;
    const uint64_t key = slot_key[s];
    int32_t* o = out + rng_off[s];
    for (long long it = (long long)blockIdx.x * KK_NT + threadIdx.x; it < items; it += (long long)gridDim.x * KK_NT) {
      const uint32_t e = (uint32_t)(it / QR), q = (uint32_t)(it % QR);
      const KpPhilox4 wn = kp_keyed_quad(key, KP_KS_NEG, e, q), wh = kp_keyed_quad(key, KP_KS_HOT, e, q);
      int32_t* ep = o + (long long)e * 3 * R;
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const int i = 4 * (int)q + l;
        if (i < R) {
          ep[R + i] = kp_keyed_neg(wn.v[l], neg_bound);
          ep[2 * (long long)R + i] = kp_keyed_hot(wh.v[l]);
        }
      }
    }
  }
}

// kp_key_perm: the permutation of one (slot, epoch) per workgroup pass: a bitonic network over
// N = 2^k >= R sort keys (key word above row index, kp_keyed_sort_key: all distinct, so the
// network's ascending order IS the stable argsort; rows >= R pad it with 0xFFFFFFFF above the
// index and sort last).  GLOBAL = false: the keys live in LDS (N <= 4096, 32 KiB) as one
// 8-byte array read with ds_read_b64: a compare distance j >= 32 keys has each 32-lane group
// on 64 consecutive dwords (no bank conflict); the five shortest distances stride the lanes
// and pay a 2-way conflict.  GLOBAL = true: the same network over the workgroup's own span of
// a global scratch, workgroup barriers between stages (one workgroup owns a span: its waves
// share the CU's L1, so a workgroup-scope barrier orders the stages).
// Jobs: (list slot, epoch), job j = list[j / epochs], epoch j % epochs; a workgroup strides them.
// `per`: the epoch's words per row (TransE 3, ComplEx / DistMult 1); the permutation is the
// first R words of the epoch.
template <bool GLOBAL>
__global__ __launch_bounds__(KK_NT) void kp_key_perm(const uint64_t* __restrict__ slot_key,
                                                      const int32_t* __restrict__ list, int n_list, int epochs,
                                                      const int32_t* __restrict__ row_off,
                                                      const int64_t* __restrict__ rng_off, int per,
                                                      int32_t* __restrict__ out, uint64_t* __restrict__ scratch,
                                                      int n_max) {
  __shared__ uint64_t lds[GLOBAL ? 1 : KK_PERM_LDS];
  uint64_t* a = GLOBAL ? scratch + (size_t)blockIdx.x * n_max : lds;
  const int cap = GLOBAL ? n_max : KK_PERM_LDS;
  const int tid = threadIdx.x;
  const long long jobs = (long long)n_list * epochs;
  for (long long job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int s = list[job / epochs];
    const uint32_t e = (uint32_t)(job % epochs);
    const int R = row_off[s + 1] - row_off[s];
    int N = 1;
    while (N < R) N <<= 1;
    if (N > cap) continue;  // never: the host sorts the slots into the two launches by R
    const uint64_t key = slot_key[s];
    for (int q = tid; 4 * q < N; q += KK_NT) {
      KpPhilox4 w{{0u, 0u, 0u, 0u}};
      if (4 * q < R) w = kp_keyed_quad(key, KP_KS_PERM, e, (uint32_t)q);
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (4 * q + l < N) a[4 * q + l] = kp_keyed_sort_key(w.v[l], (uint32_t)(4 * q + l), (uint32_t)R);
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < N / 2; t += KK_NT) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // bit j clear
          const int l = i | j;
          const uint64_t x = a[i], y = a[l];
          if ((x > y) == ((i & k) == 0)) {
            a[i] = y;
            a[l] = x;
          }
        }
        __syncthreads();
      }
    }
    int32_t* o = out + rng_off[s] + (long long)e * per * R;
    for (int i = tid; i < R; i += KK_NT) o[i] = (int32_t)(uint32_t)a[i];
    __syncthreads();  // the next job refills a[]
  }
}

int grid_for(long long items, int cap) {
  return (int)std::max<long long>(1, std::min<long long>((items + KK_NT - 1) / KK_NT, cap));
}

}  // namespace

void keyed_x0_dev(kp_ctx* c, const kp_keyed* k, int ns, float* dX) {
  if (ns <= 0) return;
  const uint64_t* dKey = upload(c, c->kd.init_key, k->init_key, (size_t)ns);
  const bool normal = c->model == KP_MODEL_TRANSE;
  const long long items = (long long)ns * (normal ? c->dp : c->dp / 4);
  if (normal)
    hipLaunchKernelGGL(kp_key_x0<true>, dim3(grid_for(items, 2048)), dim3(KK_NT), 0, c->stream, dKey, ns, c->dim, c->dp,
                       k->x0_scale, dX);
  else
    hipLaunchKernelGGL(kp_key_x0<false>, dim3(grid_for(items, 2048)), dim3(KK_NT), 0, c->stream, dKey, ns, c->dim,
                       c->dp, k->x0_scale, dX);
  KP_HIP(hipGetLastError());
}

void keyed_rng_dev(kp_ctx* c, const kp_hp* hp, const kp_keyed* k, int ns, const int32_t* row_off,
                   const int64_t* rng_off, int32_t* dRng) {
  if (ns <= 0 || rng_off[ns] == 0) return;
  const bool te = c->model == KP_MODEL_TRANSE;
  const int E = hp->epochs;
  // the slots with words, by the network that sorts them; every buffer is sized here
  std::vector<int32_t> lds_slots, big_slots;
  int max_r = 0, max_big = 0;
  for (int s = 0; s < ns; ++s) {
    if (rng_off[s + 1] == rng_off[s]) continue;
    const int R = row_off[s + 1] - row_off[s];
    max_r = std::max(max_r, R);
    if (R <= KK_PERM_LDS) {
      lds_slots.push_back(s);
    } else {
      big_slots.push_back(s);
      max_big = std::max(max_big, R);
    }
  }
  const uint64_t* dKey = upload(c, c->kd.slot_key, k->slot_key, (size_t)ns);
  const int32_t* dRow = upload(c, c->kd.row_off, row_off, (size_t)ns + 1);
  const int64_t* dOff = upload(c, c->kd.rng_off, rng_off, (size_t)ns + 1);
  const int32_t* dLds = upload(c, c->kd.lds_slots, lds_slots.data(), lds_slots.size());
  const int32_t* dBig = upload(c, c->kd.big_slots, big_slots.data(), big_slots.size());
  const int per = te ? 3 : 1;
  if (!lds_slots.empty()) {
    const long long jobs = (long long)lds_slots.size() * E;
    hipLaunchKernelGGL(kp_key_perm<false>, dim3((unsigned)std::min<long long>(jobs, 1 << 20)), dim3(KK_NT), 0, c->stream,
                       dKey, dLds, (int)lds_slots.size(), E, dRow, dOff, per, dRng, (uint64_t*)nullptr, 0);
    KP_HIP(hipGetLastError());
  }
  if (!big_slots.empty()) {
    // one span of the scratch per workgroup; the workgroups stride the jobs
    long long n_max = 1;
    while (n_max < max_big) n_max <<= 1;
    const long long jobs = (long long)big_slots.size() * E;
    const long long wgs = std::max<long long>(
        1, std::min<long long>({jobs, 1024, (long long)(KK_SCRATCH_BYTES / (sizeof(uint64_t) * (size_t)n_max))}));
    uint64_t* scratch = ensure_n<uint64_t>(c->kd.scratch, (size_t)wgs * (size_t)n_max);
    hipLaunchKernelGGL(kp_key_perm<true>, dim3((unsigned)wgs), dim3(KK_NT), 0, c->stream, dKey, dBig,
                       (int)big_slots.size(), E, dRow, dOff, per, dRng, scratch, (int)n_max);
    KP_HIP(hipGetLastError());
  }
  if (te) {
    const long long items = (long long)((max_r + 3) / 4) * E;
    hipLaunchKernelGGL(kp_key_words, dim3(grid_for(items, 64), std::min(ns, 65535)), dim3(KK_NT), 0, c->stream, dKey, ns,
                       E, dRow, dOff, (uint64_t)k->neg_bound, dRng);
    KP_HIP(hipGetLastError());
  }
}

// kp_keyed_draws: generate into the keyed workspace's own buffers and download
void keyed_draws(kp_ctx* c, const kp_hp* hp, int ns, const int32_t* row_off, const kp_keyed* k, float* out_x0,
                 int64_t* out_rng_off, int32_t* out_rng, int64_t cap) {
  int code = KP_EINVAL;
  KP_REQUIRE(ns >= 0 && out_rng_off && cap >= 0, "kp_keyed_draws: bad arguments");
  if (const char* why = kp_check_keyed(c->model, hp, ns, row_off, k, &code))
    throw KpError{code, std::string("kp_keyed_draws: ") + why};
  std::vector<int64_t> words((size_t)ns + 1);
  (void)kp_keyed_words_host(c->model, hp, ns, row_off, words.data(), out_rng_off);
  const int64_t total = out_rng_off[ns];
  KP_REQUIRE(total <= cap && (total == 0 || out_rng), "kp_keyed_draws: out_rng is too small");
  if (ns == 0) return;
  if (out_x0) {
    float* dX = ensure_n<float>(c->kd.x, (size_t)ns * c->dp);
    keyed_x0_dev(c, k, ns, dX);
    KP_HIP(hipMemcpy2DAsync(out_x0, sizeof(float) * c->dim, dX, sizeof(float) * c->dp, sizeof(float) * c->dim, ns,
                            hipMemcpyDeviceToHost, c->stream));
  }
  if (total > 0) {
    int32_t* dRng = ensure_n<int32_t>(c->kd.rng, (size_t)total);
    keyed_rng_dev(c, hp, k, ns, row_off, out_rng_off, dRng);
    KP_HIP(hipMemcpyAsync(out_rng, dRng, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
  }
  KP_HIP(hipStreamSynchronize(c->stream));
}
