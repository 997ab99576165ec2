// kp_keyed.hpp -- keyed draws (include/kelpie_hip.h, "Keyed draws"): the counter-based
// generator, the counter layout, the streams' scalar definitions, the per-slot word counts and
// the request check, as pure host functions (no HIP: tests/native/keyed_driver.cpp builds this
// header alone under the host sanitizers).  The generation kernels of kp_keyed.hip call the
// same scalar functions (KP_HD), so the device and the native driver state one definition.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/kelpie_hip.h"

#if defined(__HIPCC__)
#define KP_HD __host__ __device__ inline
#else
#define KP_HD inline
#endif

// the streams of a key (counter word 2)
enum { KP_KS_X0 = 0, KP_KS_PERM = 1, KP_KS_NEG = 2, KP_KS_HOT = 3 };

struct KpPhilox4 {
  uint32_t v[4];
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
KP_HD KpPhilox4 kp_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return KpPhilox4{{c0, c1, c2, c3}};
}

// the four words [4 q, 4 q + 4) of stream `stream`, epoch `epoch`, under `key`
KP_HD KpPhilox4 kp_keyed_quad(uint64_t key, uint32_t stream, uint32_t epoch, uint32_t q) {
  return kp_philox4x32_10(q, epoch, stream, 0u, (uint32_t)key, (uint32_t)(key >> 32));
}

// word w of the stream
KP_HD uint32_t kp_keyed_word(uint64_t key, uint32_t stream, uint32_t epoch, uint32_t w) {
  return kp_keyed_quad(key, stream, epoch, w >> 2).v[w & 3];
}

// stream 0, ComplEx / DistMult: kelpie_init's one float32 multiply of a [0, 1) uniform
KP_HD float kp_keyed_uniform(uint32_t word, float init_scale) {
  return ((float)(word >> 8) * 5.9604644775390625e-8f) * init_scale;  // 2^-24
}

// stream 0, TransE: Box-Muller in float64 on the element's two words, rounded once
KP_HD float kp_keyed_normal(uint32_t w0, uint32_t w1, float std_) {
  const double u1 = ((double)w0 + 1.0) * 2.3283064365386962890625e-10;  // 2^-32
  const double u2 = (double)w1 * 2.3283064365386962890625e-10;
  const double r = sqrt(-2.0 * log(u1));
  const double c = cos(6.283185307179586476925286766559 * u2);
  return (float)(((double)std_ * r) * c);
}

// stream 2: the negative entity below `n`; stream 3: head (1) or tail (0), as kp_batch.rng holds them
KP_HD int32_t kp_keyed_neg(uint32_t word, uint64_t n) { return (int32_t)(((uint64_t)word * n) >> 32); }
KP_HD int32_t kp_keyed_hot(uint32_t word) { return (int32_t)(word >> 31); }

// stream 1: the sort key of row i, key word above row index: ascending order of these is the
// stable ascending argsort of the key words.  Rows at or past R pad a sorting network's input
// and sort behind every row.
KP_HD uint64_t kp_keyed_sort_key(uint32_t word, uint32_t i, uint32_t R) {
  return ((uint64_t)(i < R ? word : 0xFFFFFFFFu) << 32) | i;
}

// ---- host only -------------------------------------------------------------------------

inline bool kp_keyed_family(int model) {
  return model == KP_MODEL_TRANSE || model == KP_MODEL_COMPLEX || model == KP_MODEL_DISTMULT;
}

// The words of every slot (kp_batch.rng's layout): TransE epochs x 3 R; ComplEx / DistMult
// epochs x R for a slot of more than one step per epoch (R > batch_size), none otherwise.
// out[s] for s < n_slots; off (may be null) [n_slots + 1] their prefix sums.  nullptr, or the
// rule broken.
inline const char* kp_keyed_words_host(int model, const kp_hp* hp, int n_slots, const int32_t* row_off,
                                       int64_t* out, int64_t* off) {
  if (!kp_keyed_family(model)) return "keyed draws serve TransE, ComplEx and DistMult";
  if (!hp) return "missing hyper-parameters";
  if (hp->epochs < 0) return "negative epochs";
  if (hp->batch_size <= 0) return "batch_size must be positive";
  if (n_slots < 0) return "negative n_slots";
  if (n_slots > 0 && !row_off) return "missing row_off";
  if (n_slots > 0 && row_off[0] != 0) return "bad row_off";
  int64_t total = 0;
  if (off) off[0] = 0;
  for (int s = 0; s < n_slots; ++s) {
    const int64_t R = (int64_t)row_off[s + 1] - row_off[s];
    if (R < 0) return "bad row_off";
    // epochs < 2^31, R < 2^31: each factor pair is below 2^62, the triple product may not be
    int64_t per = 0;
    if (model == KP_MODEL_TRANSE)
      per = 3 * R;
    else if (R > hp->batch_size)
      per = R;
    if (per != 0 && (int64_t)hp->epochs > INT64_MAX / per) return "word count beyond int64";
    const int64_t w = per * hp->epochs;
    if (w > INT64_MAX - total) return "word count beyond int64";
    total += w;
    if (out) out[s] = w;
    if (off) off[s + 1] = total;
  }
  return nullptr;
}

// The request check of an armed call, after the batch check and before any device work:
// keys present, n_slots that of the batch, the family, the scale and the bound, the word
// counts within int64.  *code is KP_ENOTSUP for a family without keyed draws, else KP_EINVAL.
inline const char* kp_check_keyed(int model, const kp_hp* hp, int n_slots, const int32_t* row_off,
                                  const kp_keyed* k, int* code) {
  *code = KP_EINVAL;
  if (!k) return "missing request";
  if (!kp_keyed_family(model)) {
    *code = KP_ENOTSUP;
    return "keyed draws serve TransE, ComplEx and DistMult";
  }
  if (k->n_slots != n_slots) return "n_slots differs from the batch's";
  if (n_slots > 0 && (!k->init_key || !k->slot_key)) return "missing keys";
  if (!(k->x0_scale == k->x0_scale)) return "x0_scale is not a number";
  if (model == KP_MODEL_TRANSE && (k->neg_bound < 1 || k->neg_bound > ((int64_t)1 << 31)))
    return "neg_bound must be in [1, 2^31]";
  return kp_keyed_words_host(model, hp, n_slots, row_off, nullptr, nullptr);
}

// the stable ascending argsort of epoch e's key words of a slot of R rows
inline void kp_keyed_perm_host(uint64_t slot_key, uint32_t epoch, int32_t R, int32_t* out) {
  std::vector<uint64_t> a((size_t)R);
  for (int32_t i = 0; i < R; ++i)
    a[i] = kp_keyed_sort_key(kp_keyed_word(slot_key, KP_KS_PERM, epoch, (uint32_t)i), (uint32_t)i, (uint32_t)R);
  std::sort(a.begin(), a.end());
  for (int32_t i = 0; i < R; ++i) out[i] = (int32_t)(uint32_t)a[i];
}

// one slot's words, by the scalar definitions (what the kernels of kp_keyed.hip generate);
// `out` holds kp_keyed_words_host's count for the slot
inline void kp_keyed_slot_host(int model, const kp_hp* hp, int32_t R, uint64_t slot_key, int64_t neg_bound,
                               int32_t* out) {
  const bool te = model == KP_MODEL_TRANSE;
  if (!te && R <= hp->batch_size) return;
  for (int e = 0; e < hp->epochs; ++e) {
    int32_t* ep = out + (int64_t)e * (te ? 3 : 1) * R;
    kp_keyed_perm_host(slot_key, (uint32_t)e, R, ep);
    if (!te) continue;
    for (int32_t i = 0; i < R; ++i) {
      ep[R + i] = kp_keyed_neg(kp_keyed_word(slot_key, KP_KS_NEG, (uint32_t)e, (uint32_t)i), (uint64_t)neg_bound);
      ep[2 * (int64_t)R + i] = kp_keyed_hot(kp_keyed_word(slot_key, KP_KS_HOT, (uint32_t)e, (uint32_t)i));
    }
  }
}

// one slot's initial row [dim]
inline void kp_keyed_x0_host(int model, int dim, uint64_t init_key, float x0_scale, float* out) {
  for (int i = 0; i < dim; ++i) {
    if (model == KP_MODEL_TRANSE)
      out[i] = kp_keyed_normal(kp_keyed_word(init_key, KP_KS_X0, 0, 2u * i), kp_keyed_word(init_key, KP_KS_X0, 0, 2u * i + 1),
                               x0_scale);
    else
      out[i] = kp_keyed_uniform(kp_keyed_word(init_key, KP_KS_X0, 0, (uint32_t)i), x0_scale);
  }
}
