// kp_attrib_check.hpp -- the attributions' request check (include/kelpie_hip.h,
// "Attributions").  Pure host code: tests/native/attrib_driver.cpp builds this header alone
// (`make attrib attrib_asan`).
#pragma once

#include <cstdint>

#include "../../include/kelpie_hip.h"

// The check of an attributions request, after the margins check and before any upload: nullptr,
// or the first rule broken, with *code KP_EINVAL or KP_ENOTSUP.  `pred` [n_slots][3] are the
// kelpie-form triples the slots rank (the kelpie entity is n_ent).
inline const char* kp_check_attrib(int model, const kp_hp* hp, int n_ent, int n_slots, const int32_t* row_off,
                                   const int32_t* pred, const kp_attrib* a, int* code) {
  *code = KP_EINVAL;
  if (!a) return "missing request";
  const int rows = n_slots > 0 ? row_off[n_slots] : 0;
  if (rows > 0 && (!a->out_fit || !a->out_reg)) return "missing out_fit or out_reg";
  if (n_slots > 0 && !a->out_delta) return "missing out_delta";
  *code = KP_ENOTSUP;
  if (model != KP_MODEL_COMPLEX && model != KP_MODEL_DISTMULT)
    return "attributions serve ComplEx and DistMult only (the score must be linear in the row)";
  if (hp->optimizer == KP_OPT_ADAM) return "attributions are not offered with Adam (Adagrad and SGD only)";
  for (int s = 0; s < n_slots; ++s)
    if (pred[3 * (size_t)s + 2] == n_ent)
      return "the tail of a slot's pred is the kelpie entity (its score is quadratic in the row)";
  return nullptr;
}
