// kp_batch_check.hpp -- the structural checks of a post-training batch that every model
// family needs, as one pure host function (no HIP: tests/native/batch_check_driver.cpp
// builds it alone under the host sanitizers).
#pragma once

#include <cstdint>

#include "../../include/kelpie_hip.h"

// nullptr when the batch is well formed for a model of n_ent frozen entities (the kelpie
// entity is id n_ent) and n_rel2 relations, else the rule it breaks.  Every id is checked
// here, before it indexes a host vector or a device table; each *_posttrain_rank calls
// this before its first upload or launch.  `dim` only has to be positive: x0 is
// [n_slots][dim] by contract and carries no length to check against.
inline const char* kp_check_batch(int n_ent, int n_rel2, int dim, const kp_batch* b) {
  if (n_ent <= 0 || n_rel2 <= 0 || dim <= 0) return "empty model";
  const int ns = b->n_slots;
  if (ns < 0) return "negative n_slots";
  if (b->row_off[0] != 0) return "bad row_off";
  for (int s = 0; s < ns; ++s) {
    if (b->row_off[s + 1] < b->row_off[s]) return "bad row_off";
    if (b->filt_off[s + 1] < b->filt_off[s]) return "bad filt_off";
  }
  if (b->filt_off[0] < 0) return "bad filt_off";
  for (int64_t i = 0; i < (int64_t)b->row_off[ns]; ++i) {
    const int32_t* rw = b->rows + 3 * i;
    if (rw[0] < 0 || rw[0] > n_ent || rw[2] < 0 || rw[2] > n_ent || rw[1] < 0 || rw[1] >= n_rel2)
      return "row id out of range";
  }
  for (int s = 0; s < ns; ++s) {
    const int32_t* p = b->pred + 3 * s;
    if (p[0] != n_ent) return "the ranked triple must start at the kelpie entity";
    if (p[1] < 0 || p[1] >= n_rel2) return "ranked relation out of range";
    if (p[2] < 0 || p[2] > n_ent) return "ranked object out of range";
  }
  // filt is uploaded whole, [0, filt_off[n_slots])
  for (int64_t i = 0; i < (int64_t)b->filt_off[ns]; ++i)
    if (b->filt[i] < 0 || b->filt[i] > n_ent) return "filter id out of range";
  return nullptr;
}
