// kp_probe_check.hpp -- the structural checks of a batch's probes (kp_probes), as one pure
// host function (no HIP: tests/native/probe_check_driver.cpp builds it alone under the
// host sanitizers), the slots' and the probes' expansion into rank rows and the chunking of
// rank rows.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/kelpie_hip.h"

// nullptr when the probes are well formed for a batch of n_slots slots on a model of n_ent
// frozen entities (the kelpie entity is id n_ent) and n_rel2 relations, else the rule they
// break.  Every offset and id is checked here, before it indexes a host vector or a device
// table; each *_posttrain_rank calls this after its batch check and before its first upload.
inline const char* kp_check_probes(int n_ent, int n_rel2, int n_slots, const kp_probes* p) {
  if (n_ent <= 0 || n_rel2 <= 0) return "empty model";
  if (n_slots < 0) return "negative n_slots";
  const int n = p->n;
  if (n < 0) return "negative probe count";
  if (!p->probe_off) return "missing probe_off";
  if (p->probe_off[0] != 0) return "probe_off must start at 0";
  for (int s = 0; s < n_slots; ++s)
    if (p->probe_off[s + 1] < p->probe_off[s]) return "probe_off decreases";
  if (p->probe_off[n_slots] != n) return "probe_off must end at the probe count";
  if (n == 0) return nullptr;
  if (!p->probes) return "missing probes";
  if (!p->filt_off) return "missing filt_off";
  if (!p->out_score || !p->out_rank) return "missing probe output";
  for (int i = 0; i < n; ++i) {
    const int32_t* t = p->probes + 2 * (size_t)i;
    if (t[0] < 0 || t[0] >= n_rel2) return "probe relation out of range";
    if (t[1] < 0 || t[1] > n_ent) return "probe object out of range";
  }
  if (p->filt_off[0] != 0) return "filt_off must start at 0";
  for (int i = 0; i < n; ++i)
    if (p->filt_off[i + 1] < p->filt_off[i]) return "filt_off decreases";
  if (p->filt_off[n] > 0 && !p->filt) return "missing filt";
  // filt is uploaded whole, [0, filt_off[n])
  for (int64_t i = 0; i < (int64_t)p->filt_off[n]; ++i)
    if (p->filt[i] < 0 || p->filt[i] > n_ent) return "probe filter id out of range";
  return nullptr;
}

// A batch's slots as rank rows (kp_common.hpp's RankSet): row s is trip[3 s ..] = (s, p, o) of
// the slot's ranked triple pred[3 s ..] = (kelpie, p, o), po[s] its object.  The batch's filter
// CSR is already one list per row.
inline void kp_slot_rows(int n_slots, const int32_t* pred, std::vector<int32_t>& trip, std::vector<int32_t>& po) {
  trip.assign((size_t)std::max(0, n_slots) * 3, 0);
  po.assign((size_t)std::max(0, n_slots), 0);
  for (int s = 0; s < n_slots; ++s) {
    trip[3 * (size_t)s] = s;
    trip[3 * (size_t)s + 1] = pred[3 * (size_t)s + 1];
    trip[3 * (size_t)s + 2] = po[s] = pred[3 * (size_t)s + 2];
  }
}

// The probes kp_check_probes accepted as rank rows: row i is trip[3 i ..] = (slot, p, o) of
// probe i, po[i] its object.  The probes' filter CSR is already one list per row.
inline void kp_probe_rows(int n_slots, const kp_probes* p, std::vector<int32_t>& trip, std::vector<int32_t>& po) {
  trip.assign((size_t)p->n * 3, 0);
  po.assign((size_t)p->n, 0);
  for (int s = 0; s < n_slots; ++s)
    for (int i = p->probe_off[s]; i < p->probe_off[s + 1]; ++i) {
      trip[3 * (size_t)i] = s;
      trip[3 * (size_t)i + 1] = p->probes[2 * (size_t)i];
      trip[3 * (size_t)i + 2] = po[i] = p->probes[2 * (size_t)i + 1];
    }
}

// Rank rows per chunk (the probes', the mark rows'): whole rows of `row_bytes` (the fp64 query row, the filter bitmap and
// whatever else the model holds per row) within `budget` bytes, a multiple of `group` rows
// when more than one group fits, at least one row and at most n.  `forced` > 0
// (KP_PROBE_CHUNK, KP_MARKS_CHUNK) overrides the budget.
inline int kp_probe_chunk(int n, size_t row_bytes, size_t budget, int group, int forced) {
  if (n <= 0) return 0;
  if (forced > 0) return std::min(n, forced);
  size_t rows = std::max<size_t>(1, budget / std::max<size_t>(1, row_bytes));
  if (group > 1 && rows >= (size_t)group) rows -= rows % (size_t)group;
  return (int)std::min<size_t>((size_t)n, rows);
}
