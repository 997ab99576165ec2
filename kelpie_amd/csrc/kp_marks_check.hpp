// kp_marks_check.hpp -- the epoch marks of kp_posttrain_rank_marks (include/kelpie_hip.h,
// "Epoch marks"): the structural check of a call's kp_marks, the mark plan and the marks'
// expansion into rank rows, as pure host functions (no HIP: tests/native/marks_check_driver.cpp builds this header alone under the
// host sanitizers).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/kelpie_hip.h"
#include "kp_trace_check.hpp"

constexpr int KP_MARKS_MAX = 16;

// nullptr when `m` is a well-formed marks request for a call of hp->epochs epochs, else the
// rule it breaks: 1 <= n <= 16 epochs, strictly increasing, each in [0, hp->epochs], and both
// result arrays (out_x may be NULL).  Each *_posttrain_rank calls this after its batch, probe
// and trace checks and before its first upload.
inline const char* kp_check_marks(const kp_hp* hp, const kp_marks* m) {
  if (!hp) return "missing hyper-parameters";
  if (hp->epochs < 0) return "negative epochs";
  if (m->n < 1 || m->n > KP_MARKS_MAX) return "n must be in [1, 16]";
  if (!m->epochs) return "missing epochs";
  for (int j = 0; j < m->n; ++j) {
    if (m->epochs[j] < 0) return "negative epoch";
    if (j > 0 && m->epochs[j] <= m->epochs[j - 1]) return "epochs must be strictly increasing";
    if (m->epochs[j] > hp->epochs) return "epoch beyond hp->epochs";
  }
  if (!m->out_score || !m->out_rank) return "missing mark output";
  return nullptr;
}

// The plan of a call's marks.  Mark j of slot s is the slot's kelpie row after
// slot_step[s * n + j] = e_j * (the slot's steps per epoch, as kp_trace_steps counts them) of
// its steps; 0 is the padded x0 every mark row starts as, so mark 0 and a slot without rows
// need no capture.  Every slot starts at global step 0 (kp_cx_plan.hpp, kp_cv_plan.hpp), so
// slot step k is global step k: for the host-driven step loops, global step t (0-based)
// captures, after its update, the (slot, mark row) pairs cap[2 i], cap[2 i + 1] for i in
// [step_off[t], step_off[t + 1]), slots ascending; mark row = s * n + j, the row of the mark
// workspace [slots][n][dp].  A (slot, step) holds at most one mark: the epochs are distinct.
struct KpMarkPlan {
  int n = 0, T = 0;                 // marks per slot; global steps (those of the longest slot)
  std::vector<int32_t> slot_step;   // [slots][n]
  std::vector<int32_t> step_off;    // [T + 1]
  std::vector<int32_t> cap;         // [step_off[T]][2]
};

// steps per epoch of one slot: kp_trace_slot_steps' count for one epoch
inline int kp_marks_steps_per_epoch(int model, int batch_size, const int32_t* rows, int R) {
  return (int)kp_trace_slot_steps(model, 1, batch_size, rows, R);
}

// Fills `plan` for a batch the batch check accepted and marks kp_check_marks accepted;
// nullptr, or the rule the arguments break.
inline const char* kp_marks_plan(int model, const kp_hp* hp, int n_slots, const int32_t* row_off,
                                 const int32_t* rows, const kp_marks* m, KpMarkPlan& plan) {
  plan = KpMarkPlan{};
  if (const char* why = kp_check_trace_args(model, hp, n_slots, row_off, rows)) return why;
  if (const char* why = kp_check_marks(hp, m)) return why;
  const int n = m->n;
  plan.n = n;
  plan.slot_step.assign((size_t)n_slots * n, 0);
  int64_t T = 0;
  for (int s = 0; s < n_slots; ++s) {
    const int R = row_off[s + 1] - row_off[s];
    const int64_t spe = kp_marks_steps_per_epoch(model, hp->batch_size, rows + 3 * (size_t)row_off[s], R);
    if (spe * hp->epochs > INT32_MAX) return "more than 2^31 - 1 steps";
    T = std::max(T, spe * hp->epochs);
    for (int j = 0; j < n; ++j) plan.slot_step[(size_t)s * n + j] = (int32_t)(spe * m->epochs[j]);
  }
  plan.T = (int)T;
  plan.step_off.assign((size_t)plan.T + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {  // count, then fill: slots ascending within a step
    std::vector<int32_t> at(plan.step_off.begin(), plan.step_off.end());
    for (int s = 0; s < n_slots; ++s)
      for (int j = 0; j < n; ++j) {
        const int k = plan.slot_step[(size_t)s * n + j];
        if (k <= 0) continue;
        if (pass == 0) {
          plan.step_off[k] += 1;  // step k - 1's count, one place up for the prefix sum
        } else {
          const int i = at[k - 1]++;
          plan.cap[2 * (size_t)i] = s;
          plan.cap[2 * (size_t)i + 1] = s * n + j;
        }
      }
    if (pass == 0) {
      for (int t = 0; t < plan.T; ++t) plan.step_off[t + 1] += plan.step_off[t];
      plan.cap.assign(2 * (size_t)plan.step_off[plan.T], 0);
    }
  }
  return nullptr;
}

// the mark row slot s captures after global step t (0-based), or -1
inline int kp_marks_row_at(const KpMarkPlan& plan, int s, int t) {
  for (int j = 0; j < plan.n; ++j)
    if (plan.slot_step[(size_t)s * plan.n + j] == t + 1) return s * plan.n + j;
  return -1;
}

// The marks of a batch the batch check accepted as rank rows (kp_common.hpp's RankSet):
// row r = s * nm + j is trip[3 r ..] = (r, p, o) of slot s (pred [n_slots][3]), po[r] its
// object, and its filter list [fo[r], fo[r + 1]) of `f` a copy of the slot's (`f` holds at
// least one entry).  nullptr, or the bound the rows exceed: nothing is written then, and
// `filt` is not read before the entry count is known to fit an int32.
inline const char* kp_mark_rows(int n_slots, int nm, const int32_t* pred, const int32_t* filt_off, const int32_t* filt,
                                std::vector<int32_t>& trip, std::vector<int32_t>& po, std::vector<int32_t>& fo,
                                std::vector<int32_t>& f) {
  if ((int64_t)n_slots * nm > INT32_MAX / 4) return "too many mark rows";
  int64_t nf = 0;
  for (int s = 0; s < n_slots; ++s) nf += (int64_t)nm * (filt_off[s + 1] - filt_off[s]);
  if (nf > INT32_MAX) return "the mark rows' filter lists exceed 2^31 - 1 entries";
  const size_t n = (size_t)n_slots * nm;
  trip.assign(n * 3, 0);
  po.assign(n, 0);
  fo.assign(n + 1, 0);
  f.assign((size_t)std::max<int64_t>(1, nf), 0);
  for (int s = 0; s < n_slots; ++s)
    for (int j = 0; j < nm; ++j) {
      const size_t r = (size_t)s * nm + j;
      trip[3 * r] = (int32_t)r;
      trip[3 * r + 1] = pred[3 * s + 1];
      trip[3 * r + 2] = po[r] = pred[3 * s + 2];
      const int len = filt_off[s + 1] - filt_off[s];
      if (len > 0) std::memcpy(&f[fo[r]], filt + filt_off[s], sizeof(int32_t) * len);
      fo[r + 1] = fo[r] + len;
    }
  return nullptr;
}
