// kp_trace_check.hpp -- the post-training trace's step counts (kp_trace_steps) and the
// structural check of a call's kp_trace, as pure host functions (no HIP:
// tests/native/trace_check_driver.cpp builds this header alone under the host sanitizers).
#pragma once

#include <cstddef>
#include <cstdint>
#include <unordered_set>

#include "../../include/kelpie_hip.h"

// Steps of one slot: the step_on_batch calls of its post-training (include/kelpie_hip.h,
// "Post-training trace").  `rows` [R][3] are the slot's rows, inverses included.
//   ComplEx / DistMult / TransE: epochs * ceil(R / batch_size)
//     (multiclass_nll_optimizer.py:147-164, pairwise_ranking_optimizer.py:165-203)
//   ConvE: epochs * ceil(P / batch_size), P = the rows' distinct (head, relation) pairs,
//     the er_vocab keys kp_cv_plan.hpp groups (bce_optimizer.py:167-208)
// A slot without rows has no step.  The caller has checked batch_size > 0 and epochs >= 0.
inline int64_t kp_trace_slot_steps(int model, int epochs, int batch_size, const int32_t* rows, int R) {
  if (R <= 0 || epochs <= 0) return 0;
  int64_t n = R;
  if (model == KP_MODEL_CONVE) {
    std::unordered_set<uint64_t> seen;
    for (int j = 0; j < R; ++j)
      seen.insert(((uint64_t)(uint32_t)rows[3 * (size_t)j] << 32) | (uint32_t)rows[3 * (size_t)j + 1]);
    n = (int64_t)seen.size();
  }
  return (int64_t)epochs * ((n + batch_size - 1) / batch_size);
}

// nullptr when the arguments of kp_trace_steps are well formed, else the rule they break
inline const char* kp_check_trace_args(int model, const kp_hp* hp, int n_slots, const int32_t* row_off,
                                       const int32_t* rows) {
  if (model < KP_MODEL_TRANSE || model > KP_MODEL_DISTMULT) return "unknown model";
  if (!hp) return "missing hyper-parameters";
  if (hp->batch_size <= 0) return "batch_size must be positive";
  if (hp->epochs < 0) return "negative epochs";
  if (n_slots < 0) return "negative n_slots";
  if (n_slots == 0) return nullptr;
  if (!row_off) return "missing row_off";
  if (row_off[0] != 0) return "row_off must start at 0";
  for (int s = 0; s < n_slots; ++s)
    if (row_off[s + 1] < row_off[s]) return "row_off decreases";
  if (row_off[n_slots] > 0 && !rows) return "missing rows";
  return nullptr;
}

// out_steps[s] = the steps of slot s; nullptr, or the rule the arguments break (then
// out_steps is untouched).  A count that does not fit an int32 is refused.
inline const char* kp_trace_steps_host(int model, const kp_hp* hp, int n_slots, const int32_t* row_off,
                                       const int32_t* rows, int32_t* out_steps) {
  if (const char* why = kp_check_trace_args(model, hp, n_slots, row_off, rows)) return why;
  if (n_slots > 0 && !out_steps) return "missing out_steps";
  int64_t total = 0;
  for (int s = 0; s < n_slots; ++s) {
    total += kp_trace_slot_steps(model, hp->epochs, hp->batch_size, rows + 3 * (size_t)row_off[s],
                                 row_off[s + 1] - row_off[s]);
    if (total > INT32_MAX) return "more than 2^31 - 1 steps";
  }
  for (int s = 0; s < n_slots; ++s)
    out_steps[s] = (int32_t)kp_trace_slot_steps(model, hp->epochs, hp->batch_size, rows + 3 * (size_t)row_off[s],
                                                row_off[s + 1] - row_off[s]);
  return nullptr;
}

// nullptr when `tr` is a well-formed trace request for the batch (whose row_off / rows the
// batch check has accepted), else the rule it breaks: trace_off must be the prefix sums of
// kp_trace_steps' counts, and out_loss must be there when there is a step to write.  Each
// *_posttrain_rank calls this after its batch and probe checks and before its first upload.
inline const char* kp_check_trace(int model, const kp_hp* hp, int n_slots, const int32_t* row_off,
                                  const int32_t* rows, const kp_trace* tr) {
  if (const char* why = kp_check_trace_args(model, hp, n_slots, row_off, rows)) return why;
  if (!tr->trace_off) return "missing trace_off";
  if (tr->trace_off[0] != 0) return "trace_off must start at 0";
  int64_t total = 0;
  for (int s = 0; s < n_slots; ++s) {
    total += kp_trace_slot_steps(model, hp->epochs, hp->batch_size, rows + 3 * (size_t)row_off[s],
                                 row_off[s + 1] - row_off[s]);
    if (total > INT32_MAX) return "more than 2^31 - 1 steps";
    if ((int64_t)tr->trace_off[s + 1] != total) return "trace_off disagrees with kp_trace_steps";
  }
  if (total > 0 && !tr->out_loss) return "missing out_loss";
  return nullptr;
}
