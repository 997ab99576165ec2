// kp_cx_rowmap.hpp -- which training row is which in a ComplEx / DistMult step plan.  The plan
// (kp_cx_plan.hpp) merges a minibatch's rows by relation and by frozen (h, r) pair and forgets
// the rows; the attributions (include/kelpie_hip.h, "Attributions") write one number per row,
// so this map restores, per plan, each query's frozen target -> row id, each query's
// kelpie-target rows, and each tail's rows.  Row ids are batch-wide: row_off[slot] + the row's
// index in the slot.  No HIP in here: tests/native/attrib_driver.cpp builds this header alone
// (make attrib_asan).
#pragma once

#include <cstdint>
#include <unordered_map>
#include <vector>

#include "kp_cx_plan.hpp"

struct CxRowMap {
  std::vector<int32_t> tg_row;  // [sp.targets]: the row whose frozen tail is sp.targets[i]
  std::vector<int32_t> qk_off;  // [sp.pqs + 1]: query j's (kelpie, rel, kelpie) rows are
  std::vector<int32_t> qk_row;  //   qk_row[qk_off[j], qk_off[j + 1]), sp.pqs[j].ck of them
  std::vector<int32_t> t_off;   // [sp.pts + 1]: tail j's rows are t_row[t_off[j], t_off[j + 1]),
  std::vector<int32_t> t_row;   //   sp.pts[j].c of them
};

// the rows of one minibatch into the map of plan `plan`: rows[idx[k]] (idx == nullptr: rows[k])
// for k < n, row ids base + that index; in the plan builder's order (CxPlanBuilder::add_plan)
inline const char* cx_row_map_plan(const CxStepPlan& sp, int plan, int K, const int32_t* rows, const int32_t* idx,
                                   int n, int base, CxRowMap& m) {
  if (plan >= (int)sp.plans.size()) return "row map: more minibatches than plans";
  const CxPlan& P = sp.plans[plan];
  if (P.b != n) return "row map: a plan of another minibatch size";
  if (P.q_begin != (int)m.qk_off.size() - 1 || P.t_begin != (int)m.t_off.size() - 1)
    return "row map: the plans are not in the planner's order";
  std::unordered_map<int, int> rel_q;                // relation -> plan query
  std::unordered_map<int64_t, int> pair_t;           // h * 2^32 + r -> plan tail
  for (int j = 0; j < P.q_count; ++j) rel_q.emplace(sp.pqs[P.q_begin + j].rel, P.q_begin + j);
  for (int j = 0; j < P.t_count; ++j) {
    const CxI2 hr = sp.pairs[sp.pts[P.t_begin + j].pair];
    pair_t.emplace(((int64_t)hr.x << 32) | (uint32_t)hr.y, P.t_begin + j);
  }
  std::vector<int> tg_fill(P.q_count, 0), qk_fill(P.q_count, 0), t_fill(P.t_count, 0);
  // offsets first: the counts are the plan's
  for (int j = 0; j < P.q_count; ++j) m.qk_off.push_back(m.qk_off.back() + sp.pqs[P.q_begin + j].ck);
  for (int j = 0; j < P.t_count; ++j) m.t_off.push_back(m.t_off.back() + sp.pts[P.t_begin + j].c);
  m.qk_row.resize(m.qk_off.back(), -1);
  m.t_row.resize(m.t_off.back(), -1);
  for (int k = 0; k < n; ++k) {
    const int i = idx ? idx[k] : k;
    const int32_t* rw = rows + 3 * (size_t)i;
    if (rw[0] == K) {
      const auto it = rel_q.find(rw[1]);
      if (it == rel_q.end()) return "row map: a row's relation has no query";
      const int q = it->second, j = q - P.q_begin;
      const CxQuery& Q = sp.pqs[q];
      if (rw[2] == K) {
        if (qk_fill[j] >= Q.ck) return "row map: more kelpie-target rows than the query counts";
        m.qk_row[m.qk_off[q] + qk_fill[j]++] = base + i;
      } else {
        if (tg_fill[j] >= Q.tg_count || sp.targets[Q.tg_begin + tg_fill[j]] != rw[2])
          return "row map: a frozen target out of the plan's order";
        m.tg_row[Q.tg_begin + tg_fill[j]++] = base + i;
      }
    } else {
      const auto it = pair_t.find(((int64_t)rw[0] << 32) | (uint32_t)rw[1]);
      if (it == pair_t.end()) return "row map: a row's pair has no tail";
      const int t = it->second, j = t - P.t_begin;
      if (t_fill[j] >= sp.pts[t].c) return "row map: more rows than the tail counts";
      m.t_row[m.t_off[t] + t_fill[j]++] = base + i;
    }
  }
  for (int j = 0; j < P.q_count; ++j)
    if (tg_fill[j] != sp.pqs[P.q_begin + j].tg_count || qk_fill[j] != sp.pqs[P.q_begin + j].ck)
      return "row map: a query with fewer rows than it counts";
  for (int j = 0; j < P.t_count; ++j)
    if (t_fill[j] != sp.pts[P.t_begin + j].c) return "row map: a tail with fewer rows than it counts";
  return nullptr;
}

// The map of a step plan that cx_step_plan built from the same arguments.  nullptr when good.
inline const char* cx_row_map(int n_ent, int batch_size, int epochs, const kp_batch* bt, const CxStepPlan& sp,
                              CxRowMap& m) {
  m = CxRowMap{};
  m.tg_row.assign(sp.targets.size(), -1);
  m.qk_off.assign(1, 0);
  m.t_off.assign(1, 0);
  int plan = 0;
  for (int s = 0; s < bt->n_slots; ++s) {
    const int r0 = bt->row_off[s], R = bt->row_off[s + 1] - r0;
    const int32_t* rows = bt->rows + 3 * (size_t)r0;
    if (R == 0 || epochs == 0) continue;
    const int nst = (R + batch_size - 1) / batch_size;
    const int bs = std::min(batch_size, R);
    if (nst == 1) {
      if (const char* why = cx_row_map_plan(sp, plan++, n_ent, rows, nullptr, R, r0, m)) return why;
    } else {
      const int64_t g0 = bt->rng_off[s];
      for (int e = 0; e < epochs; ++e) {
        const int32_t* perm = bt->rng + g0 + (int64_t)e * R;
        for (int j = 0; j < nst; ++j) {
          const int st = j * batch_size;
          if (const char* why = cx_row_map_plan(sp, plan++, n_ent, rows, perm + st, std::min(bs, R - st), r0, m))
            return why;
        }
      }
    }
  }
  if (plan != (int)sp.plans.size()) return "row map: fewer minibatches than plans";
  return nullptr;
}
