// kp_cx_plan.hpp -- host planning of the ComplEx / DistMult post-training steps: the
// training rows of every slot grouped into per-step plans (queries, frozen targets,
// frozen-head pairs and tails) and the per-step active lists with their offsets.  The step
// loop of kp_complex.hip adds these offsets to device pointers and its kernels index with
// the stored ids, so everything is decided here.  No HIP in here:
// tests/native/step_plan_driver.cpp builds this header alone (make step_plan_asan).
//
// When R <= batch_size (one step per epoch) the permutation only reorders the batch, so
// every epoch reuses one plan; otherwise each (epoch, step) gets its own plan from the
// permutation.
#pragma once

#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../include/kelpie_hip.h"

// one minibatch: b rows, its queries [q_begin, +q_count) and tails [t_begin, +t_count);
// cnt_l rows with the kelpie as head, cnt_r rows with the kelpie as tail
struct CxPlan {
  int b, q_begin, q_count, t_begin, t_count, cnt_l, cnt_r, pad;
};
// the rows (kelpie, rel, .) of one minibatch: c rows, ck of them with the kelpie as tail,
// the frozen tails in targets[tg_begin, +tg_count)
struct CxQuery {
  int rel, c, ck, tg_begin, tg_count, pad0, pad1, pad2;
};
// the c rows (h, r, kelpie) of one minibatch with (h, r) = pairs[pair]
struct CxTail {
  int pair, c;
};
// the device lists' element types, laid out as HIP's int2 / int4 (kp_complex.hip asserts it)
struct alignas(8) CxI2 {
  int x, y;
};
struct alignas(16) CxI4 {
  int x, y, z, w;
};

struct CxStepPlan {
  std::vector<CxPlan> plans;
  std::vector<CxQuery> pqs;
  std::vector<CxTail> pts;
  std::vector<int32_t> targets;
  std::vector<CxI2> pairs;  // distinct frozen (h, r) of the whole batch
  // per step t: acts[act_off[t], act_off[t+1]) = (slot, plan, first query, first tail of the
  // slot within the step), stepq[q_off[t], ..) = (slot, rel, query, 0), stept[t_off[t], ..)
  // = (slot, pair, c, 0)
  std::vector<CxI4> acts, stepq, stept;
  std::vector<int> act_off, q_off, t_off;  // [T + 1]
  int T = 0;                               // steps of the longest slot
  int max_nq = 0, max_items = 0;           // most queries / queries + tails of one step
};

// groups minibatches into plans; the scratch is kept across minibatches
struct CxPlanBuilder {
  CxStepPlan& sp;
  const int K, n_rel2;         // kelpie id, relation count
  std::vector<int> rel_slot;   // relation -> its query in the current minibatch, or -1
  std::vector<int> rels;       // the current minibatch's relations, first-seen order
  std::vector<int> qtg_count;  // frozen targets per query of the current minibatch
  std::unordered_map<int, int> tail_slot;    // pair -> its tail in the current minibatch
  std::unordered_map<int64_t, int> pair_id;  // h * n_rel2 + r -> pair

  CxPlanBuilder(CxStepPlan& out, int n_ent, int n_rel2_) : sp(out), K(n_ent), n_rel2(n_rel2_), rel_slot(n_rel2_, -1) {}

  // one minibatch: rows[idx[k]] (idx == nullptr: rows[k]) for k < n
  const char* add_plan(const int32_t* rows, const int32_t* idx, int n) {
    CxPlan P{};
    P.b = n;
    P.q_begin = (int)sp.pqs.size();
    P.t_begin = (int)sp.pts.size();
    rels.clear();
    qtg_count.clear();
    tail_slot.clear();
    // pass 1: group
    for (int k = 0; k < n; ++k) {
      const int32_t* rw = rows + 3 * (size_t)(idx ? idx[k] : k);
      const int h = rw[0], r = rw[1], t = rw[2];
      if (h == K) {
        if (rel_slot[r] < 0) {
          rel_slot[r] = (int)rels.size();
          rels.push_back(r);
          qtg_count.push_back(0);
          sp.pqs.push_back(CxQuery{r, 0, 0, 0, 0, 0, 0, 0});
        }
        CxQuery& Q = sp.pqs[P.q_begin + rel_slot[r]];
        Q.c += 1;
        P.cnt_l += 1;
        if (t == K) {
          Q.ck += 1;
          P.cnt_r += 1;
        } else {
          qtg_count[rel_slot[r]] += 1;
        }
      } else {
        if (t != K) return "a training row does not involve the kelpie entity";
        P.cnt_r += 1;
        const int64_t key = (int64_t)h * n_rel2 + r;
        auto it = pair_id.find(key);
        int pid;
        if (it == pair_id.end()) {
          pid = (int)sp.pairs.size();
          pair_id.emplace(key, pid);
          sp.pairs.push_back(CxI2{h, r});
        } else {
          pid = it->second;
        }
        auto jt = tail_slot.find(pid);
        if (jt == tail_slot.end()) {
          tail_slot.emplace(pid, (int)sp.pts.size());
          sp.pts.push_back(CxTail{pid, 1});
        } else {
          sp.pts[jt->second].c += 1;
        }
      }
    }
    // pass 2: frozen targets grouped per query
    int base = (int)sp.targets.size();
    for (size_t j = 0; j < rels.size(); ++j) {
      sp.pqs[P.q_begin + j].tg_begin = base;
      sp.pqs[P.q_begin + j].tg_count = 0;
      base += qtg_count[j];
    }
    sp.targets.resize(base);
    for (int k = 0; k < n; ++k) {
      const int32_t* rw = rows + 3 * (size_t)(idx ? idx[k] : k);
      if (rw[0] == K && rw[2] != K) {
        CxQuery& Q = sp.pqs[P.q_begin + rel_slot[rw[1]]];
        sp.targets[Q.tg_begin + Q.tg_count++] = rw[2];
      }
    }
    for (int r : rels) rel_slot[r] = -1;
    P.q_count = (int)rels.size();
    P.t_count = (int)sp.pts.size() - P.t_begin;
    sp.plans.push_back(P);
    return nullptr;
  }
};

// Fills `sp` for a batch that kp_check_batch accepted (every row id in range).  nullptr
// when the plan is good, else the rule the batch breaks.
inline const char* cx_step_plan(int n_ent, int n_rel2, int batch_size, int epochs, const kp_batch* bt,
                                CxStepPlan& sp) {
  sp = CxStepPlan{};
  const int ns = bt->n_slots, E = epochs;
  CxPlanBuilder pb(sp, n_ent, n_rel2);
  std::vector<int> plan_base(ns, 0), nsteps(ns, 0);
  int T = 0;
  for (int s = 0; s < ns; ++s) {
    const int r0 = bt->row_off[s], r1 = bt->row_off[s + 1];
    const int R = r1 - r0;
    const int32_t* rows = bt->rows + 3 * (size_t)r0;
    plan_base[s] = (int)sp.plans.size();
    if (R == 0 || E == 0) continue;
    const int nst = (R + batch_size - 1) / batch_size;
    const int bs = std::min(batch_size, R);
    nsteps[s] = nst;
    if (nst == 1) {
      if (const char* why = pb.add_plan(rows, nullptr, R)) return why;
    } else {
      const int64_t g0 = bt->rng_off[s], g1 = bt->rng_off[s + 1];
      if (g1 - g0 < (int64_t)E * R) return "missing randperm draws for a multi-step slot";
      for (int e = 0; e < E; ++e) {
        const int32_t* perm = bt->rng + g0 + (int64_t)e * R;
        for (int j = 0; j < R; ++j)
          if (perm[j] < 0 || perm[j] >= R) return "randperm value out of range";
        for (int j = 0; j < nst; ++j) {
          const int st = j * batch_size;
          if (const char* why = pb.add_plan(rows, perm + st, std::min(bs, R - st))) return why;
        }
      }
    }
    T = std::max(T, E * nst);
  }

  // per-step active lists
  sp.T = T;
  sp.act_off.assign(T + 1, 0);
  sp.q_off.assign(T + 1, 0);
  sp.t_off.assign(T + 1, 0);
  for (int t = 0; t < T; ++t) {
    sp.act_off[t] = (int)sp.acts.size();
    sp.q_off[t] = (int)sp.stepq.size();
    sp.t_off[t] = (int)sp.stept.size();
    int qo = 0, to = 0;
    for (int s = 0; s < ns; ++s) {
      const int nst = nsteps[s];
      if (nst == 0 || t >= E * nst) continue;
      const int plan = plan_base[s] + (nst == 1 ? 0 : t);
      sp.acts.push_back(CxI4{s, plan, qo, to});
      const CxPlan& P = sp.plans[plan];
      for (int j = 0; j < P.q_count; ++j) sp.stepq.push_back(CxI4{s, sp.pqs[P.q_begin + j].rel, P.q_begin + j, 0});
      for (int j = 0; j < P.t_count; ++j)
        sp.stept.push_back(CxI4{s, sp.pts[P.t_begin + j].pair, sp.pts[P.t_begin + j].c, 0});
      qo += P.q_count;
      to += P.t_count;
    }
    sp.max_nq = std::max(sp.max_nq, qo);
    sp.max_items = std::max(sp.max_items, qo + to);
  }
  sp.act_off[T] = (int)sp.acts.size();
  sp.q_off[T] = (int)sp.stepq.size();
  sp.t_off[T] = (int)sp.stept.size();
  return nullptr;
}
