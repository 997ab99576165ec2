// kp_attn_plan.hpp -- host side of the attention kernels' work partition: the plan
// structs handed to kp_attn / kp_attn3 and the planners that fill them.  No HIP in
// here: tests/native/attn_plan_driver.cpp builds this header alone (make attn_plan_asan).
#pragma once
#include <algorithm>

namespace kpattn {

// Work partition (stream-K style): the (64-query tile, 32-entity key tile) iterations
// of all query tiles, in query-tile-major order, are cut into equal contiguous
// ranges of per_wg iterations, one per workgroup, with exactly as many workgroups
// as the GPU holds at once.  A workgroup's range covers key-tile segments of one or
// more query tiles; each segment writes a partial (m, l, O) into slot `part` of its
// query tile, and the owner of a tile's last segment fills the unused slots up to
// n_parts with empty partials (m = -inf, l = 0, O = 0).  Consumers merge n_parts
// partials per query exactly as they merged N-split partials.
struct AttnWork {
  int ktq;      // key tiles per query tile, ceil(n_ent / 32)
  int per_wg;   // iterations per workgroup (stream-K)
  int n_parts;  // partial slots per query
  int ranges;   // > 0: XCD-grouped aligned key ranges (kp_attn3 only; attn_plan_ranges)
};

// Host: the stream-K partition for nq queries over n_ent keys on `slots` co-resident
// workgroups.  A workgroup takes at least ktq/15 key tiles, so a query tile is cut
// into at most 16 partials (the consumers' merge limit).
struct AttnPlan {
  AttnWork wk;
  int n_wg;
};
inline AttnPlan attn_plan(int nq, int n_ent, int slots) {
  const int QT = (nq + 63) / 64, ktq = (n_ent + 31) / 32;
  const long long total = (long long)QT * ktq;
  long long per = (total + slots - 1) / slots;
  per = std::max<long long>(per, (ktq + 14) / 15);
  per = std::max<long long>(per, 1);
  AttnPlan p{};
  p.n_wg = (int)((total + per - 1) / per);
  p.wk.ktq = ktq;
  p.wk.per_wg = (int)per;
  int parts = 1;
  for (int qt = 0; qt < QT; ++qt) {
    const long long w0 = ((long long)qt * ktq) / per, w1 = ((long long)(qt + 1) * ktq - 1) / per;
    parts = std::max(parts, (int)(w1 - w0 + 1));
  }
  p.wk.n_parts = parts;
  return p;
}

// What a (query tile, range) unit costs beside its key tiles, in tile-times: the Q load
// and split, the exposed first-tile DMA, the fp64 prefix correction and the O store
constexpr int kAttnUnitOverhead = 2;
// The in-flight model cuts a query tile no finer than it takes to have this share of
// the co-resident slots in units, in percent (profiles/HISTORY.md section 5, the S sweep)
#ifndef KP_ATTN_FILL_PCT
#define KP_ATTN_FILL_PCT 75  // A/B builds override it (make diag)
#endif
constexpr int kAttnInflightFillPct = KP_ATTN_FILL_PCT;

// Host: the XCD-grouped partition of kp_attn3.  The key tiles are cut into S aligned
// ranges; a unit is (query tile, range), numbered range-major, so consecutive units
// read the same keys.  Workgroup b (placed on XCD b % 8 by the dispatcher; used for
// speed only) takes logical id L = (b % 8) * (n_wg / 8) + b / 8 and units L, L + n_wg,
// ...: the workgroups of one XCD run consecutive units at the same time, so one key
// range streams into that XCD's L2 once and serves up to 32 query tiles, where the
// stream-K ranges of different workgroups are unrelated and every query tile re-reads
// the table from the Infinity Cache.  S minimises rounds x (range length + a per-unit
// overhead), at most 16 (the consumers' merge limit); every (query, range) partial is
// written.  This is the cost of a launch that has the device to itself.
inline AttnPlan attn_plan_ranges(int nq, int n_ent, int slots) {
  const int QT = (nq + 63) / 64, ktq = (n_ent + 31) / 32;
  const int n_wg = std::max(8, slots / 8 * 8);
  int best_s = 1;
  long long best = -1;
  for (int S = 1; S <= std::min(16, ktq); ++S) {
    const long long rounds = ((long long)QT * S + n_wg - 1) / n_wg;
    const long long cost = rounds * ((ktq + S - 1) / S + kAttnUnitOverhead);
    if (best < 0 || cost < best) {
      best = cost;
      best_s = S;
    }
  }
  AttnPlan p{};
  p.wk.ktq = ktq;
  p.wk.per_wg = 0;
  p.wk.n_parts = best_s;
  p.wk.ranges = best_s;
  p.n_wg = (int)std::min<long long>(n_wg, ((long long)QT * best_s + 7) / 8 * 8);
  return p;
}

// Host: S ranges (clamped to 1 .. min(16, ktq)) with one workgroup per unit, QT x S
// rounded up to the multiple of 8 the XCD mapping needs.  That may be more workgroups
// than are co-resident: the dispatcher then starts the rest as slots free up, and the
// kernel's unit walk ends after one unit (unit + n_wg >= n_units).
inline AttnPlan attn_plan_oneshot(int nq, int n_ent, int S) {
  const int QT = (nq + 63) / 64, ktq = (n_ent + 31) / 32;
  S = std::max(1, std::min(S, std::min(16, ktq)));
  AttnPlan p{};
  p.wk.ktq = ktq;
  p.wk.per_wg = 0;
  p.wk.n_parts = S;
  p.wk.ranges = S;
  p.n_wg = (int)(((long long)QT * S + 7) / 8 * 8);
  return p;
}

// Host: the model's workgroup time of a ranges plan, in tile-times: what the launch costs a
// device that other launches keep busy
inline long long attn_ranges_wg_time(int nq, int n_ent, int S) {
  const long long QT = (nq + 63) / 64, ktq = (n_ent + 31) / 32;
  return QT * S * ((ktq + S - 1) / S + kAttnUnitOverhead);
}

// The longest unit, in key tiles, the in-flight model cuts: the workgroups of an XCD share
// a range through L2 only while they stay in step, and they drift apart over a long unit
// (gains measured at 114 - 152 tiles per unit, FB15k-237; a loss at 3,113, DB100K)
constexpr int kAttnInflightMaxTiles = 256;

// Host: the ranges of a launch that shares the device with other batches' launches
// (kp_ctx_set_inflight >= 2).  The compute units a launch leaves free are taken by another
// batch's workgroups, so rounding up to whole rounds is no cost; what the launch costs the
// device is its total workgroup time, QT x S x (ktq / S + overhead), which falls with S,
// and so do the partials written and merged.  S is the smallest that still gives the
// launch kAttnInflightFillPct of the slots in units (a launch that runs alone for a while,
// or beside a short one, still spreads out), with one workgroup per unit.  Where that is
// more units than slots (the workgroups past the slots start late, alone and out of step:
// a tail of a whole unit), or units longer than kAttnInflightMaxTiles, the launch keeps
// the plan of a launch that runs alone (profiles/HISTORY.md section 5).
inline AttnPlan attn_plan_inflight(int nq, int n_ent, int slots, bool* applied = nullptr) {
  const int QT = (nq + 63) / 64, ktq = (n_ent + 31) / 32;
  const int n_slots = std::max(8, slots / 8 * 8);
  const long long want = (long long)kAttnInflightFillPct * n_slots;
  int S = 1;
  while (S < std::min(16, ktq) && 100LL * QT * S < want) ++S;
  const bool ok = (long long)QT * S <= n_slots && (ktq + S - 1) / S <= kAttnInflightMaxTiles;
  if (applied) *applied = ok;
  return ok ? attn_plan_oneshot(nq, n_ent, S) : attn_plan_ranges(nq, n_ent, slots);
}

// Host: the partition of one kp_attn3 launch.
//   part      0 chosen per launch, 1 stream-K, 2 ranges (KP_ATTN_PART)
//   inflight  the context's in-flight hint (1: the launch has the device to itself)
//   force_s   > 0: that many ranges, one workgroup per unit (KP_ATTN_RANGES)
// The ranges are taken unless their cost is more than 40 % over stream-K's balanced
// split: the L2 reuse they buy (FETCH_SIZE 14x lower, L2 hit rate 2 -> 91 %) outweighs
// a worse balance.  Alone the cost is rounds x unit time, in
// flight it is the total workgroup time of either partition.
inline AttnPlan attn_plan_select(int part, int inflight, int force_s, int nq, int n_ent, int slots) {
  const AttnPlan sk = attn_plan(nq, n_ent, slots);
  if (part == 1) return sk;
  if (force_s > 0) return attn_plan_oneshot(nq, n_ent, force_s);
  const long long QT = (nq + 63) / 64;
  bool shared = false;  // planned as a launch that shares the device
  const AttnPlan r = inflight >= 2 ? attn_plan_inflight(nq, n_ent, slots, &shared) : attn_plan_ranges(nq, n_ent, slots);
  if (part == 2) return r;
  const long long S = r.wk.ranges, ktq = r.wk.ktq;
  const long long n_wg = std::max(8, slots / 8 * 8);
  // alone: rounds x unit time; sharing the device: the launch's workgroup time per slot, as
  // stream-K's per_wg is
  const long long cost_r = shared ? (attn_ranges_wg_time(nq, n_ent, (int)S) + n_wg - 1) / n_wg
                                  : (QT * S + n_wg - 1) / n_wg * ((ktq + S - 1) / S + kAttnUnitOverhead);
  const long long cost_sk = (long long)sk.wk.per_wg + kAttnUnitOverhead;
  // measured on the interleaved kernel (tools/attn_micro.hip, FB15k-237 ComplEx, nq 800 -
  // 5,000): the ranges ran 9-21 % faster than stream-K at every size although their
  // quantisation was up to 25 % worse (profiles/r02o_attn_partition.jsonl)
  return 100 * cost_r <= 140 * cost_sk ? r : sk;
}

}  // namespace kpattn
