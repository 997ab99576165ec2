// attn_plan_driver.cpp -- the attention planners (kelpie_amd/csrc/kp_attn_plan.hpp, which
// kp_attn.hpp includes: the header with the kernels does not compile without HIP) on their
// own: `make attn_plan` builds this file plain, `make attn_plan_asan` with
// -fsanitize=address,undefined, and tests/test_attn_plan.py runs both.  For every
// (nq, n_ent, slots, in-flight hint) the plan must keep what kp_attn3 and the merge kernels
// rely on; the kernel's own unit walk is replayed on the host into a heap vector of exactly
// n_units counters, so a walk that leaves the units is reported.  Prints one line per group
// and exits 0 iff every check held.
#include <cstdio>
#include <vector>

#include "../../kelpie_amd/csrc/kp_attn_plan.hpp"

namespace {

int failures = 0;

#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      ++failures;                     \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);       \
      std::printf("\n");              \
    }                                 \
  } while (0)

int ceil8(long long x) { return (int)((x + 7) / 8 * 8); }

// kp_attn3's work loop for a ranges plan: logical id from the block id, then unit += n_wg
void check_ranges_plan(const kpattn::AttnPlan& p, int nq, int n_ent, const char* what) {
  const int QT = (nq + 63) / 64, ktq = (n_ent + 31) / 32;
  const int S = p.wk.ranges;
  CHECK(p.wk.ktq == ktq, "%s nq %d n_ent %d: ktq %d", what, nq, n_ent, p.wk.ktq);
  CHECK(S >= 1 && S <= std::min(16, ktq), "%s nq %d n_ent %d: S %d", what, nq, n_ent, S);
  CHECK(p.wk.n_parts == S, "%s nq %d n_ent %d: n_parts %d, S %d", what, nq, n_ent, p.wk.n_parts, S);
  CHECK(p.n_wg >= 8 && p.n_wg % 8 == 0, "%s nq %d n_ent %d: n_wg %d", what, nq, n_ent, p.n_wg);
  if (S < 1 || S > 16 || p.n_wg < 8 || p.n_wg % 8 != 0) return;
  // the ranges tile [0, ktq), none empty
  int at = 0;
  for (int part = 0; part < S; ++part) {
    const int kt0 = (int)((long long)part * ktq / S), kt1 = (int)((long long)(part + 1) * ktq / S);
    CHECK(kt0 == at && kt1 > kt0, "%s nq %d n_ent %d S %d: range %d = [%d, %d)", what, nq, n_ent, S, part, kt0, kt1);
    at = kt1;
  }
  CHECK(at == ktq, "%s nq %d n_ent %d S %d: ranges end at %d of %d", what, nq, n_ent, S, at, ktq);
  // every unit exactly once
  const int n_units = QT * S;
  std::vector<int> seen((size_t)n_units, 0);
  for (int b = 0; b < p.n_wg; ++b) {
    int unit = (b % 8) * (p.n_wg / 8) + b / 8;
    for (; unit < n_units; unit += p.n_wg) ++seen[(size_t)unit];
  }
  int bad = 0;
  for (int u = 0; u < n_units; ++u) bad += seen[(size_t)u] != 1;
  CHECK(bad == 0, "%s nq %d n_ent %d S %d n_wg %d: %d of %d units not visited once", what, nq, n_ent, S, p.n_wg, bad,
        n_units);
}

// kp_attn3's stream-K walk: workgroup b takes iterations [b per_wg, (b + 1) per_wg)
void check_streamk_plan(const kpattn::AttnPlan& p, int nq, int n_ent) {
  const int QT = (nq + 63) / 64, ktq = (n_ent + 31) / 32;
  const long long total = (long long)QT * ktq;
  CHECK(p.wk.per_wg >= 1 && (long long)p.n_wg * p.wk.per_wg >= total && (long long)(p.n_wg - 1) * p.wk.per_wg < total,
        "stream-K nq %d n_ent %d: n_wg %d per_wg %d", nq, n_ent, p.n_wg, p.wk.per_wg);
  CHECK(p.wk.n_parts >= 1 && p.wk.n_parts <= 16, "stream-K nq %d n_ent %d: n_parts %d", nq, n_ent, p.wk.n_parts);
}

}  // namespace

int main() {
  using namespace kpattn;
  const int nqs[] = {1, 63, 64, 65, 1029, 4204, 20000};
  const int ents[] = {33, 517, 14541};
  const int slotss[] = {8, 256, 512};
  int plans = 0;
  for (int nq : nqs)
    for (int n_ent : ents)
      for (int slots : slotss)
        for (int hint = 1; hint <= 4; ++hint) {
          const int QT = (nq + 63) / 64;
          // the ranges, as KP_ATTN_PART=ranges forces them and as the planner chooses
          const AttnPlan r = attn_plan_select(2, hint, 0, nq, n_ent, slots);
          check_ranges_plan(r, nq, n_ent, hint == 1 ? "ranges alone" : "ranges in flight");
          if (hint == 1) {
            const AttnPlan old = attn_plan_ranges(nq, n_ent, slots);
            CHECK(r.wk.ranges == old.wk.ranges && r.n_wg == old.n_wg && r.n_wg <= std::max(8, slots / 8 * 8),
                  "hint 1 nq %d n_ent %d slots %d: (%d, %d) vs (%d, %d)", nq, n_ent, slots, r.wk.ranges, r.n_wg,
                  old.wk.ranges, old.n_wg);
          } else {
            // one workgroup per unit of the smallest S that fills the share of the slots, all
            // of them resident and no unit longer than the model cuts; else the plan alone
            const AttnPlan old = attn_plan_ranges(nq, n_ent, slots);
            const int cap = std::min(16, (n_ent + 31) / 32), ktq = (n_ent + 31) / 32;
            const int n_slots = std::max(8, slots / 8 * 8);
            const long long want = (long long)kAttnInflightFillPct * n_slots;
            const int S = r.wk.ranges;
            const bool smallest = (100LL * QT * S >= want || S == cap) && (S == 1 || 100LL * QT * (S - 1) < want);
            const bool shared = r.n_wg == ceil8((long long)QT * S) && smallest && r.n_wg <= n_slots &&
                                (ktq + S - 1) / S <= kAttnInflightMaxTiles;
            const bool alone = S == old.wk.ranges && r.n_wg == old.n_wg;
            CHECK(shared || alone, "hint %d nq %d n_ent %d slots %d: (%d, %d), alone (%d, %d)", hint, nq, n_ent, slots, S,
                  r.n_wg, old.wk.ranges, old.n_wg);
          }
          const AttnPlan chosen = attn_plan_select(0, hint, 0, nq, n_ent, slots);
          if (chosen.wk.ranges)
            check_ranges_plan(chosen, nq, n_ent, "chosen");
          else
            check_streamk_plan(chosen, nq, n_ent);
          check_streamk_plan(attn_plan_select(1, hint, 0, nq, n_ent, slots), nq, n_ent);
          // KP_ATTN_RANGES: every S, past the cap too
          for (int fs : {1, 2, 3, 16, 40}) {
            const AttnPlan f = attn_plan_select(0, hint, fs, nq, n_ent, slots);
            check_ranges_plan(f, nq, n_ent, "forced");
            CHECK(f.wk.ranges == std::min(fs, std::min(16, (n_ent + 31) / 32)) && f.n_wg == ceil8((long long)QT * f.wk.ranges),
                  "forced %d nq %d n_ent %d: S %d n_wg %d", fs, nq, n_ent, f.wk.ranges, f.n_wg);
            ++plans;
          }
          plans += 3;
        }
  std::printf("grid: %d plans\n", plans);

  // hint 1 is the plan of a launch that runs alone, unchanged: 256 slots, FB15k-237
  const int alone[][3] = {{3000, 5, 240}, {3730, 13, 256}, {4204, 11, 256}, {4500, 7, 256}};
  for (const auto& a : alone) {
    const AttnPlan p = attn_plan_select(0, 1, 0, a[0], 14541, 256);
    CHECK(p.wk.ranges == a[1] && p.wk.n_parts == a[1] && p.n_wg == a[2], "alone nq %d: (%d, %d), expected (%d, %d)", a[0],
          p.wk.ranges, p.n_wg, a[1], a[2]);
  }
  std::printf("alone: 4 plans\n");

  // hint 3 at the flagship's shapes: one workgroup per unit, n_wg = ceil8(QT S)
  for (int nq : {3000, 3730, 4204, 4500, 5000}) {
    const AttnPlan p = attn_plan_select(0, 3, 0, nq, 14541, 256);
    const int QT = (nq + 63) / 64;
    CHECK(p.wk.ranges >= 1 && p.n_wg == ceil8((long long)QT * p.wk.ranges), "in flight nq %d: (%d, %d)", nq, p.wk.ranges,
          p.n_wg);
    std::printf("in flight: nq %d -> S %d, n_wg %d\n", nq, p.wk.ranges, p.n_wg);
  }
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
