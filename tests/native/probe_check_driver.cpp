// probe_check_driver.cpp -- the probes' host check and chunking (kelpie_amd/csrc/
// kp_probe_check.hpp) alone, plain and under the host sanitizers: `make probe_check
// probe_check_asan` builds this file, tests/test_probe_check.py runs it.
//   * a good set of probes passes, with and without probes, with an empty slot;
//   * errors: the good set with exactly one rule broken must yield that rule's message;
//   * the probes as rank rows: a slot without probes between two that have some;
//   * the slots as rank rows: 0, 1 and 3 slots, the kelpie entity among the objects;
//   * on 400 pseudo-random valid sets the check passes and the chunks cover every probe row
//     once, within the budget.
// The arrays are heap vectors of their exact length, so a check that reads past one is
// reported.  Prints one line per case and exits 0 iff every case went as expected.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../kelpie_amd/csrc/kp_probe_check.hpp"

namespace {

constexpr int K = 7;   // n_ent; the kelpie entity's id
constexpr int NR = 4;  // n_rel2

int failures = 0;
void fail(const std::string& what) {
  std::printf("FAIL %s\n", what.c_str());
  ++failures;
}
void expect_msg(const std::string& what, const char* got, const char* want) {
  const bool same = (got == nullptr && want == nullptr) || (got && want && std::strcmp(got, want) == 0);
  std::printf("%s: %s\n", what.c_str(), got ? got : "ok");
  if (!same) fail(what + ": expected " + (want ? want : "good probes"));
}

struct Probes {
  std::vector<int32_t> probe_off{0}, probes, filt_off{0}, filt;
  std::vector<float> score;
  std::vector<int64_t> rank;
  // one slot's probes: (p, o, filter) each
  void slot(const std::vector<std::vector<int>>& ps) {
    for (auto& p : ps) {
      probes.push_back(p[0]);
      probes.push_back(p[1]);
      filt.insert(filt.end(), p.begin() + 2, p.end());
      filt_off.push_back((int32_t)filt.size());
    }
    probe_off.push_back((int32_t)(probes.size() / 2));
  }
  kp_probes view() {
    score.assign(probes.size() / 2, 0.f);
    rank.assign(probes.size() / 2, 0);
    kp_probes v;
    v.n = (int32_t)(probes.size() / 2);
    v.probe_off = probe_off.data();
    v.probes = probes.data();
    v.filt_off = filt_off.data();
    v.filt = filt.data();
    v.out_score = score.data();
    v.out_rank = rank.data();
    return v;
  }
  int slots() const { return (int)probe_off.size() - 1; }
};

// three slots, the middle one empty: (p, o, filter ...)
Probes good() {
  Probes g;
  g.slot({{0, 3, 1, 2}, {3, K}});
  g.slot({});
  g.slot({{1, 0, K, 0}});
  return g;
}

void errors() {
  {
    Probes g = good();
    kp_probes v = g.view();
    expect_msg("good", kp_check_probes(K, NR, g.slots(), &v), nullptr);
  }
  {
    Probes g;
    g.slot({});
    g.slot({});
    kp_probes v = g.view();
    v.probes = nullptr, v.filt_off = nullptr, v.filt = nullptr, v.out_score = nullptr, v.out_rank = nullptr;
    expect_msg("no probes, null arrays", kp_check_probes(K, NR, 2, &v), nullptr);
  }
  struct Case {
    const char* name;
    void (*edit)(Probes&, kp_probes&);
    const char* want;
  };
  const Case cases[] = {
      {"probe_off starts at 1", [](Probes& g, kp_probes&) { g.probe_off[0] = 1; }, "probe_off must start at 0"},
      {"probe_off decreases", [](Probes& g, kp_probes&) { g.probe_off[1] = 3, g.probe_off[2] = 2; }, "probe_off decreases"},
      {"probe_off ends short", [](Probes& g, kp_probes&) { g.probe_off[3] = 2; }, "probe_off must end at the probe count"},
      {"probe_off ends past", [](Probes&, kp_probes& v) { v.n = 2; }, "probe_off must end at the probe count"},
      {"negative count", [](Probes&, kp_probes& v) { v.n = -1; }, "negative probe count"},
      {"null probe_off", [](Probes&, kp_probes& v) { v.probe_off = nullptr; }, "missing probe_off"},
      {"null probes", [](Probes&, kp_probes& v) { v.probes = nullptr; }, "missing probes"},
      {"null filt_off", [](Probes&, kp_probes& v) { v.filt_off = nullptr; }, "missing filt_off"},
      {"null filt", [](Probes&, kp_probes& v) { v.filt = nullptr; }, "missing filt"},
      {"null out_score", [](Probes&, kp_probes& v) { v.out_score = nullptr; }, "missing probe output"},
      {"null out_rank", [](Probes&, kp_probes& v) { v.out_rank = nullptr; }, "missing probe output"},
      {"relation n_rel2", [](Probes& g, kp_probes&) { g.probes[2] = NR; }, "probe relation out of range"},
      {"relation -1", [](Probes& g, kp_probes&) { g.probes[0] = -1; }, "probe relation out of range"},
      {"object n_ent + 1", [](Probes& g, kp_probes&) { g.probes[3] = K + 1; }, "probe object out of range"},
      {"object -1", [](Probes& g, kp_probes&) { g.probes[5] = -1; }, "probe object out of range"},
      {"filt_off starts at 1", [](Probes& g, kp_probes&) { g.filt_off[0] = 1; }, "filt_off must start at 0"},
      {"filt_off decreases", [](Probes& g, kp_probes&) { g.filt_off[1] = 3, g.filt_off[2] = 2; }, "filt_off decreases"},
      {"filter id n_ent + 1", [](Probes& g, kp_probes&) { g.filt[3] = K + 1; }, "probe filter id out of range"},
      {"filter id -1", [](Probes& g, kp_probes&) { g.filt[0] = -1; }, "probe filter id out of range"},
  };
  for (const Case& c : cases) {
    Probes g = good();
    kp_probes v = g.view();
    c.edit(g, v);
    expect_msg(c.name, kp_check_probes(K, NR, g.slots(), &v), c.want);
  }
  {
    Probes g = good();
    kp_probes v = g.view();
    expect_msg("empty model", kp_check_probes(0, NR, g.slots(), &v), "empty model");
    expect_msg("negative n_slots", kp_check_probes(K, NR, -1, &v), "negative n_slots");
  }
}

// the probes as rank rows (kp_probe_rows): row i is (slot, p, o) of probe i
void rank_rows() {
  Probes g = good();  // slot 0: two probes, slot 1: none, slot 2: one
  const kp_probes v = g.view();
  std::vector<int32_t> trip{99}, po{99, 99};  // stale contents must go
  kp_probe_rows(g.slots(), &v, trip, po);
  const bool ok = trip == std::vector<int32_t>{0, 0, 3, 0, 3, K, 2, 1, 0} && po == std::vector<int32_t>{3, K, 0};
  std::printf("rows, empty middle slot: %s\n", ok ? "ok" : "wrong rows");
  if (!ok) fail("rows, empty middle slot");
  Probes e;
  e.slot({});
  e.slot({});
  const kp_probes ev = e.view();
  kp_probe_rows(2, &ev, trip, po);
  std::printf("rows, no probes: %s\n", trip.empty() && po.empty() ? "ok" : "wrong rows");
  if (!trip.empty() || !po.empty()) fail("rows, no probes");
}

// the slots as rank rows (kp_slot_rows): row s is (s, p, o) of the slot's ranked triple
// (kelpie, p, o); 0, 1 and 3 slots, the kelpie entity among the objects
void slot_rows() {
  struct Case {
    const char* name;
    std::vector<int32_t> pred, trip, po;
  };
  const Case cases[] = {
      {"slot rows, no slots", {}, {}, {}},
      {"slot rows, one slot", {K, 2, K}, {0, 2, K}, {K}},
      {"slot rows, three slots", {K, 0, 3, K, 3, K, K, 1, 0}, {0, 0, 3, 1, 3, K, 2, 1, 0}, {3, K, 0}},
  };
  for (const Case& c : cases) {
    std::vector<int32_t> trip{99, 99}, po{99};  // stale contents must go
    kp_slot_rows((int)c.po.size(), c.pred.data(), trip, po);
    const bool ok = trip == c.trip && po == c.po;
    std::printf("%s: %s\n", c.name, ok ? "ok" : "wrong rows");
    if (!ok) fail(c.name);
  }
}

uint32_t rnd_state = 12345u;
int rnd(int n) {  // [0, n)
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return (int)((rnd_state >> 8) % (uint32_t)n);
}

void random_sets() {
  int n_sets = 0;
  for (int it = 0; it < 400; ++it) {
    const int n_ent = 1 + rnd(300), n_rel2 = 2 * (1 + rnd(6)), ns = rnd(9);
    Probes g;
    for (int s = 0; s < ns; ++s) {
      std::vector<std::vector<int>> ps(rnd(4) == 0 ? 0 : rnd(20));
      for (auto& p : ps) {
        p = {rnd(n_rel2), rnd(n_ent + 1)};
        for (int f = rnd(6); f > 0; --f) p.push_back(rnd(n_ent + 1));
      }
      g.slot(ps);
    }
    kp_probes v = g.view();
    const char* why = kp_check_probes(n_ent, n_rel2, ns, &v);
    if (why) fail(std::string("random set ") + std::to_string(it) + ": " + why);
    // the chunks: every row once, whole groups when one fits, within the budget
    const size_t row_bytes = 8 * (size_t)(16 * (1 + rnd(25))) + 4 * (size_t)((n_ent + 32) / 32);
    const size_t budget = (size_t)1 << (10 + rnd(17));
    const int forced = rnd(3) == 0 ? 1 + rnd(40) : 0;
    const int chunk = kp_probe_chunk(v.n, row_bytes, budget, 16, forced);
    if (v.n == 0) {
      if (chunk != 0) fail("chunk of no probes");
    } else {
      if (chunk < 1 || chunk > v.n) fail("chunk out of [1, n]");
      if (forced && chunk != std::min(v.n, forced)) fail("forced chunk ignored");
      if (!forced && chunk > 1 && (size_t)chunk * row_bytes > budget) fail("chunk over budget");
      if (!forced && chunk >= 16 && chunk < v.n && chunk % 16 != 0) fail("chunk splits a group");
      int covered = 0;
      for (int r0 = 0; r0 < v.n; r0 += chunk) covered += std::min(chunk, v.n - r0);
      if (covered != v.n) fail("chunks do not cover the rows once");
    }
    ++n_sets;
  }
  std::printf("random sets: %d\n", n_sets);
}

}  // namespace

int main() {
  errors();
  rank_rows();
  slot_rows();
  random_sets();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
