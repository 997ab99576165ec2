// marks_check_driver.cpp -- the epoch marks' host check and mark plan
// (kelpie_amd/csrc/kp_marks_check.hpp) alone, plain and under the host sanitizers: `make
// marks_check marks_check_asan` builds this file, tests/test_marks_check.py runs it.
//   * a good request passes; the good request with exactly one rule broken must yield that
//     rule's message;
//   * hand-derived plans: slots of 1, 2 and 3 steps per epoch and an empty slot in one batch,
//     the marks {0}, {E} and all of 0..15, ConvE's pair counts with a last step of one pair;
//   * the marks as rank rows: two slots by two marks, one slot's filter list empty; a filter
//     entry count past 2^31 - 1 and a row count past the bound are refused before anything is
//     read or written;
//   * on 400 pseudo-random batches the plan equals a second, independent statement of the rule.
// The arrays are heap vectors of their exact length, so a plan that reads past one is
// reported.  Prints one line per case and exits 0 iff every case went as expected.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../kelpie_amd/csrc/kp_marks_check.hpp"

namespace {

constexpr int K = 50;  // the kelpie entity's id

int failures = 0;
void fail(const std::string& what) {
  std::printf("FAIL %s\n", what.c_str());
  ++failures;
}
void expect_msg(const std::string& what, const char* got, const char* want) {
  const bool same = (got == nullptr && want == nullptr) || (got && want && std::strcmp(got, want) == 0);
  std::printf("%s: %s\n", what.c_str(), got ? got : "ok");
  if (!same) fail(what + ": expected " + (want ? want : "a good request"));
}

kp_hp make_hp(int epochs, int batch_size) {
  kp_hp hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.epochs = epochs;
  hp.batch_size = batch_size;
  return hp;
}

struct Batch {
  std::vector<int32_t> row_off{0}, rows;
  void slot(const std::vector<std::vector<int>>& rs) {
    for (auto& r : rs) rows.insert(rows.end(), r.begin(), r.end());
    row_off.push_back((int32_t)(rows.size() / 3));
  }
  int slots() const { return (int)row_off.size() - 1; }
};

struct Marks {
  std::vector<int32_t> epochs;
  std::vector<float> score;
  std::vector<int64_t> rank;
  Marks(std::vector<int32_t> e, int n_slots) : epochs(std::move(e)) {
    score.assign(epochs.size() * (size_t)n_slots, 0.f);
    rank.assign(epochs.size() * (size_t)n_slots, 0);
  }
  kp_marks view() { return kp_marks{(int32_t)epochs.size(), epochs.data(), score.data(), rank.data(), nullptr}; }
};

void errors() {
  const kp_hp hp = make_hp(6, 2);
  Marks g({0, 1, 2, 4, 6}, 3);
  {
    const kp_marks m = g.view();
    expect_msg("good", kp_check_marks(&hp, &m), nullptr);
  }
  {
    kp_marks m = g.view();
    m.epochs = nullptr;
    expect_msg("null epochs", kp_check_marks(&hp, &m), "missing epochs");
  }
  {
    kp_marks m = g.view();
    m.n = 0;
    expect_msg("n 0", kp_check_marks(&hp, &m), "n must be in [1, 16]");
    m.n = -3;
    expect_msg("n -3", kp_check_marks(&hp, &m), "n must be in [1, 16]");
  }
  {
    const kp_hp big = make_hp(40, 2);
    std::vector<int32_t> e;
    for (int j = 0; j < 17; ++j) e.push_back(j);
    Marks t(e, 3);
    const kp_marks m = t.view();
    expect_msg("n 17", kp_check_marks(&big, &m), "n must be in [1, 16]");
  }
  {
    Marks t({0, 2, 2, 4}, 3);
    const kp_marks m = t.view();
    expect_msg("repeated", kp_check_marks(&hp, &m), "epochs must be strictly increasing");
    Marks u({0, 3, 2}, 3);
    const kp_marks mu = u.view();
    expect_msg("decreasing", kp_check_marks(&hp, &mu), "epochs must be strictly increasing");
  }
  {
    Marks t({-1, 2}, 3);
    const kp_marks m = t.view();
    expect_msg("negative", kp_check_marks(&hp, &m), "negative epoch");
  }
  {
    Marks t({0, 7}, 3);
    const kp_marks m = t.view();
    expect_msg("beyond", kp_check_marks(&hp, &m), "epoch beyond hp->epochs");
  }
  {
    kp_marks m = g.view();
    m.out_rank = nullptr;
    expect_msg("null out_rank", kp_check_marks(&hp, &m), "missing mark output");
    m = g.view();
    m.out_score = nullptr;
    expect_msg("null out_score", kp_check_marks(&hp, &m), "missing mark output");
  }
  {
    const kp_marks m = g.view();
    expect_msg("null hp", kp_check_marks(nullptr, &m), "missing hyper-parameters");
    const kp_hp neg = make_hp(-1, 2);
    expect_msg("epochs -1", kp_check_marks(&neg, &m), "negative epochs");
  }
  {
    // the plan refuses what the check refuses, and a malformed batch
    Batch b;
    b.slot({{K, 0, 1}});
    Marks t({0, 7}, 1);
    const kp_marks m = t.view();
    KpMarkPlan plan;
    expect_msg("plan: beyond", kp_marks_plan(KP_MODEL_COMPLEX, &hp, 1, b.row_off.data(), b.rows.data(), &m, plan),
               "epoch beyond hp->epochs");
    const kp_marks gm = g.view();
    expect_msg("plan: model 9", kp_marks_plan(9, &hp, 1, b.row_off.data(), b.rows.data(), &gm, plan), "unknown model");
    const kp_hp h0 = make_hp(6, 0);
    expect_msg("plan: batch_size 0", kp_marks_plan(KP_MODEL_COMPLEX, &h0, 1, b.row_off.data(), b.rows.data(), &gm, plan),
               "batch_size must be positive");
  }
}

// slot 0: six rows, four distinct (h, r) pairs; slot 1: empty; slot 2: four rows, three pairs;
// slot 3: two rows, one pair
Batch mixed() {
  Batch b;
  b.slot({{K, 0, 1}, {K, 0, 2}, {K, 1, 1}, {3, 2, K}, {3, 2, K}, {4, 2, K}});
  b.slot({});
  b.slot({{K, 0, 1}, {K, 1, 2}, {K, 1, 1}, {5, 0, K}});
  b.slot({{K, 0, 1}, {K, 0, 2}});
  return b;
}

void expect_plan(const std::string& what, int model, int epochs, int bs, const std::vector<int32_t>& marks,
                 const std::vector<int32_t>& want_steps, int want_T,
                 const std::vector<std::vector<std::pair<int, int>>>& want_cap) {
  Batch b = mixed();
  const kp_hp hp = make_hp(epochs, bs);
  Marks mk(marks, b.slots());
  const kp_marks m = mk.view();
  KpMarkPlan plan;
  const char* why = kp_marks_plan(model, &hp, b.slots(), b.row_off.data(), b.rows.data(), &m, plan);
  bool ok = !why && plan.n == (int)marks.size() && plan.T == want_T && plan.slot_step == want_steps &&
            (int)plan.step_off.size() == want_T + 1 && (int)want_cap.size() == want_T;
  for (int t = 0; ok && t < want_T; ++t) {
    const int i0 = plan.step_off[t], i1 = plan.step_off[t + 1];
    ok = i1 - i0 == (int)want_cap[t].size();
    for (int i = i0; ok && i < i1; ++i)
      ok = plan.cap[2 * (size_t)i] == want_cap[t][i - i0].first && plan.cap[2 * (size_t)i + 1] == want_cap[t][i - i0].second &&
           kp_marks_row_at(plan, want_cap[t][i - i0].first, t) == want_cap[t][i - i0].second;
  }
  for (int s = 0; ok && s < b.slots(); ++s)
    for (int t = 0; ok && t < want_T; ++t) {
      bool listed = false;
      for (auto& pr : want_cap[t]) listed |= pr.first == s;
      if (!listed) ok = kp_marks_row_at(plan, s, t) == -1;
    }
  std::printf("%s: %s\n", what.c_str(), why ? why : (ok ? "ok" : "wrong plan"));
  if (!ok) fail(what);
}

void hand_plans() {
  // rows, batch size 2: slot 0 takes 3 steps per epoch, slot 1 none, slot 2 two, slot 3 one;
  // 2 epochs, marks {0, 1, 2}: mark row = slot * 3 + j
  for (int model : {KP_MODEL_COMPLEX, KP_MODEL_DISTMULT, KP_MODEL_TRANSE})
    expect_plan("rows model " + std::to_string(model) + " 3/0/2/1 steps", model, 2, 2, {0, 1, 2},
                {0, 3, 6, 0, 0, 0, 0, 2, 4, 0, 1, 2}, 6,
                {{{3, 10}}, {{2, 7}, {3, 11}}, {{0, 1}}, {{2, 8}}, {}, {{0, 2}}});
  // the mark {0} alone captures nothing; the mark {E} alone is every slot's last step
  expect_plan("mark {0}", KP_MODEL_COMPLEX, 2, 2, {0}, {0, 0, 0, 0}, 6, {{}, {}, {}, {}, {}, {}});
  expect_plan("mark {E}", KP_MODEL_COMPLEX, 2, 2, {2}, {6, 0, 4, 2}, 6, {{}, {{3, 3}}, {}, {{2, 2}}, {}, {{0, 0}}});
  expect_plan("no epoch", KP_MODEL_COMPLEX, 0, 2, {0}, {0, 0, 0, 0}, 0, {});
  // ConvE counts (head, relation) pairs: 4, 0, 3 and 1 pairs; batch size 3 leaves slot 0 a
  // last step of one pair (2 steps per epoch), slots 2 and 3 one step per epoch
  expect_plan("pairs bs 3", KP_MODEL_CONVE, 3, 3, {1, 3}, {2, 6, 0, 0, 1, 3, 1, 3}, 6,
              {{{2, 4}, {3, 6}}, {{0, 0}}, {{2, 5}, {3, 7}}, {}, {}, {{0, 1}}});
  // batch size 2: 2, 0, 2 (a last step of one pair) and 1 steps per epoch
  expect_plan("pairs bs 2", KP_MODEL_CONVE, 2, 2, {0, 2}, {0, 4, 0, 0, 0, 4, 0, 2}, 4,
              {{}, {{3, 7}}, {}, {{0, 1}, {2, 5}}});
  {
    // all of 0 .. 15 on one-step slots: mark j is captured by step j - 1
    std::vector<int32_t> marks, steps;
    std::vector<std::vector<std::pair<int, int>>> cap(15);
    for (int j = 0; j < 16; ++j) marks.push_back(j);
    for (int s = 0; s < 4; ++s)
      for (int j = 0; j < 16; ++j) steps.push_back(s == 1 ? 0 : j);
    for (int t = 0; t < 15; ++t)
      for (int s : {0, 2, 3}) cap[t].push_back({s, s * 16 + t + 1});
    expect_plan("marks 0..15", KP_MODEL_TRANSE, 15, 100, marks, steps, 15, cap);
  }
}

// the marks as rank rows (kp_mark_rows): row s * nm + j is (row, p, o) of slot s with a copy of
// the slot's filter list
void rank_rows() {
  const std::vector<int32_t> pred{K, 3, 7, K, 1, K}, filt_off{0, 0, 2}, filt{4, 9};  // slot 0: no filter entry
  std::vector<int32_t> trip{99}, po{99}, fo{99}, f;
  const char* why = kp_mark_rows(2, 2, pred.data(), filt_off.data(), filt.data(), trip, po, fo, f);
  bool ok = !why && trip == std::vector<int32_t>{0, 3, 7, 1, 3, 7, 2, 1, K, 3, 1, K} &&
            po == std::vector<int32_t>{7, 7, K, K} && fo == std::vector<int32_t>{0, 0, 0, 2, 4} &&
            f == std::vector<int32_t>{4, 9, 4, 9};
  std::printf("rows 2 x 2, one empty filter: %s\n", why ? why : (ok ? "ok" : "wrong rows"));
  if (!ok) fail("rows 2 x 2");
  // no filter entry at all: `f` still holds one (zero) entry to upload
  const std::vector<int32_t> none{0, 0, 0};
  why = kp_mark_rows(2, 2, pred.data(), none.data(), nullptr, trip, po, fo, f);
  ok = !why && fo == std::vector<int32_t>{0, 0, 0, 0, 0} && f == std::vector<int32_t>{0};
  std::printf("rows without a filter: %s\n", why ? why : (ok ? "ok" : "wrong rows"));
  if (!ok) fail("rows without a filter");
  // 16 marks of two slots whose lists hold 2^27 entries each: 2^32 entries.  The offsets alone
  // say so: there is no filter array behind them, and the outputs stay as they were
  const std::vector<int32_t> huge{0, 1 << 27, 1 << 28};
  trip = {99};
  expect_msg("rows: 2^32 filter entries", kp_mark_rows(2, 16, pred.data(), huge.data(), nullptr, trip, po, fo, f),
             "the mark rows' filter lists exceed 2^31 - 1 entries");
  // two marks of one slot of 2^30 entries: 2^31, one more than fits
  const std::vector<int32_t> edge{0, 1 << 30, 1 << 30};
  expect_msg("rows: 2^31 filter entries", kp_mark_rows(2, 2, pred.data(), edge.data(), nullptr, trip, po, fo, f),
             "the mark rows' filter lists exceed 2^31 - 1 entries");
  if (trip != std::vector<int32_t>{99}) fail("rows: a refused call wrote its outputs");
  expect_msg("rows: too many", kp_mark_rows(INT32_MAX / 4 / 16 + 1, 16, pred.data(), huge.data(), nullptr, trip, po, fo, f),
             "too many mark rows");
}

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

void random_batches() {
  int n = 0;
  for (int it = 0; it < 400; ++it) {
    Batch b;
    const int ns = 1 + rnd() % 6;
    for (int s = 0; s < ns; ++s) {
      std::vector<std::vector<int>> rs;
      const int R = rnd() % 4 == 0 ? 0 : 1 + rnd() % 40;
      for (int j = 0; j < R; ++j) {
        const int e = rnd() % K, r = rnd() % 5;
        if (rnd() % 2) rs.push_back({K, r, e});
        else rs.push_back({e, r, K});
      }
      b.slot(rs);
    }
    const int model = rnd() % 4;
    const kp_hp hp = make_hp(rnd() % 9, 1 + rnd() % 17);
    std::vector<int32_t> ep;
    for (int e = 0; e <= hp.epochs && (int)ep.size() < 16; ++e)
      if (rnd() % 2) ep.push_back(e);
    if (ep.empty()) ep.push_back(hp.epochs);
    Marks mk(ep, ns);
    const kp_marks m = mk.view();
    KpMarkPlan plan;
    if (kp_marks_plan(model, &hp, ns, b.row_off.data(), b.rows.data(), &m, plan)) {
      fail("random: refused");
      continue;
    }
    // the rule, stated a second time: walk every slot's epochs step by step
    const int nm = (int)ep.size();
    std::map<int, std::vector<std::pair<int, int>>> at;  // global step -> (slot, row)
    int T = 0;
    bool ok = plan.n == nm;
    for (int s = 0; s < ns; ++s) {
      std::set<std::pair<int, int>> pairs;
      int cnt = b.row_off[s + 1] - b.row_off[s];
      for (int j = b.row_off[s]; j < b.row_off[s + 1]; ++j) pairs.insert({b.rows[3 * j], b.rows[3 * j + 1]});
      if (model == KP_MODEL_CONVE) cnt = (int)pairs.size();
      int step = 0;
      for (int j = 0; j < nm; ++j)
        if (ep[j] == 0) ok &= plan.slot_step[(size_t)s * nm + j] == 0;
      for (int e = 1; e <= hp.epochs; ++e) {
        for (int left = cnt; left > 0; left -= hp.batch_size) ++step;
        for (int j = 0; j < nm; ++j)
          if (ep[j] == e) {
            ok &= plan.slot_step[(size_t)s * nm + j] == step;
            if (step > 0) at[step - 1].push_back({s, s * nm + j});
          }
      }
      T = std::max(T, step);
    }
    ok &= plan.T == T && (int)plan.step_off.size() == T + 1;
    for (int t = 0; ok && t < T; ++t) {
      const std::vector<std::pair<int, int>>& want = at[t];
      ok &= plan.step_off[t + 1] - plan.step_off[t] == (int)want.size();
      for (int i = 0; ok && i < (int)want.size(); ++i) {
        const size_t k = (size_t)plan.step_off[t] + i;
        ok &= plan.cap[2 * k] == want[i].first && plan.cap[2 * k + 1] == want[i].second;
      }
    }
    if (ok) ok &= plan.cap.size() == 2 * (size_t)plan.step_off[T];
    if (!ok) fail("random: plan of batch " + std::to_string(it));
    ++n;
  }
  std::printf("random batches: %d\n", n);
}

}  // namespace

int main() {
  errors();
  hand_plans();
  rank_rows();
  random_batches();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
