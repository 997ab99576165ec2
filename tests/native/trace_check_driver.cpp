// trace_check_driver.cpp -- the post-training trace's step counts and host check
// (kelpie_amd/csrc/kp_trace_check.hpp) alone, plain and under the host sanitizers: `make
// trace_check trace_check_asan` builds this file, tests/test_trace_check.py runs it.
//   * hand-derived counts: every model family, an empty slot, epochs == 0, a last step of
//     one row, ConvE's distinct (head, relation) pairs;
//   * a good trace passes; the good trace with exactly one rule broken must yield that
//     rule's message;
//   * on 400 pseudo-random batches the counts equal a second, independent statement of the
//     rule, their prefix sums pass the check and every single offset moved by one fails it.
// The arrays are heap vectors of their exact length, so a check that reads past one is
// reported.  Prints one line per case and exits 0 iff every case went as expected.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../kelpie_amd/csrc/kp_trace_check.hpp"

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
  if (!same) fail(what + ": expected " + (want ? want : "a good trace"));
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

// slot 0: seven rows, four distinct (h, r) pairs; slot 1: empty; slot 2: three rows, two pairs
Batch good() {
  Batch b;
  b.slot({{K, 0, 1}, {K, 0, 2}, {K, 1, 1}, {3, 2, K}, {3, 2, K}, {4, 2, K}, {K, 0, K}});
  b.slot({});
  b.slot({{K, 0, 1}, {K, 0, 2}, {K, 1, 1}});
  return b;
}

void expect_counts(const std::string& what, int model, int epochs, int bs, const std::vector<int32_t>& want) {
  Batch b = good();
  const kp_hp hp = make_hp(epochs, bs);
  std::vector<int32_t> got(b.slots(), -1);
  const char* why = kp_trace_steps_host(model, &hp, b.slots(), b.row_off.data(), b.rows.data(), got.data());
  std::printf("%s: %s\n", what.c_str(), why ? why : (got == want ? "ok" : "wrong counts"));
  if (why || got != want) fail(what);
}

void hand_counts() {
  for (int model : {KP_MODEL_COMPLEX, KP_MODEL_DISTMULT, KP_MODEL_TRANSE}) {
    const std::string m = "rows model " + std::to_string(model);
    expect_counts(m + " bs 2", model, 3, 2, {12, 0, 6});  // ceil(7 / 2) = 4, ceil(3 / 2) = 2
    expect_counts(m + " bs 6", model, 3, 6, {6, 0, 3});   // R = batch_size + 1: a last step of one row
    expect_counts(m + " bs 7", model, 3, 7, {3, 0, 3});   // R = batch_size
    expect_counts(m + " bs 100", model, 5, 100, {5, 0, 5});
    expect_counts(m + " no epoch", model, 0, 2, {0, 0, 0});
  }
  expect_counts("pairs bs 2", KP_MODEL_CONVE, 3, 2, {6, 0, 3});  // 4 pairs, 2 pairs
  expect_counts("pairs bs 3", KP_MODEL_CONVE, 3, 3, {6, 0, 3});  // a last step of one pair
  expect_counts("pairs bs 4", KP_MODEL_CONVE, 5, 4, {5, 0, 5});
  expect_counts("pairs no epoch", KP_MODEL_CONVE, 0, 4, {0, 0, 0});
}

struct Trace {
  std::vector<int32_t> off;
  std::vector<float> loss;
  kp_trace view() { return kp_trace{off.data(), loss.empty() ? nullptr : loss.data()}; }
};
Trace trace_of(const std::vector<int32_t>& steps) {
  Trace t;
  t.off.push_back(0);
  for (int32_t s : steps) t.off.push_back(t.off.back() + s);
  t.loss.assign((size_t)t.off.back(), 0.f);
  return t;
}

void errors() {
  Batch b = good();
  const kp_hp hp = make_hp(3, 2);
  auto check = [&](const kp_hp* h, const kp_trace& tr) {
    return kp_check_trace(KP_MODEL_COMPLEX, h, b.slots(), b.row_off.data(), b.rows.data(), &tr);
  };
  Trace g = trace_of({12, 0, 6});
  expect_msg("good", check(&hp, g.view()), nullptr);
  {
    Trace z = trace_of({0, 0, 0});  // nothing to write: out_loss may be NULL
    const kp_hp h0 = make_hp(0, 2);
    expect_msg("no step, null out_loss", check(&h0, z.view()), nullptr);
  }
  {
    kp_trace tr = g.view();
    tr.trace_off = nullptr;
    expect_msg("null trace_off", check(&hp, tr), "missing trace_off");
  }
  {
    Trace t = g;
    t.off[0] = 1;
    expect_msg("start", check(&hp, t.view()), "trace_off must start at 0");
  }
  for (int s = 1; s <= 3; ++s)
    for (int dlt : {-1, 1}) {
      Trace t = g;
      t.off[s] += dlt;
      expect_msg("offset " + std::to_string(s) + (dlt < 0 ? " - 1" : " + 1"), check(&hp, t.view()),
                 "trace_off disagrees with kp_trace_steps");
    }
  {
    // the counts of another family's rule (ConvE's pairs) are not this model's
    Trace t = trace_of({6, 0, 3});
    expect_msg("pairs' counts", check(&hp, t.view()), "trace_off disagrees with kp_trace_steps");
  }
  {
    kp_trace tr = g.view();
    tr.out_loss = nullptr;
    expect_msg("null out_loss", check(&hp, tr), "missing out_loss");
  }
  {
    const kp_hp h = make_hp(3, 0);
    expect_msg("batch_size 0", check(&h, g.view()), "batch_size must be positive");
    const kp_hp h2 = make_hp(-1, 2);
    expect_msg("epochs -1", check(&h2, g.view()), "negative epochs");
    expect_msg("null hp", check(nullptr, g.view()), "missing hyper-parameters");
  }
  {
    const kp_trace tr = g.view();
    expect_msg("model 9", kp_check_trace(9, &hp, b.slots(), b.row_off.data(), b.rows.data(), &tr), "unknown model");
    expect_msg("slots -1", kp_check_trace(KP_MODEL_COMPLEX, &hp, -1, b.row_off.data(), b.rows.data(), &tr),
               "negative n_slots");
    expect_msg("null row_off", kp_check_trace(KP_MODEL_COMPLEX, &hp, b.slots(), nullptr, b.rows.data(), &tr),
               "missing row_off");
    expect_msg("null rows", kp_check_trace(KP_MODEL_COMPLEX, &hp, b.slots(), b.row_off.data(), nullptr, &tr),
               "missing rows");
    Batch c = good();
    c.row_off[0] = 1;
    expect_msg("row_off start", kp_check_trace(KP_MODEL_COMPLEX, &hp, c.slots(), c.row_off.data(), c.rows.data(), &tr),
               "row_off must start at 0");
    Batch d = good();
    d.row_off[2] = 3;
    expect_msg("row_off order", kp_check_trace(KP_MODEL_COMPLEX, &hp, d.slots(), d.row_off.data(), d.rows.data(), &tr),
               "row_off decreases");
    std::vector<int32_t> steps(3);
    expect_msg("null out_steps", kp_trace_steps_host(KP_MODEL_COMPLEX, &hp, 3, b.row_off.data(), b.rows.data(), nullptr),
               "missing out_steps");
    // 2^31 steps and more are refused, not wrapped
    const kp_hp big = make_hp(INT32_MAX, 1);
    expect_msg("too many steps", kp_trace_steps_host(KP_MODEL_COMPLEX, &big, 3, b.row_off.data(), b.rows.data(),
                                                     steps.data()),
               "more than 2^31 - 1 steps");
  }
  {
    // no slot at all: nothing is read
    const kp_trace tr{g.off.data(), nullptr};
    expect_msg("no slots", kp_check_trace(KP_MODEL_TRANSE, &hp, 0, nullptr, nullptr, &tr), nullptr);
  }
}

uint32_t rng_state = 12345;
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
    const kp_hp hp = make_hp(rnd() % 6, 1 + rnd() % 17);
    std::vector<int32_t> steps(ns, -1);
    if (kp_trace_steps_host(model, &hp, ns, b.row_off.data(), b.rows.data(), steps.data())) {
      fail("random: refused");
      continue;
    }
    // the rule, stated a second time
    for (int s = 0; s < ns; ++s) {
      std::set<std::pair<int, int>> pairs;
      int cnt = b.row_off[s + 1] - b.row_off[s];
      for (int j = b.row_off[s]; j < b.row_off[s + 1]; ++j) pairs.insert({b.rows[3 * j], b.rows[3 * j + 1]});
      if (model == KP_MODEL_CONVE) cnt = (int)pairs.size();
      int per_epoch = 0;
      for (int left = cnt; left > 0; left -= hp.batch_size) ++per_epoch;
      if (steps[s] != hp.epochs * per_epoch) fail("random: count of slot " + std::to_string(s));
    }
    Trace t = trace_of(steps);
    const kp_trace tv = t.view();
    if (kp_check_trace(model, &hp, ns, b.row_off.data(), b.rows.data(), &tv)) fail("random: good trace refused");
    for (int s = 1; s <= ns; ++s) {
      Trace u = t;
      u.off[s] += (rnd() % 2) ? 1 : -1;
      u.loss.assign((size_t)std::max(1, u.off.back() + 2), 0.f);
      const kp_trace v = u.view();
      const char* why = kp_check_trace(model, &hp, ns, b.row_off.data(), b.rows.data(), &v);
      if (!why || std::strcmp(why, "trace_off disagrees with kp_trace_steps") != 0) fail("random: moved offset accepted");
    }
    ++n;
  }
  std::printf("random batches: %d\n", n);
}

}  // namespace

int main() {
  hand_counts();
  errors();
  random_batches();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
