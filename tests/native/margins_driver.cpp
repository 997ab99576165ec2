// margins_driver.cpp -- the rank margins' request check and threshold rule
// (kelpie_amd/csrc/kp_margins_check.hpp) alone, plain and under the host sanitizers: `make
// margins margins_asan` builds this file, tests/test_margins_check.py runs it.
//   * a good request passes; the good request with exactly one rule broken must yield that
//     rule's message and code;
//   * the threshold rule per kind of compared value against hand-computed values: tol == 0
//     gives c_t itself (the same bits, also where sqrt(c)^2 != c), the L2 lower threshold is
//     clamped at 0, delta is relative above a score of 1 and absolute below;
//   * an L2 delta below the rounding of the root leaves both thresholds at c_t;
//   * on 2,000 pseudo-random rows thr_lo is never a worse value than c_t and thr_hi never a
//     better one, and the thresholds of a larger tol enclose those of a smaller.
// Prints one line per case and exits 0 iff every case went as expected.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../kelpie_amd/csrc/kp_margins_check.hpp"

namespace {

int failures = 0;
void fail(const std::string& what) {
  std::printf("FAIL %s\n", what.c_str());
  ++failures;
}
void expect_msg(const std::string& what, const char* got, int code, const char* want, int want_code) {
  const bool same = (got == nullptr && want == nullptr) || (got && want && std::strcmp(got, want) == 0);
  std::printf("%s: %s\n", what.c_str(), got ? got : "ok");
  if (!same) fail(what + ": expected " + (want ? want : "a good request"));
  if (got && code != want_code) fail(what + ": code " + std::to_string(code));
}
void expect_eq(const std::string& what, double got, double want) {
  const bool same = std::memcmp(&got, &want, sizeof(double)) == 0;
  std::printf("%s: %s\n", what.c_str(), same ? "ok" : "differs");
  if (!same) {
    std::printf("  got %.17g want %.17g\n", got, want);
    fail(what);
  }
}

// the check of (m, n_probes, n_marks, rank64): the message first, then the code it left
void check(const std::string& what, const kp_margins* m, int n_probes, int n_marks, bool rank64, const char* want,
           int want_code) {
  int code = 0;
  const char* got = kp_check_margins(m, n_probes, n_marks, rank64, &code);
  expect_msg(what, got, code, want, want_code);
}

// the outputs of one kind of rank row, heap vectors of their exact length
struct Out {
  std::vector<int64_t> lo, hi, ties;
  std::vector<double> gb, gw;
  std::vector<int32_t> ib, iw;
  explicit Out(size_t n) : lo(n), hi(n), ties(n), gb(n), gw(n), ib(n), iw(n) {}
  kp_margin_out view() {
    return kp_margin_out{lo.data(), hi.data(), ties.data(), gb.data(), gw.data(), ib.data(), iw.data()};
  }
};

void errors() {
  Out s(3), p(4), m(6);
  const kp_margin_out none{};
  const auto good = [&] { return kp_margins{1e-4, s.view(), p.view(), m.view()}; };
  {
    kp_margins g = good();
    check("good", &g, 4, 2, true, nullptr, 0);
    g.probes = none, g.marks = none;
    check("good: slots alone", &g, 0, 0, true, nullptr, 0);
    g.tol = 0.0;
    check("good: tol 0", &g, 0, 0, true, nullptr, 0);
    g.tol = 1.0;
    check("good: tol 1", &g, 0, 0, true, nullptr, 0);
    g.slots = none;
    g.slots.ties = s.ties.data();
    check("good: ties alone", &g, 0, 0, true, nullptr, 0);
  }
  check("null request", nullptr, 4, 2, true, "missing request", KP_EINVAL);
  {
    kp_margins g = good();
    g.tol = std::numeric_limits<double>::quiet_NaN();
    check("nan tol", &g, 4, 2, true, "tol is NaN", KP_EINVAL);
    g.tol = -1e-300;
    check("negative tol", &g, 4, 2, true, "negative tol", KP_EINVAL);
    g.tol = std::nextafter(1.0, 2.0);
    check("tol above 1", &g, 4, 2, true, "tol above 1", KP_EINVAL);
    g.tol = std::numeric_limits<double>::infinity();
    check("infinite tol", &g, 4, 2, true, "tol above 1", KP_EINVAL);
  }
  {
    kp_margins g = good();
    g.slots.rank_hi = nullptr;
    check("slots: rank_lo alone", &g, 4, 2, true, "rank_lo and rank_hi go together", KP_EINVAL);
    g = good();
    g.probes.rank_lo = nullptr;
    check("probes: rank_hi alone", &g, 4, 2, true, "rank_lo and rank_hi go together", KP_EINVAL);
    g = good();
    g.marks.rank_hi = nullptr;
    check("marks: rank_lo alone", &g, 4, 2, true, "rank_lo and rank_hi go together", KP_EINVAL);
  }
  {
    kp_margins g = good();
    check("probe outputs, no probes", &g, 0, 2, true, "probe outputs without probes", KP_EINVAL);
    check("mark outputs, no marks", &g, 4, 0, true, "mark outputs without marks",
               KP_EINVAL);
    g.probes = none;
    g.probes.id_worse = p.iw.data();
    check("one probe output, no probes", &g, 0, 2, true, "probe outputs without probes", KP_EINVAL);
  }
  {
    kp_margins g = good();
    check("fp32 rank", &g, 4, 2, false, "margins need the fp64 rank (the fp32 rank switch is set)", KP_ENOTSUP);
    g.tol = 2.0;  // a malformed request is told so first
    check("fp32 rank, bad tol", &g, 4, 2, false, "tol above 1", KP_EINVAL);
  }
}

void thresholds() {
  double lo = 0, hi = 0;
  // tol == 0: c_t itself, for every kind; `odd` is a value the square of whose rounded root is another
  double odd = 2.0;
  while (std::sqrt(odd) * std::sqrt(odd) == odd) odd = std::nextafter(odd, 3.0);
  for (int mode : {KP_MG_DOT, KP_MG_SIGMOID, KP_MG_DIST, KP_MG_DIST1}) {
    for (double c : {odd, 0.0, 1e-300, 3.5e7}) {
      kp_margin_thresholds(mode, c, 0.0, &lo, &hi);
      expect_eq("tol 0 mode " + std::to_string(mode) + " c " + std::to_string(c) + " lo", lo, c);
      expect_eq("tol 0 mode " + std::to_string(mode) + " c " + std::to_string(c) + " hi", hi, c);
    }
  }
  kp_margin_thresholds(KP_MG_DOT, -0.5, 0.0, &lo, &hi);
  expect_eq("tol 0 negative score lo", lo, -0.5);
  // maximizers: delta absolute below a score of 1, relative above (0.25 and 4 are exact)
  kp_margin_thresholds(KP_MG_DOT, 0.5, 0.25, &lo, &hi);
  expect_eq("dot 0.5 lo", lo, 0.75);
  expect_eq("dot 0.5 hi", hi, 0.25);
  kp_margin_thresholds(KP_MG_SIGMOID, -4.0, 0.25, &lo, &hi);
  expect_eq("logit -4 lo", lo, -3.0);
  expect_eq("logit -4 hi", hi, -5.0);
  // L1: the better side is below
  kp_margin_thresholds(KP_MG_DIST1, 8.0, 0.125, &lo, &hi);
  expect_eq("l1 8 lo", lo, 7.0);
  expect_eq("l1 8 hi", hi, 9.0);
  // L2: in distances, squared; c_t = 16 is the distance 4
  kp_margin_thresholds(KP_MG_DIST, 16.0, 0.25, &lo, &hi);
  expect_eq("l2 16 lo", lo, 9.0);
  expect_eq("l2 16 hi", hi, 25.0);
  // L2: delta 0.5 (absolute) past the distance 0.25: the lower threshold is clamped at 0
  kp_margin_thresholds(KP_MG_DIST, 0.0625, 0.5, &lo, &hi);
  expect_eq("l2 clamp lo", lo, 0.0);
  expect_eq("l2 clamp hi", hi, 0.5625);
  kp_margin_thresholds(KP_MG_DIST, 0.0, 1.0, &lo, &hi);
  expect_eq("l2 zero distance lo", lo, 0.0);
  expect_eq("l2 zero distance hi", hi, 1.0);
  // L2: a delta that the root's rounding swallows never carries a threshold across c_t
  for (double c : {odd, 3.0, 1e-9, 7e11}) {
    kp_margin_thresholds(KP_MG_DIST, c, 1e-300, &lo, &hi);
    if (!(lo <= c && c <= hi)) fail("l2 tiny tol crosses c_t at " + std::to_string(c));
  }
  std::printf("l2 tiny tol: checked\n");
  expect_eq("units l2", kp_margin_units(KP_MG_DIST, 16.0), 4.0);
  expect_eq("units l1", kp_margin_units(KP_MG_DIST1, 16.0), 16.0);

  // order and nesting on pseudo-random rows
  unsigned long long x = 0x9E3779B97F4A7C15ull;
  const auto next = [&] {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return (double)(x >> 11) / 9007199254740992.0;
  };
  int rows = 0;
  for (int i = 0; i < 2000; ++i) {
    const int mode = i & 3;
    const bool mini = mode == KP_MG_DIST || mode == KP_MG_DIST1;
    double c = std::ldexp(next(), (int)(next() * 40) - 20);
    if (!mini && (i & 4)) c = -c;
    const double t1 = next() * 1e-3, t2 = t1 + next() * 1e-2;
    double lo1, hi1, lo2, hi2;
    kp_margin_thresholds(mode, c, t1, &lo1, &hi1);
    kp_margin_thresholds(mode, c, t2, &lo2, &hi2);
    const bool ordered = mini ? (lo1 <= c && c <= hi1) : (lo1 >= c && c >= hi1);
    const bool nested = mini ? (lo2 <= lo1 && hi1 <= hi2) : (lo2 >= lo1 && hi1 >= hi2);
    if (!ordered || !nested) fail("random row " + std::to_string(i));
    ++rows;
  }
  std::printf("random rows: %d\n", rows);
}

}  // namespace

int main() {
  errors();
  thresholds();
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
