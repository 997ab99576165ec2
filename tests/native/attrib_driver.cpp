// attrib_driver.cpp -- the attributions' request check (kelpie_amd/csrc/kp_attrib_check.hpp)
// and the step plan's row map (kelpie_amd/csrc/kp_cx_rowmap.hpp) alone, plain and under the
// host sanitizers: `make attrib attrib_asan` builds this file, tests/test_attrib_check.py runs it.
//   * good requests pass; the good request with exactly one rule broken must yield that rule's
//     message and code, and with two rules broken the earlier one;
//   * the row map of two hand-written batches against hand-derived maps: a single-step slot
//     with a repeated relation, a repeated pair, a self-loop and a duplicate row beside an empty
//     slot, and a multi-step slot whose minibatches come from its permutations;
//   * on pseudo-random batches the map's index invariants: every row of a minibatch appears
//     exactly once in its plan's lists, under the item (relation, pair, frozen target) it belongs
//     to, and the lists' lengths are the plan's counts.
// Prints one line per case and exits 0 iff every case went as expected.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../kelpie_amd/csrc/kp_attrib_check.hpp"
#include "../../kelpie_amd/csrc/kp_cx_rowmap.hpp"

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
void expect_vec(const std::string& what, const std::vector<int32_t>& got, const std::vector<int32_t>& want) {
  const bool same = got == want;
  std::printf("%s: %s\n", what.c_str(), same ? "ok" : "differs");
  if (!same) {
    std::printf("  got ");
    for (int v : got) std::printf(" %d", v);
    std::printf("\n  want");
    for (int v : want) std::printf(" %d", v);
    std::printf("\n");
    fail(what);
  }
}

const char* LINEAR = "attributions serve ComplEx and DistMult only (the score must be linear in the row)";
const char* ADAM = "attributions are not offered with Adam (Adagrad and SGD only)";
const char* QUAD = "the tail of a slot's pred is the kelpie entity (its score is quadratic in the row)";

void errors() {
  const int n_ent = 50;
  const std::vector<int32_t> row_off = {0, 4, 4, 10};
  const std::vector<int32_t> pred = {50, 1, 7, 50, 2, 8, 50, 3, 9};
  std::vector<double> fit(10), reg(10), delta(3);
  kp_hp hp{};
  hp.optimizer = KP_OPT_ADAGRAD;
  const auto good = [&] { return kp_attrib{fit.data(), reg.data(), delta.data()}; };
  const auto check = [&](const std::string& what, int model, const kp_hp& h, int ns, const int32_t* ro,
                         const std::vector<int32_t>& pr, const kp_attrib* a, const char* want, int want_code) {
    int code = 0;
    const char* got = kp_check_attrib(model, &h, n_ent, ns, ro, pr.data(), a, &code);
    expect_msg(what, got, code, want, want_code);
  };
  kp_attrib g = good();
  check("good: ComplEx Adagrad", KP_MODEL_COMPLEX, hp, 3, row_off.data(), pred, &g, nullptr, 0);
  check("good: DistMult", KP_MODEL_DISTMULT, hp, 3, row_off.data(), pred, &g, nullptr, 0);
  {
    kp_hp sgd = hp;
    sgd.optimizer = KP_OPT_SGD;
    check("good: SGD", KP_MODEL_COMPLEX, sgd, 3, row_off.data(), pred, &g, nullptr, 0);
  }
  {
    const std::vector<int32_t> none = {0, 0};
    kp_attrib d{nullptr, nullptr, delta.data()};
    check("good: no rows, delta alone", KP_MODEL_COMPLEX, hp, 1, none.data(), pred, &d, nullptr, 0);
    kp_attrib e{};
    check("good: no slots", KP_MODEL_COMPLEX, hp, 0, nullptr, pred, &e, nullptr, 0);
  }
  check("null request", KP_MODEL_COMPLEX, hp, 3, row_off.data(), pred, nullptr, "missing request", KP_EINVAL);
  g = good(), g.out_fit = nullptr;
  check("null out_fit", KP_MODEL_COMPLEX, hp, 3, row_off.data(), pred, &g, "missing out_fit or out_reg", KP_EINVAL);
  g = good(), g.out_reg = nullptr;
  check("null out_reg", KP_MODEL_COMPLEX, hp, 3, row_off.data(), pred, &g, "missing out_fit or out_reg", KP_EINVAL);
  g = good(), g.out_delta = nullptr;
  check("null out_delta", KP_MODEL_COMPLEX, hp, 3, row_off.data(), pred, &g, "missing out_delta", KP_EINVAL);
  g = good();
  check("TransE", KP_MODEL_TRANSE, hp, 3, row_off.data(), pred, &g, LINEAR, KP_ENOTSUP);
  check("ConvE", KP_MODEL_CONVE, hp, 3, row_off.data(), pred, &g, LINEAR, KP_ENOTSUP);
  kp_hp adam = hp;
  adam.optimizer = KP_OPT_ADAM;
  check("Adam", KP_MODEL_COMPLEX, adam, 3, row_off.data(), pred, &g, ADAM, KP_ENOTSUP);
  std::vector<int32_t> loop = pred;
  loop[5] = n_ent;
  check("kelpie tail", KP_MODEL_DISTMULT, hp, 3, row_off.data(), loop, &g, QUAD, KP_ENOTSUP);
  // the first rule broken is the one reported
  g.out_fit = nullptr;
  check("null out_fit on TransE", KP_MODEL_TRANSE, hp, 3, row_off.data(), pred, &g, "missing out_fit or out_reg",
        KP_EINVAL);
  g = good();
  check("TransE with Adam", KP_MODEL_TRANSE, adam, 3, row_off.data(), pred, &g, LINEAR, KP_ENOTSUP);
  check("Adam with a kelpie tail", KP_MODEL_COMPLEX, adam, 3, row_off.data(), loop, &g, ADAM, KP_ENOTSUP);
}

struct Batch {
  std::vector<int32_t> row_off, rows, rng;
  std::vector<int64_t> rng_off;
  kp_batch view() {
    kp_batch b{};
    b.n_slots = (int)row_off.size() - 1;
    b.row_off = row_off.data();
    b.rows = rows.data();
    b.rng_off = rng_off.data();
    b.rng = rng.data();
    return b;
  }
};

void hand_maps() {
  const int K = 20, n_rel2 = 8;
  {
    // slot 0: one step (batch_size 16).  rows 0..7:
    //   0 (K,1,3)  1 (K,2,5)  2 (K,1,4)  3 (6,5,K)  4 (K,1,K)  5 (K,1,3)  6 (6,5,K)  7 (7,6,K)
    // slot 1 is empty; slot 2: rows 8, 9 = (K,2,9), (9,6,K)
    Batch b;
    b.row_off = {0, 8, 8, 10};
    b.rows = {K, 1, 3, K, 2, 5, K, 1, 4, 6, 5, K, K, 1, K, K, 1, 3, 6, 5, K, 7, 6, K, K, 2, 9, 9, 6, K};
    b.rng_off = {0, 0, 0, 0};
    b.rng = {0};
    kp_batch bt = b.view();
    CxStepPlan sp;
    CxRowMap m;
    const char* why = cx_step_plan(K, n_rel2, 16, 3, &bt, sp);
    if (!why) why = cx_row_map(K, 16, 3, &bt, sp, m);
    expect_msg("hand single-step: map", why, 0, nullptr, 0);
    // plan 0: queries rel 1 (targets 3, 4, 3; one kelpie target), rel 2 (target 5); tails (6,5) x2, (7,6)
    expect_vec("hand single-step: targets", sp.targets, {3, 4, 3, 5, 9});
    expect_vec("hand single-step: tg_row", m.tg_row, {0, 2, 5, 1, 8});
    expect_vec("hand single-step: qk_off", m.qk_off, {0, 1, 1, 1});
    expect_vec("hand single-step: qk_row", m.qk_row, {4});
    expect_vec("hand single-step: t_off", m.t_off, {0, 2, 3, 4});
    expect_vec("hand single-step: t_row", m.t_row, {3, 6, 7, 9});
  }
  {
    // one slot of 5 rows, batch_size 2, 2 epochs: 3 minibatches per epoch from the permutations
    //   0 (K,1,3)  1 (K,1,4)  2 (5,2,K)  3 (K,3,K)  4 (5,2,K)
    Batch b;
    b.row_off = {0, 5};
    b.rows = {K, 1, 3, K, 1, 4, 5, 2, K, K, 3, K, 5, 2, K};
    b.rng_off = {0, 10};
    b.rng = {4, 0, 1, 2, 3, /* epoch 1 */ 3, 2, 4, 1, 0};
    kp_batch bt = b.view();
    CxStepPlan sp;
    CxRowMap m;
    const char* why = cx_step_plan(K, n_rel2, 2, 2, &bt, sp);
    if (!why) why = cx_row_map(K, 2, 2, &bt, sp, m);
    expect_msg("hand multi-step: map", why, 0, nullptr, 0);
    // minibatches: {4,0} {1,2} {3} | {3,2} {4,1} {0}
    //   queries:   rel1      rel1     rel3   rel3       rel1     rel1
    //   tails:     (5,2)     (5,2)    -      (5,2)      (5,2)    -
    expect_vec("hand multi-step: tg_row", m.tg_row, {0, 1, 1, 0});
    expect_vec("hand multi-step: qk_off", m.qk_off, {0, 0, 0, 1, 2, 2, 2});
    expect_vec("hand multi-step: qk_row", m.qk_row, {3, 3});
    expect_vec("hand multi-step: t_off", m.t_off, {0, 1, 2, 3, 4});
    expect_vec("hand multi-step: t_row", m.t_row, {4, 2, 2, 4});
    // a plan that is not this batch's is refused, not indexed
    CxRowMap other;
    why = cx_row_map(K, 3, 2, &bt, sp, other);
    std::printf("hand multi-step: another batch_size: %s\n", why ? "refused" : "accepted");
    if (!why) fail("hand multi-step: another batch_size");
  }
}

void random_batches() {
  unsigned long long x = 0x9E3779B97F4A7C15ull;
  const auto next = [&](int n) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return (int)((x >> 11) % (unsigned long long)n);
  };
  int batches = 0, rows_seen = 0;
  for (int it = 0; it < 200; ++it) {
    const int K = 5 + next(30), n_rel2 = 2 + next(6), ns = 1 + next(4), bs = 1 + next(9), epochs = next(4);
    Batch b;
    b.row_off = {0};
    b.rng_off = {0};
    for (int s = 0; s < ns; ++s) {
      const int R = next(14);
      for (int i = 0; i < R; ++i) {
        const int kind = next(4);  // head, head, tail, self-loop
        const int e = next(K), r = next(n_rel2);
        const int h = kind == 2 ? e : K, t = kind == 2 || kind == 3 ? K : e;
        b.rows.insert(b.rows.end(), {h, r, t});
      }
      b.row_off.push_back(b.row_off.back() + R);
      for (int e = 0; e < epochs; ++e) {
        std::vector<int32_t> perm(R);
        for (int i = 0; i < R; ++i) perm[i] = i;
        for (int i = R - 1; i > 0; --i) std::swap(perm[i], perm[next(i + 1)]);
        b.rng.insert(b.rng.end(), perm.begin(), perm.end());
      }
      b.rng_off.push_back((int64_t)b.rng.size());
    }
    if (b.rows.empty()) b.rows.push_back(0);
    if (b.rng.empty()) b.rng.push_back(0);
    kp_batch bt = b.view();
    CxStepPlan sp;
    CxRowMap m;
    const char* why = cx_step_plan(K, n_rel2, bs, epochs, &bt, sp);
    if (!why) why = cx_row_map(K, bs, epochs, &bt, sp, m);
    if (why) {
      fail(std::string("random batch ") + std::to_string(it) + ": " + why);
      continue;
    }
    ++batches;
    const std::string tag = "random batch " + std::to_string(it);
    if (m.tg_row.size() != sp.targets.size() || m.qk_off.size() != sp.pqs.size() + 1 ||
        m.t_off.size() != sp.pts.size() + 1 || (int)m.qk_row.size() != m.qk_off.back() ||
        (int)m.t_row.size() != m.t_off.back()) {
      fail(tag + ": sizes");
      continue;
    }
    const int total = b.row_off.back();
    // every plan: its lists hold b distinct rows of its slot, each under its own item
    int plan = 0;
    for (int s = 0; s < ns; ++s) {
      const int r0 = b.row_off[s], R = b.row_off[s + 1] - r0;
      if (R == 0 || epochs == 0) continue;
      const int nst = (R + bs - 1) / bs, nplans = nst == 1 ? 1 : epochs * nst;
      for (int pi = 0; pi < nplans; ++pi, ++plan) {
        const CxPlan& P = sp.plans[plan];
        std::vector<int> seen(total, 0);
        int count = 0;
        const auto row_is = [&](int row, int h, int r, int t) {
          if (row < r0 || row >= r0 + R) return false;
          ++seen[row], ++count;
          const int32_t* rw = &b.rows[3 * (size_t)row];
          return rw[0] == h && rw[1] == r && rw[2] == t;
        };
        bool good = true;
        for (int j = P.q_begin; j < P.q_begin + P.q_count; ++j) {
          const CxQuery& Q = sp.pqs[j];
          good = good && m.qk_off[j + 1] - m.qk_off[j] == Q.ck && Q.c == Q.ck + Q.tg_count;
          for (int i = 0; i < Q.tg_count; ++i)
            good = good && row_is(m.tg_row[Q.tg_begin + i], K, Q.rel, sp.targets[Q.tg_begin + i]);
          for (int i = m.qk_off[j]; i < m.qk_off[j + 1]; ++i) good = good && row_is(m.qk_row[i], K, Q.rel, K);
        }
        for (int j = P.t_begin; j < P.t_begin + P.t_count; ++j) {
          const CxI2 hr = sp.pairs[sp.pts[j].pair];
          good = good && m.t_off[j + 1] - m.t_off[j] == sp.pts[j].c;
          for (int i = m.t_off[j]; i < m.t_off[j + 1]; ++i) good = good && row_is(m.t_row[i], hr.x, hr.y, K);
        }
        good = good && count == P.b;
        for (int v : seen) good = good && v <= 1;
        if (!good) fail(tag + ": plan " + std::to_string(plan));
        rows_seen += count;
      }
    }
    if (plan != (int)sp.plans.size()) fail(tag + ": plan count");
  }
  std::printf("random batches: %d\n", batches);
  std::printf("random rows: %s\n", rows_seen > 1000 ? "many" : "few");
}

}  // namespace

int main() {
  errors();
  hand_maps();
  random_batches();
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
