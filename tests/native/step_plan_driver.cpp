// step_plan_driver.cpp -- the post-training step planners (kelpie_amd/csrc/kp_cx_plan.hpp:
// ComplEx / DistMult, kp_cv_plan.hpp: ConvE) alone, plain and under the host sanitizers:
// `make step_plan step_plan_asan` builds this file, tests/test_step_plan.py runs it.
//   * exact: for a few tiny batches every array of the plan is compared with values written
//     out below, derived by hand from the rules (n_ent = K = 5, n_rel2 = 4);
//   * errors: a good batch with exactly one rule broken must yield that rule's message;
//   * invariants: on a few hundred pseudo-random batches, what the kernels rely on when they
//     index with the plan's values (offsets, ranges, row accounting).
// The batch arrays are heap vectors of their exact length, so a planner that reads past one
// is reported.  Prints one line per case and exits 0 iff every case went as expected.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../kelpie_amd/csrc/kp_cv_plan.hpp"
#include "../../kelpie_amd/csrc/kp_cx_plan.hpp"

namespace {

constexpr int K = 5;  // n_ent; the kelpie entity's id
constexpr int NR = 4;
constexpr int DIM = 20;
using V = std::vector<long long>;

int failures = 0;
void fail(const std::string& what) {
  std::printf("FAIL %s\n", what.c_str());
  ++failures;
}
#define CHECK(cond, what) \
  do {                    \
    if (!(cond)) fail(std::string(what) + ": " #cond); \
  } while (0)

void expect(const std::string& what, const V& got, const V& want) {
  if (got == want) return;
  std::string s = what + ": got [";
  for (long long v : got) s += std::to_string(v) + " ";
  s += "] want [";
  for (long long v : want) s += std::to_string(v) + " ";
  fail(s + "]");
}
void expect_msg(const std::string& what, const char* got, const char* want) {
  const bool same = (got == nullptr && want == nullptr) || (got && want && std::strcmp(got, want) == 0);
  std::printf("%s: %s\n", what.c_str(), got ? got : "ok");
  if (!same) fail(what + ": expected " + (want ? want : "a good plan"));
}

struct Batch {
  std::vector<int32_t> row_off{0}, rows, rng;
  std::vector<int64_t> rng_off{0};
  // one slot: its rows and where its draws end
  void slot(const std::vector<int>& r, int64_t rng_end) {
    rows.insert(rows.end(), r.begin(), r.end());
    row_off.push_back((int32_t)(rows.size() / 3));
    rng_off.push_back(rng_end);
  }
  kp_batch view() const {
    kp_batch b;
    std::memset(&b, 0, sizeof(b));
    b.n_slots = (int32_t)(row_off.size() - 1);
    b.row_off = row_off.data();
    b.rows = rows.data();
    b.rng_off = rng_off.data();
    b.rng = rng.data();
    return b;
  }
};

// ---- the plan arrays, flattened for comparison
V fl(const std::vector<int>& v) { return V(v.begin(), v.end()); }
V fl(const std::vector<CxPlan>& v) {
  V o;
  for (auto& p : v) o.insert(o.end(), {p.b, p.q_begin, p.q_count, p.t_begin, p.t_count, p.cnt_l, p.cnt_r, p.pad});
  return o;
}
V fl(const std::vector<CxQuery>& v) {  // (rel, c, ck, tg_begin, tg_count)
  V o;
  for (auto& q : v) {
    o.insert(o.end(), {q.rel, q.c, q.ck, q.tg_begin, q.tg_count});
    CHECK(q.pad0 == 0 && q.pad1 == 0 && q.pad2 == 0, "query padding");
  }
  return o;
}
V fl(const std::vector<CxTail>& v) {
  V o;
  for (auto& t : v) o.insert(o.end(), {t.pair, t.c});
  return o;
}
template <class I2>
V fl2(const std::vector<I2>& v) {
  V o;
  for (auto& p : v) o.insert(o.end(), {p.x, p.y});
  return o;
}
template <class I4>
V fl4(const std::vector<I4>& v) {
  V o;
  for (auto& p : v) o.insert(o.end(), {p.x, p.y, p.z, p.w});
  return o;
}
V fl(const std::vector<CvInst>& v) {  // (slot, rel, b, pos, in, fm, hid, tail_begin, tail_count)
  V o;
  for (auto& i : v)
    o.insert(o.end(), {i.slot, i.rel, i.b, i.pos, i.mb.in, i.mb.fm, i.mb.hid, i.tail_begin, i.tail_count});
  return o;
}
V fl(const std::vector<CvFInst>& v) {  // (slot, fp, b, pos, in, fm, hid)
  V o;
  for (auto& i : v) o.insert(o.end(), {i.slot, i.fp, i.b, i.pos, i.mb.in, i.mb.fm, i.mb.hid});
  return o;
}
V fl(const std::vector<CvAct>& v) {  // (slot, k_begin, k_count, f_begin, f_count, pad0, pad1)
  V o;
  for (auto& a : v) {
    o.insert(o.end(), {a.slot, a.k_begin, a.k_count, a.f_begin, a.f_count, a.pad0, a.pad1});
    CHECK(a.pad2 == 0, "act padding");
  }
  return o;
}
V fl(const std::vector<CvBits>& v) {
  V o;
  for (auto& b : v) o.insert(o.end(), {b.in, b.fm, b.hid});
  return o;
}

// ---------------------------------------------------------------------------------------
// ComplEx / DistMult, exact
// ---------------------------------------------------------------------------------------
// the five rows and two permutations of the multi-step cases: steps of 2, 2, 1 rows
const std::vector<int> ROWS5 = {K, 0, 1, 2, 1, K, K, 0, K, 2, 1, K, K, 3, 4};
const std::vector<int32_t> PERMS5 = {4, 1, 0, 3, 2, 3, 2, 1, 0, 4};

void cx_one_step() {
  Batch b;
  b.slot({K, 1, 2, K, 1, K, 3, 0, K, K, 2, 4, 3, 0, K, K, 1, 0}, 0);
  const kp_batch v = b.view();
  for (int bs : {6, 512}) {
    const std::string w = "cx one step (batch_size " + std::to_string(bs) + ")";
    CxStepPlan sp;
    expect_msg(w, cx_step_plan(K, NR, bs, 2, &v, sp), nullptr);
    // rows 0, 1, 5 are the query of relation 1 (one with the kelpie as tail), row 3 the query
    // of relation 2, rows 2 and 4 the tail of pair (3, 0)
    expect(w + " plans", fl(sp.plans), {6, 0, 2, 0, 1, 4, 3, 0});
    expect(w + " pqs", fl(sp.pqs), {1, 3, 1, 0, 2, /**/ 2, 1, 0, 2, 1});
    expect(w + " targets", fl(std::vector<int>(sp.targets.begin(), sp.targets.end())), {2, 0, 4});
    expect(w + " pairs", fl2(sp.pairs), {3, 0});
    expect(w + " pts", fl(sp.pts), {0, 2});
    CHECK(sp.T == 2 && sp.max_nq == 2 && sp.max_items == 3, w);
    expect(w + " acts", fl4(sp.acts), {0, 0, 0, 0, /**/ 0, 0, 0, 0});  // both steps: plan 0
    expect(w + " stepq", fl4(sp.stepq), {0, 1, 0, 0, 0, 2, 1, 0, /**/ 0, 1, 0, 0, 0, 2, 1, 0});
    expect(w + " stept", fl4(sp.stept), {0, 0, 2, 0, /**/ 0, 0, 2, 0});
    expect(w + " act_off", fl(sp.act_off), {0, 1, 2});
    expect(w + " q_off", fl(sp.q_off), {0, 2, 4});
    expect(w + " t_off", fl(sp.t_off), {0, 1, 2});
  }
}

void cx_several_steps() {
  Batch b;
  b.slot(ROWS5, 10);
  b.rng = PERMS5;
  const kp_batch v = b.view();
  const std::string w = "cx several steps";
  CxStepPlan sp;
  expect_msg(w, cx_step_plan(K, NR, 2, 2, &v, sp), nullptr);
  // epoch 0: rows (4, 1) (0, 3) (2); epoch 1: rows (3, 2) (1, 0) (4)
  expect(w + " plans", fl(sp.plans),
         {2, 0, 1, 0, 1, 1, 1, 0, /**/ 2, 1, 1, 1, 1, 1, 1, 0, /**/ 1, 2, 1, 2, 0, 1, 1, 0,
          2, 3, 1, 2, 1, 1, 2, 0, /**/ 2, 4, 1, 3, 1, 1, 1, 0, /**/ 1, 5, 1, 4, 0, 1, 0, 0});
  expect(w + " pqs", fl(sp.pqs),
         {3, 1, 0, 0, 1, /**/ 0, 1, 0, 1, 1, /**/ 0, 1, 1, 2, 0,
          0, 1, 1, 2, 0, /**/ 0, 1, 0, 2, 1, /**/ 3, 1, 0, 3, 1});
  expect(w + " targets", fl(std::vector<int>(sp.targets.begin(), sp.targets.end())), {4, 1, 1, 4});
  expect(w + " pairs", fl2(sp.pairs), {2, 1});  // one pair id for every plan
  expect(w + " pts", fl(sp.pts), {0, 1, 0, 1, 0, 1, 0, 1});
  CHECK(sp.T == 6 && sp.max_nq == 1 && sp.max_items == 2, w);
  expect(w + " acts", fl4(sp.acts),  // step t: plan t
         {0, 0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 4, 0, 0, 0, 5, 0, 0});
  expect(w + " stepq", fl4(sp.stepq),
         {0, 3, 0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 4, 0, 0, 3, 5, 0});
  expect(w + " stept", fl4(sp.stept), {0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0});
  expect(w + " act_off", fl(sp.act_off), {0, 1, 2, 3, 4, 5, 6});
  expect(w + " q_off", fl(sp.q_off), {0, 1, 2, 3, 4, 5, 6});
  expect(w + " t_off", fl(sp.t_off), {0, 1, 2, 2, 3, 4, 4});
}

void cx_mixed_slots() {
  Batch b;
  b.slot({K, 0, 1, 1, 2, K}, 0);  // one step per epoch: no draws
  b.slot(ROWS5, 10);              // three steps per epoch
  b.slot({}, 10);                 // no rows
  b.rng = PERMS5;
  const kp_batch v = b.view();
  const std::string w = "cx mixed slots";
  CxStepPlan sp;
  expect_msg(w, cx_step_plan(K, NR, 2, 2, &v, sp), nullptr);
  // slot 0: plan 0 for its 2 steps; slot 1: plans 1..6, the several-steps case shifted by
  // slot 0's one query, one target, one tail and one pair
  expect(w + " plans", fl(sp.plans),
         {2, 0, 1, 0, 1, 1, 1, 0,
          2, 1, 1, 1, 1, 1, 1, 0, /**/ 2, 2, 1, 2, 1, 1, 1, 0, /**/ 1, 3, 1, 3, 0, 1, 1, 0,
          2, 4, 1, 3, 1, 1, 2, 0, /**/ 2, 5, 1, 4, 1, 1, 1, 0, /**/ 1, 6, 1, 5, 0, 1, 0, 0});
  expect(w + " pqs", fl(sp.pqs),
         {0, 1, 0, 0, 1,
          3, 1, 0, 1, 1, /**/ 0, 1, 0, 2, 1, /**/ 0, 1, 1, 3, 0,
          0, 1, 1, 3, 0, /**/ 0, 1, 0, 3, 1, /**/ 3, 1, 0, 4, 1});
  expect(w + " targets", fl(std::vector<int>(sp.targets.begin(), sp.targets.end())), {1, 4, 1, 1, 4});
  expect(w + " pairs", fl2(sp.pairs), {1, 2, 2, 1});
  expect(w + " pts", fl(sp.pts), {0, 1, 1, 1, 1, 1, 1, 1, 1, 1});
  CHECK(sp.T == 6 && sp.max_nq == 2 && sp.max_items == 4, w);
  // steps 0 and 1 hold both slots, slot 1 after slot 0's one query and one tail; steps 2..5
  // only slot 1; slot 2 never
  expect(w + " acts", fl4(sp.acts),
         {0, 0, 0, 0, 1, 1, 1, 1, /**/ 0, 0, 0, 0, 1, 2, 1, 1, /**/ 1, 3, 0, 0, 1, 4, 0, 0, 1, 5, 0, 0, 1, 6, 0, 0});
  expect(w + " stepq", fl4(sp.stepq),
         {0, 0, 0, 0, 1, 3, 1, 0, /**/ 0, 0, 0, 0, 1, 0, 2, 0, /**/ 1, 0, 3, 0, 1, 0, 4, 0, 1, 0, 5, 0, 1, 3, 6, 0});
  expect(w + " stept", fl4(sp.stept),
         {0, 0, 1, 0, 1, 1, 1, 0, /**/ 0, 0, 1, 0, 1, 1, 1, 0, /**/ 1, 1, 1, 0, 1, 1, 1, 0});
  expect(w + " act_off", fl(sp.act_off), {0, 2, 4, 5, 6, 7, 8});
  expect(w + " q_off", fl(sp.q_off), {0, 2, 4, 5, 6, 7, 8});
  expect(w + " t_off", fl(sp.t_off), {0, 2, 4, 4, 5, 6, 6});
}

void cx_no_epochs() {
  Batch b;
  b.slot(ROWS5, 0);
  const kp_batch v = b.view();
  CxStepPlan sp;
  expect_msg("cx epochs = 0", cx_step_plan(K, NR, 2, 0, &v, sp), nullptr);
  CHECK(sp.T == 0 && sp.max_nq == 0 && sp.max_items == 0, "cx epochs = 0");
  CHECK(sp.plans.empty() && sp.pqs.empty() && sp.pts.empty() && sp.targets.empty() && sp.pairs.empty() &&
            sp.acts.empty() && sp.stepq.empty() && sp.stept.empty(),
        "cx epochs = 0");
  expect("cx epochs = 0 act_off", fl(sp.act_off), {0});
  expect("cx epochs = 0 q_off", fl(sp.q_off), {0});
  expect("cx epochs = 0 t_off", fl(sp.t_off), {0});
}

// ---------------------------------------------------------------------------------------
// ConvE, exact
// ---------------------------------------------------------------------------------------
// pairs in first-seen order: A = (K, 0) tails 1, 2, 1 (stored as 1, 2), C = (2, 3) frozen,
// B = (K, 1) tails 3, K.  batch_size 2: batch 0 = (A, C), batch 1 = (B)
const std::vector<int> ROWS_DEDUP = {K, 0, 1, 2, 3, K, K, 0, 2, K, 1, 3, K, 0, 1, K, 1, K};

void cv_tail_dedup(bool all_drops) {
  Batch b;
  b.slot(ROWS_DEDUP, all_drops ? 22 : 6);
  const kp_batch v = b.view();
  const std::string w = all_drops ? "cv tail dedup (in + fm + hidden, fr_step)" : "cv tail dedup (hidden only)";
  CvStepPlan sp;
  expect_msg(w, cv_step_plan(K, NR, DIM, 2, 2, all_drops, all_drops, true, all_drops, &v, sp), nullptr);
  CHECK(sp.T == 4 && sp.max_k == 1 && sp.max_sr == 1 && sp.max_fch == 1, w);  // nb = 2
  expect(w + " fpairs", fl2(sp.fpairs), {2, 3});
  expect(w + " tails", fl(std::vector<int>(sp.tails.begin(), sp.tails.end())), {1, 2, 3, K});
  // step t takes batch t % 2.  Words per step, runs in the order in (40 b bits), fm (32 b),
  // hidden (20 b), each rounded up to words: b = 2: 3, 2, 2; b = 1: 2, 1, 1
  if (!all_drops) {
    // hidden runs start at words 0, 2, 3, 5; a pair's bits at 32 * word + 20 * pos
    expect(w + " kinst", fl(sp.kinst),
           {0, 0, 2, 0, -1, -1, 0, 0, 2, /**/ 0, 1, 1, 0, -1, -1, 64, 2, 2,
            0, 0, 2, 0, -1, -1, 96, 0, 2, /**/ 0, 1, 1, 0, -1, -1, 160, 2, 2});
    expect(w + " finst", fl(sp.finst), {0, 0, 2, 1, -1, -1, 20, /**/ 0, 0, 2, 1, -1, -1, 116});  // fp: id in fpairs
    expect(w + " enc_src", fl2(sp.enc_src), {-1, 0, -1, 1, -1, 0, -1, 1});
    expect(w + " enc_bits", fl(sp.enc_bits), {-1, -1, 0, -1, -1, 64, -1, -1, 96, -1, -1, 160});
    expect(w + " enc_off", fl(sp.enc_off), {0, 1, 2, 3, 4});
    CHECK(sp.max_enc == 1, w);
  } else {
    // runs (in, fm, hidden) start at words (0, 3, 5) (7, 9, 10) (11, 14, 16) (18, 20, 21)
    expect(w + " kinst", fl(sp.kinst),
           {0, 0, 2, 0, 0, 96, 160, 0, 2, /**/ 0, 1, 1, 0, 224, 288, 320, 2, 2,
            0, 0, 2, 0, 352, 448, 512, 0, 2, /**/ 0, 1, 1, 0, 576, 640, 672, 2, 2});
    // fp: the row after the step's one kelpie pair
    expect(w + " finst", fl(sp.finst), {0, 1, 2, 1, 40, 128, 180, /**/ 0, 1, 2, 1, 392, 480, 532});
    expect(w + " enc_src", fl2(sp.enc_src), {-1, 0, 2, 3, /**/ -1, 1, /**/ -1, 0, 2, 3, /**/ -1, 1});
    expect(w + " enc_bits", fl(sp.enc_bits),
           {0, 96, 160, 40, 128, 180, /**/ 224, 288, 320, /**/ 352, 448, 512, 392, 480, 532, /**/ 576, 640, 672});
    expect(w + " enc_off", fl(sp.enc_off), {0, 2, 3, 5, 6});
    CHECK(sp.max_enc == 2, w);
  }
  expect(w + " acts", fl(sp.acts),
         {0, 0, 1, 0, 1, 0, 1, /**/ 0, 0, 1, 0, 0, 0, 0, /**/ 0, 0, 1, 0, 1, 0, 1, /**/ 0, 0, 1, 0, 0, 0, 0});
  expect(w + " fchunks", fl4(sp.fchunks), {0, 0, 1, 0, /**/ 0, 0, 1, 0});
  expect(w + " sr_src", fl2(sp.sr_src), {-1, 0, -1, 0, -1, 0, -1, 0});
  expect(w + " sr_rng", fl2(sp.sr_rng), {0, 1, 0, 1, 0, 1, 0, 1});
  expect(w + " psr", fl2(sp.psr), {0, 1, 0, 1, 0, 1, 0, 1});
  expect(w + " kin_off", fl(sp.kin_off), {0, 1, 2, 3, 4});
  expect(w + " fin_off", fl(sp.fin_off), {0, 1, 1, 2, 2});
  expect(w + " act_off", fl(sp.act_off), {0, 1, 2, 3, 4});
  expect(w + " sr_off", fl(sp.sr_off), {0, 1, 2, 3, 4});
  expect(w + " fch_off", fl(sp.fch_off), {0, 1, 1, 2, 2});
}

// one step of three slots: slot 0 = kelpie pairs (K, 0), (K, 1) and FCH + 1 frozen pairs
// (i % 5, i / 5); slot 1 = frozen (3, 2), which is slot 0's 13th, then kelpie (K, 2); slot 2 =
// frozen (1, 1) only, slot 0's 6th.  Hidden dropout only; the slots' draws start at words
// 0, 12 (19 pairs x 20 bits = 380 bits), 14.
void cv_shared_rows() {
  Batch b;
  std::vector<int> r0 = {K, 0, 1, K, 1, 2};
  for (int i = 0; i < FCH + 1; ++i) r0.insert(r0.end(), {i % 5, i / 5, K});
  b.slot(r0, 12);
  b.slot({3, 2, K, K, 2, 4}, 14);
  b.slot({1, 1, K}, 15);
  const kp_batch v = b.view();
  const std::string w = "cv shared rows";
  CvStepPlan sp;
  expect_msg(w, cv_step_plan(K, NR, DIM, 20, 1, false, false, true, false, &v, sp), nullptr);
  CHECK(sp.T == 1 && sp.max_k == 3 && sp.max_enc == 3 && sp.max_sr == 2 && sp.max_fch == 4, w);
  V fp;
  for (int i = 0; i < FCH + 1; ++i) fp.insert(fp.end(), {i % 5, i / 5});
  expect(w + " fpairs", fl2(sp.fpairs), fp);
  expect(w + " tails", fl(std::vector<int>(sp.tails.begin(), sp.tails.end())), {1, 2, 4});
  expect(w + " kinst", fl(sp.kinst),
         {0, 0, 19, 0, -1, -1, 0, 0, 1, /**/ 0, 1, 19, 1, -1, -1, 20, 1, 1,
          1, 2, 2, 1, -1, -1, 32 * 12 + 20, 2, 1});
  V fi;
  for (int i = 0; i < FCH + 1; ++i) fi.insert(fi.end(), {0, i, 19, 2 + i, -1, -1, 20 * (2 + i)});
  fi.insert(fi.end(), {1, 13, 2, 0, -1, -1, 32 * 12, /**/ 2, 6, 1, 0, -1, -1, 32 * 14});
  expect(w + " finst", fl(sp.finst), fi);
  expect(w + " acts", fl(sp.acts),
         {0, 0, 2, 0, FCH + 1, 0, 2, /**/ 1, 2, 1, FCH + 1, 1, 2, 1, /**/ 2, 3, 0, FCH + 2, 1, 3, 1});
  expect(w + " fchunks", fl4(sp.fchunks), {0, 0, FCH, 0, 0, FCH, 1, 0, /**/ 1, 0, 1, 0, /**/ 2, 0, 1, 0});
  // one shared row per slot with a kelpie pair; first = 1 only on the row's first pair
  expect(w + " sr_src", fl2(sp.sr_src), {-1, 0, -2, 0});
  expect(w + " sr_rng", fl2(sp.sr_rng), {0, 2, 2, 3});
  expect(w + " psr", fl2(sp.psr), {0, 1, 0, 0, 1, 1});
  expect(w + " enc_src", fl2(sp.enc_src), {-1, 0, -1, 1, -2, 2});
  expect(w + " enc_bits", fl(sp.enc_bits), {-1, -1, 0, -1, -1, 20, -1, -1, 32 * 12 + 20});
  expect(w + " kin_off", fl(sp.kin_off), {0, 3});
  expect(w + " fin_off", fl(sp.fin_off), {0, FCH + 3});
  expect(w + " act_off", fl(sp.act_off), {0, 3});
  expect(w + " enc_off", fl(sp.enc_off), {0, 3});
  expect(w + " sr_off", fl(sp.sr_off), {0, 2});
  expect(w + " fch_off", fl(sp.fch_off), {0, 4});
}

void cv_no_epochs() {
  Batch b;
  b.slot(ROWS_DEDUP, 0);
  const kp_batch v = b.view();
  CvStepPlan sp;
  expect_msg("cv epochs = 0", cv_step_plan(K, NR, DIM, 2, 0, false, false, true, false, &v, sp), nullptr);
  CHECK(sp.T == 0 && sp.kinst.empty() && sp.finst.empty() && sp.acts.empty() && sp.enc_src.empty() &&
            sp.sr_src.empty() && sp.psr.empty() && sp.fchunks.empty() && sp.tails.empty(),
        "cv epochs = 0");
  for (const std::vector<int>* o : {&sp.kin_off, &sp.fin_off, &sp.act_off, &sp.enc_off, &sp.sr_off, &sp.fch_off})
    expect("cv epochs = 0 offsets", fl(*o), {0});
}

// ---------------------------------------------------------------------------------------
// every error, once
// ---------------------------------------------------------------------------------------
const char* const E_ROW = "a training row does not involve the kelpie entity";
const char* const E_DRAWS = "missing randperm draws for a multi-step slot";
const char* const E_PERM = "randperm value out of range";
const char* const E_BITS = "missing dropout keep bits";

const char* cx_plan_of(const Batch& b, int bs, int epochs) {
  const kp_batch v = b.view();
  CxStepPlan sp;
  return cx_step_plan(K, NR, bs, epochs, &v, sp);
}
const char* cv_plan_of(const Batch& b, int bs, int epochs, bool drops = false) {
  const kp_batch v = b.view();
  CvStepPlan sp;
  return cv_step_plan(K, NR, DIM, bs, epochs, drops, drops, true, drops, &v, sp);
}

void errors() {
  Batch good;
  good.slot(ROWS5, 10);
  good.rng = PERMS5;
  expect_msg("cx good", cx_plan_of(good, 2, 2), nullptr);
  {
    Batch b = good;
    b.rows[3 * 1 + 2] = 3;  // (2, 1, 3)
    expect_msg("cx frozen row, multi-step", cx_plan_of(b, 2, 2), E_ROW);
    expect_msg("cx frozen row, one step", cx_plan_of(b, 8, 2), E_ROW);
  }
  {
    Batch b = good;
    b.rng_off[1] = 9;
    b.rng.pop_back();
    expect_msg("cx one draw short", cx_plan_of(b, 2, 2), E_DRAWS);
  }
  {
    Batch b = good;  // draws for one epoch of two
    b.rng_off[1] = 5;
    b.rng.resize(5);
    expect_msg("cx one epoch short", cx_plan_of(b, 2, 2), E_DRAWS);
  }
  for (int bad : {5, -1})
    for (int at : {0, 9}) {
      Batch b = good;
      b.rng[at] = bad;
      expect_msg("cx perm value " + std::to_string(bad) + " at " + std::to_string(at), cx_plan_of(b, 2, 2), E_PERM);
    }
  {
    Batch b = good;  // rng_off decreases across the slot
    b.rng_off = {10, 0};
    expect_msg("cx rng_off decreases", cx_plan_of(b, 2, 2), E_DRAWS);
  }
  Batch cv;
  cv.slot(ROWS_DEDUP, 6);
  expect_msg("cv good", cv_plan_of(cv, 2, 2), nullptr);
  {
    Batch b = cv;
    b.rows[3 * 1 + 2] = 4;  // (2, 3, 4)
    expect_msg("cv frozen row", cv_plan_of(b, 2, 2), E_ROW);
  }
  {
    Batch b = cv;
    b.rng_off[1] = 5;
    expect_msg("cv one word short", cv_plan_of(b, 2, 2), E_BITS);
  }
  {
    Batch b = cv;
    b.rng_off[1] = 21;
    expect_msg("cv one word short, three dropouts", cv_plan_of(b, 2, 2, true), E_BITS);
    b.rng_off[1] = 22;
    expect_msg("cv three dropouts", cv_plan_of(b, 2, 2, true), nullptr);
  }
  {
    Batch b = cv;
    b.rng_off = {6, 0};
    expect_msg("cv rng_off decreases", cv_plan_of(b, 2, 2), E_BITS);
  }
  {
    Batch b = cv;  // a slot without a step still may not run backwards
    b.rng_off = {6, 0};
    expect_msg("cv rng_off decreases, epochs = 0", cv_plan_of(b, 2, 0), E_BITS);
  }
}

// ---------------------------------------------------------------------------------------
// invariants on pseudo-random batches
// ---------------------------------------------------------------------------------------
struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(s >> 33);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

bool offsets_ok(const std::vector<int>& off, int T, size_t total) {
  if ((int)off.size() != T + 1 || off[0] != 0 || off[T] != (int)total) return false;
  for (int t = 0; t < T; ++t)
    if (off[t + 1] < off[t]) return false;
  return true;
}

void cx_invariants(const Batch& b, int ne, int nr, int bs, int epochs, const std::string& w) {
  const kp_batch v = b.view();
  CxStepPlan sp;
  const char* why = cx_step_plan(ne, nr, bs, epochs, &v, sp);
  if (why) return fail(w + ": " + why);
  const int T = sp.T, ns = v.n_slots;
  CHECK(offsets_ok(sp.act_off, T, sp.acts.size()) && offsets_ok(sp.q_off, T, sp.stepq.size()) &&
            offsets_ok(sp.t_off, T, sp.stept.size()),
        w);
  const int npl = (int)sp.plans.size(), npq = (int)sp.pqs.size(), npt = (int)sp.pts.size();
  long long rows_planned = 0, rows_expected = 0;
  int t_expected = 0;
  for (int s = 0; s < ns; ++s) {
    const int R = v.row_off[s + 1] - v.row_off[s];
    if (R == 0 || epochs == 0) continue;
    const int nst = (R + bs - 1) / bs;
    rows_expected += nst == 1 ? R : (long long)epochs * R;
    t_expected = std::max(t_expected, epochs * nst);
  }
  CHECK(T == t_expected, w);
  for (const CxPlan& P : sp.plans) {
    CHECK(P.q_begin >= 0 && P.q_count >= 0 && P.q_begin + P.q_count <= npq, w);
    CHECK(P.t_begin >= 0 && P.t_count >= 0 && P.t_begin + P.t_count <= npt, w);
    CHECK(P.b >= 1 && P.b <= bs, w);
    if (failures) return;
    int c = 0, ck = 0, tc = 0;
    for (int j = 0; j < P.q_count; ++j) {
      const CxQuery& Q = sp.pqs[P.q_begin + j];
      CHECK(Q.rel >= 0 && Q.rel < nr && Q.c >= 1 && Q.ck >= 0 && Q.c == Q.ck + Q.tg_count, w);
      CHECK(Q.tg_begin >= 0 && Q.tg_count >= 0 && Q.tg_begin + Q.tg_count <= (int)sp.targets.size(), w);
      c += Q.c;
      ck += Q.ck;
    }
    for (int j = 0; j < P.t_count; ++j) {
      const CxTail& t = sp.pts[P.t_begin + j];
      CHECK(t.pair >= 0 && t.pair < (int)sp.pairs.size() && t.c >= 1, w);
      tc += t.c;
    }
    // every row once: a (K, r, K) row is a query row that also counts on the right
    CHECK(c + tc == P.b && P.cnt_l == c && P.cnt_r == ck + tc, w);
    rows_planned += P.b;
  }
  CHECK(rows_planned == rows_expected, w);
  for (int32_t t : sp.targets) CHECK(t >= 0 && t < ne, w);
  for (const CxI2& p : sp.pairs) CHECK(p.x >= 0 && p.x < ne && p.y >= 0 && p.y < nr, w);
  int max_nq = 0, max_items = 0;
  for (int t = 0; t < T && !failures; ++t) {
    const int nq = sp.q_off[t + 1] - sp.q_off[t], nt = sp.t_off[t + 1] - sp.t_off[t];
    max_nq = std::max(max_nq, nq);
    max_items = std::max(max_items, nq + nt);
    int qo = 0, to = 0, last_slot = -1;
    for (int a = sp.act_off[t]; a < sp.act_off[t + 1]; ++a) {
      const CxI4 A = sp.acts[a];
      CHECK(A.x > last_slot && A.x < ns && A.y >= 0 && A.y < npl && A.z == qo && A.w == to, w);
      if (failures) return;
      last_slot = A.x;
      const CxPlan& P = sp.plans[A.y];
      CHECK(qo + P.q_count <= nq && to + P.t_count <= nt, w);
      if (failures) return;
      for (int j = 0; j < P.q_count; ++j) {
        const CxI4 q = sp.stepq[sp.q_off[t] + qo + j];
        CHECK(q.x == A.x && q.z == P.q_begin + j && q.y == sp.pqs[q.z].rel && q.w == 0, w);
      }
      for (int j = 0; j < P.t_count; ++j) {
        const CxI4 q = sp.stept[sp.t_off[t] + to + j];
        CHECK(q.x == A.x && q.y == sp.pts[P.t_begin + j].pair && q.z == sp.pts[P.t_begin + j].c && q.w == 0, w);
      }
      qo += P.q_count;
      to += P.t_count;
    }
    CHECK(qo == nq && to == nt, w);
  }
  CHECK(max_nq == sp.max_nq && max_items == sp.max_items, w);
}

void cv_invariants(const Batch& b, int ne, int nr, int bs, int epochs, bool has_in, bool has_fm, bool has_mask,
                   const std::string& w) {
  const kp_batch v = b.view();
  const bool fr_step = has_in || has_fm;
  CvStepPlan sp;
  const char* why = cv_step_plan(ne, nr, DIM, bs, epochs, has_in, has_fm, has_mask, fr_step, &v, sp);
  if (why) return fail(w + ": " + why);
  const int T = sp.T, ns = v.n_slots;
  CHECK(offsets_ok(sp.kin_off, T, sp.kinst.size()) && offsets_ok(sp.fin_off, T, sp.finst.size()) &&
            offsets_ok(sp.act_off, T, sp.acts.size()) && offsets_ok(sp.enc_off, T, sp.enc_src.size()) &&
            offsets_ok(sp.sr_off, T, sp.sr_src.size()) && offsets_ok(sp.fch_off, T, sp.fchunks.size()),
        w);
  CHECK(sp.enc_bits.size() == sp.enc_src.size() && sp.psr.size() == sp.kinst.size() &&
            sp.sr_rng.size() == sp.sr_src.size(),
        w);
  if (failures) return;
  // the slots' pairs in first-seen order, found the slow way: (h, r, kelpie-head)
  std::vector<std::vector<CvI2>> pairs(ns);
  int t_expected = 0;
  for (int s = 0; s < ns; ++s) {
    for (int j = v.row_off[s]; j < v.row_off[s + 1]; ++j) {
      bool seen = false;
      for (const CvI2& p : pairs[s]) seen |= p.x == v.rows[3 * j] && p.y == v.rows[3 * j + 1];
      if (!seen) pairs[s].push_back(CvI2{v.rows[3 * j], v.rows[3 * j + 1]});
    }
    t_expected = std::max(t_expected, epochs * (int)((pairs[s].size() + bs - 1) / bs));
  }
  CHECK(T == t_expected, w);
  for (int32_t t : sp.tails) CHECK(t >= 0 && t <= ne, w);
  for (const CvI2& p : sp.fpairs) CHECK(p.x >= 0 && p.x < ne && p.y >= 0 && p.y < nr, w);
  // a pair's keep bits lie inside its slot's draws, or are not drawn at all
  auto bits_ok = [&](const CvBits& m, int s) {
    const long long lo = 32 * v.rng_off[s], hi = 32 * v.rng_off[s + 1];
    return (has_in ? m.in >= lo && m.in + 2 * DIM <= hi : m.in == -1) &&
           (has_fm ? m.fm >= lo && m.fm + 32 <= hi : m.fm == -1) &&
           (has_mask ? m.hid >= lo && m.hid + DIM <= hi : m.hid == -1);
  };
  int max_k = 0, max_enc = 0, max_sr = 0, max_fch = 0;
  for (int t = 0; t < T && !failures; ++t) {
    const int nk = sp.kin_off[t + 1] - sp.kin_off[t], nf = sp.fin_off[t + 1] - sp.fin_off[t];
    const int ne_ = sp.enc_off[t + 1] - sp.enc_off[t], na = sp.act_off[t + 1] - sp.act_off[t];
    const int nsr = sp.sr_off[t + 1] - sp.sr_off[t], nch = sp.fch_off[t + 1] - sp.fch_off[t];
    max_k = std::max(max_k, nk);
    max_enc = std::max(max_enc, ne_);
    max_sr = std::max(max_sr, nsr);
    max_fch = std::max(max_fch, nch);
    CHECK(ne_ == nk + (fr_step ? nf : 0), w);
    const CvInst* KI = sp.kinst.data() + sp.kin_off[t];
    const CvFInst* FI = sp.finst.data() + sp.fin_off[t];
    const CvI2* ES = sp.enc_src.data() + sp.enc_off[t];
    int k = 0, f = 0, ch = 0, sr = 0, a = 0;
    for (int s = 0; s < ns; ++s) {
      const int np = (int)pairs[s].size(), nb = (np + bs - 1) / bs;
      if (nb == 0 || t >= epochs * nb) continue;  // the slot has ended
      CHECK(a < na, w);
      if (failures) return;
      const CvAct A = sp.acts[sp.act_off[t] + a];
      // each step's kelpie / frozen instances of a slot are that batch's pairs, in order
      const int p0 = (t % nb) * bs, p1 = std::min(np, p0 + bs);
      int want_k = 0, want_f = 0;
      for (int q = p0; q < p1; ++q) (pairs[s][q].x == ne ? want_k : want_f) += 1;
      CHECK(A.slot == s && A.k_begin == k && A.k_count == want_k && A.f_begin == f && A.f_count == want_f, w);
      CHECK(k + want_k <= nk && f + want_f <= nf, w);
      CHECK(A.pad0 == ch && A.pad1 == (want_f + FCH - 1) / FCH && ch + A.pad1 <= nch, w);
      if (failures) return;
      int ik = k, jf = f;
      for (int q = p0; q < p1; ++q) {
        if (pairs[s][q].x == ne) {
          const CvInst& I = KI[ik];
          CHECK(I.slot == s && I.rel == pairs[s][q].y && I.b == p1 - p0 && I.pos == q - p0 && bits_ok(I.mb, s), w);
          CHECK(I.tail_begin >= 0 && I.tail_count >= 1 && I.tail_begin + I.tail_count <= (int)sp.tails.size(), w);
          CHECK(ES[ik].x == -s - 1 && ES[ik].y == I.rel, w);
          const CvI2 ps = sp.psr[sp.kin_off[t] + ik];
          CHECK(ps.x == sr && ps.y == (ik == k ? 1 : 0), w);
          ++ik;
        } else {
          const CvFInst& F = FI[jf];
          CHECK(F.slot == s && F.b == p1 - p0 && F.pos == q - p0 && bits_ok(F.mb, s), w);
          if (fr_step) {  // its row of the step's encoder output holds its (h, r)
            CHECK(F.fp == nk + jf && ES[F.fp].x == pairs[s][q].x && ES[F.fp].y == pairs[s][q].y, w);
          } else {
            CHECK(F.fp >= 0 && F.fp < (int)sp.fpairs.size(), w);
            if (failures) return;
            CHECK(sp.fpairs[F.fp].x == pairs[s][q].x && sp.fpairs[F.fp].y == pairs[s][q].y, w);
          }
          ++jf;
        }
      }
      if (want_k > 0) {
        CHECK(sr < nsr, w);
        if (failures) return;
        const CvI2 src = sp.sr_src[sp.sr_off[t] + sr], rng = sp.sr_rng[sp.sr_off[t] + sr];
        CHECK(src.x == -s - 1 && src.y == 0 && rng.x == k && rng.y == k + want_k, w);
        ++sr;
      }
      int covered = 0;
      for (int q = 0; q < A.pad1; ++q) {
        const CvI4 c4 = sp.fchunks[sp.fch_off[t] + ch + q];
        CHECK(c4.x == a && c4.y == covered && c4.z >= 1 && c4.z <= FCH && c4.w == 0, w);
        covered += c4.z;
      }
      CHECK(covered == want_f, w);
      k += want_k;
      f += want_f;
      ch += A.pad1;
      ++a;
    }
    CHECK(a == na && k == nk && f == nf && ch == nch && sr == nsr, w);
    for (int i = 0; i < ne_; ++i) {
      const CvBits &m = sp.enc_bits[sp.enc_off[t] + i], &o = i < nk ? KI[i].mb : FI[i - nk].mb;
      CHECK(m.in == o.in && m.fm == o.fm && m.hid == o.hid, w);
    }
  }
  // a kelpie pair's tails are distinct
  for (const CvInst& I : sp.kinst)
    for (int i = 0; i < I.tail_count; ++i)
      for (int j = 0; j < i; ++j) CHECK(sp.tails[I.tail_begin + i] != sp.tails[I.tail_begin + j], w);
  CHECK(max_k == sp.max_k && max_enc == sp.max_enc && max_sr == sp.max_sr && max_fch == sp.max_fch, w);
}

void random_batches() {
  Rng g{20240611};
  int n = 0;
  for (; n < 400 && !failures; ++n) {
    const int ne = 3 + g.below(6), nr = 2 + g.below(5);
    const int bs = 1 + g.below(8), epochs = g.below(4), ns = g.below(9);
    Batch cx, cv;
    for (int s = 0; s < ns; ++s) {
      const int R = g.below(5) == 0 ? 0 : 1 + g.below(40);
      std::vector<int> rows;
      for (int j = 0; j < R; ++j) {
        if (g.below(2))
          rows.insert(rows.end(), {ne, g.below(nr), g.below(ne + 1)});
        else
          rows.insert(rows.end(), {g.below(ne), g.below(nr), ne});
      }
      // ComplEx: epochs x R permutation draws when the slot takes several steps per epoch
      if (R > bs)
        for (int e = 0; e < epochs; ++e) {
          std::vector<int32_t> perm(R);
          for (int j = 0; j < R; ++j) perm[j] = j;
          for (int j = R - 1; j > 0; --j) std::swap(perm[j], perm[g.below(j + 1)]);
          cx.rng.insert(cx.rng.end(), perm.begin(), perm.end());
        }
      cx.slot(rows, (int64_t)cx.rng.size());
      // ConvE: at most 3 epochs x 40 steps x (10 + 8 + 5) words
      cv.slot(rows, 4096 * (int64_t)(s + 1));
    }
    const std::string w = "random batch " + std::to_string(n);
    cx_invariants(cx, ne, nr, bs, epochs, w + " (cx)");
    const int drops = g.below(4);
    cv_invariants(cv, ne, nr, bs, epochs, drops & 1, drops & 2, drops != 3, w + " (cv)");
  }
  std::printf("random batches: %d\n", n);
}

}  // namespace

int main() {
  cx_one_step();
  cx_several_steps();
  cx_mixed_slots();
  cx_no_epochs();
  cv_tail_dedup(false);
  cv_tail_dedup(true);
  cv_shared_rows();
  cv_no_epochs();
  errors();
  random_batches();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
