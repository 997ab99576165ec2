// batch_check_driver.cpp -- kp_check_batch (kelpie_amd/csrc/kp_batch_check.hpp) under the host
// sanitizers: `make batch_asan` builds this file alone with -fsanitize=address,undefined, and
// tests/test_batch_check.py runs it.  One well-formed batch of 3 slots must pass; every
// malformed batch is that batch with exactly one rule broken and must yield a message.  The
// arrays are heap vectors of their exact length, so a check that reads past one is reported.
// Prints one line per case and exits 0 iff every case went as expected.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../kelpie_amd/csrc/kp_batch_check.hpp"

namespace {

constexpr int N_ENT = 50;  // the kelpie entity is id 50
constexpr int N_REL2 = 8;
constexpr int DIM = 4;

struct Batch {
  std::vector<float> x0;
  std::vector<int32_t> row_off, rows, pred, filt_off, filt;
  std::vector<int64_t> rng_off;
  std::vector<float> out_score;
  std::vector<int64_t> out_rank;
  kp_batch view() {
    kp_batch b;
    std::memset(&b, 0, sizeof(b));
    b.n_slots = (int32_t)(row_off.size() - 1);
    b.x0 = x0.data();
    b.row_off = row_off.data();
    b.rows = rows.data();
    b.rng_off = rng_off.data();
    b.rng = nullptr;
    b.pred = pred.data();
    b.filt_off = filt_off.data();
    b.filt = filt.data();
    b.out_x = nullptr;
    b.out_score = out_score.data();
    b.out_rank = out_rank.data();
    return b;
  }
};

// 3 slots; the boundary values that must be accepted are all here: n_ent as head, tail,
// ranked object and filter id, 0 and n_rel2 - 1 as relations, a slot without rows and a
// slot without filter ids
Batch good() {
  Batch b;
  b.x0.assign(3 * DIM, 0.5f);
  b.row_off = {0, 2, 2, 5};
  b.rows = {N_ENT, 0, 7,           //
            7,     4, N_ENT,       //
            N_ENT, N_REL2 - 1, 0,  //
            49,    3, N_ENT,       //
            N_ENT, 2, N_ENT};
  b.rng_off = {0, 0, 0, 0};
  b.pred = {N_ENT, 0, 7,           //
            N_ENT, N_REL2 - 1, 0,  //
            N_ENT, 3, N_ENT};
  b.filt_off = {0, 3, 3, 5};
  b.filt = {0, 7, N_ENT, 49, 12};
  b.out_score.assign(3, 0.f);
  b.out_rank.assign(3, 0);
  return b;
}

struct Case {
  const char* name;
  std::function<void(Batch&)> breakit;
};

}  // namespace

int main() {
  int failures = 0;
  {
    Batch b = good();
    kp_batch v = b.view();
    const char* why = kp_check_batch(N_ENT, N_REL2, DIM, &v);
    std::printf("good: %s\n", why ? why : "ok");
    if (why) ++failures;
  }
  {  // no slots at all is well formed too
    Batch b = good();
    b.row_off = {0};
    b.filt_off = {0};
    b.rows.clear();
    b.pred.clear();
    b.filt.clear();
    kp_batch v = b.view();
    const char* why = kp_check_batch(N_ENT, N_REL2, DIM, &v);
    std::printf("empty: %s\n", why ? why : "ok");
    if (why) ++failures;
  }
  const std::vector<Case> bad = {
      {"row_off[0] != 0", [](Batch& b) { b.row_off[0] = 1; }},
      {"row_off decreases", [](Batch& b) { b.row_off[1] = 3; }},  // {0, 3, 2, 5}
      {"filt_off decreases", [](Batch& b) { b.filt_off[1] = 4; }},  // {0, 4, 3, 5}
      {"head n_ent + 1", [](Batch& b) { b.rows[3 * 1 + 0] = N_ENT + 1; }},
      {"head -1", [](Batch& b) { b.rows[3 * 1 + 0] = -1; }},
      {"tail n_ent + 1", [](Batch& b) { b.rows[3 * 0 + 2] = N_ENT + 1; }},
      {"tail -1", [](Batch& b) { b.rows[3 * 0 + 2] = -1; }},
      {"relation n_rel2", [](Batch& b) { b.rows[3 * 2 + 1] = N_REL2; }},
      {"relation -1", [](Batch& b) { b.rows[3 * 2 + 1] = -1; }},
      {"last row's tail out of range", [](Batch& b) { b.rows[3 * 4 + 2] = N_ENT + 1; }},
      {"ranked subject a frozen entity", [](Batch& b) { b.pred[3 * 1 + 0] = 7; }},
      {"ranked subject n_ent + 1", [](Batch& b) { b.pred[3 * 2 + 0] = N_ENT + 1; }},
      {"ranked relation n_rel2", [](Batch& b) { b.pred[3 * 0 + 1] = N_REL2; }},
      {"ranked relation -1", [](Batch& b) { b.pred[3 * 0 + 1] = -1; }},
      {"ranked object n_ent + 1", [](Batch& b) { b.pred[3 * 2 + 2] = N_ENT + 1; }},
      {"ranked object -1", [](Batch& b) { b.pred[3 * 1 + 2] = -1; }},
      {"filter id n_ent + 1", [](Batch& b) { b.filt[2] = N_ENT + 1; }},
      {"filter id -1", [](Batch& b) { b.filt[0] = -1; }},
      {"last filter id out of range", [](Batch& b) { b.filt[4] = N_ENT + 1; }},
  };
  for (const Case& k : bad) {
    Batch b = good();
    k.breakit(b);
    kp_batch v = b.view();
    const char* why = kp_check_batch(N_ENT, N_REL2, DIM, &v);
    const bool rejected = why && why[0] != '\0';
    std::printf("%s: %s\n", k.name, rejected ? why : "ACCEPTED");
    if (!rejected) ++failures;
  }
  std::printf("%d cases, %d failures\n", (int)bad.size() + 2, failures);
  return failures ? 1 : 0;
}
