// keyed_driver.cpp -- the keyed draws' pure-host header (kelpie_amd/csrc/kp_keyed.hpp) alone:
// `make keyed keyed_asan` builds this file plain and with -fsanitize=address,undefined, and
// tests/test_keyed_check.py runs both.  It checks the generator's three known answers, the
// word counts and each rule of the request check, and, given a file name, writes the sweep of
// draws that the test compares with the numpy restatement (tests/keyed_reference.py):
//   for R in {0, 1, 2, 63, 64, 65, 4096, 4097}, epochs in {0, 1, 3}:
//     for n in {1, 2, 517}: the TransE words of one slot (slot_key = SLOT_KEY + 1000003 R + epochs)
//     the ComplEx words of that slot at batch_size 64
//   for d in {3, 50, 260}: the uniform row (scale 1e-3f), then the normal row
//     (std = float(sqrt(2 / (d + 1)))), under init_key = INIT_KEY + d, as float32 bits
// every value as one int32.  Prints one line per case and exits 0 iff every case went as expected.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../kelpie_amd/csrc/kp_keyed.hpp"

namespace {

constexpr uint64_t INIT_KEY = 0x0123456789ABCDEFull, SLOT_KEY = 0xFEDCBA9876543210ull;
int failures = 0;

void report(const std::string& name, bool ok) {
  std::printf("%s: %s\n", name.c_str(), ok ? "ok" : "FAIL");
  if (!ok) ++failures;
}

void expect_msg(const std::string& name, const char* got, const char* want) {
  const bool ok = got && std::strcmp(got, want) == 0;
  std::printf("%s: %s%s\n", name.c_str(), got ? got : "(accepted)", ok ? "" : " FAIL");
  if (!ok) ++failures;
}

void known_answers() {
  struct Kat {
    uint32_t c[4], k[2], out[4];
  };
  const Kat kats[] = {
      {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
      {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
       {0xffffffffu, 0xffffffffu},
       {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
      {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u},
       {0xa4093822u, 0x299f31d0u},
       {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
  };
  int i = 0;
  for (const Kat& t : kats) {
    const KpPhilox4 r = kp_philox4x32_10(t.c[0], t.c[1], t.c[2], t.c[3], t.k[0], t.k[1]);
    report("known answer " + std::to_string(i++), std::memcmp(r.v, t.out, sizeof(t.out)) == 0);
  }
  // the counter layout: word w is lane w % 4 of the block (w / 4, epoch, stream, 0)
  const uint64_t key = 0x299f31d0a4093822ull;
  const KpPhilox4 blk = kp_philox4x32_10(5, 7, 2, 0, 0xa4093822u, 0x299f31d0u);
  report("counter layout", kp_keyed_word(key, 2, 7, 22) == blk.v[2] && kp_keyed_quad(key, 2, 7, 5).v[0] == blk.v[0]);
}

void counts_and_check() {
  kp_hp hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.epochs = 3;
  hp.batch_size = 64;
  const std::vector<int32_t> row_off = {0, 0, 64, 129, 140};
  std::vector<int64_t> w(4), off(5);
  const char* why = kp_keyed_words_host(KP_MODEL_TRANSE, &hp, 4, row_off.data(), w.data(), off.data());
  report("words TransE", !why && w == std::vector<int64_t>({0, 576, 585, 99}) && off[4] == 1260 && off[0] == 0);
  why = kp_keyed_words_host(KP_MODEL_COMPLEX, &hp, 4, row_off.data(), w.data(), off.data());
  report("words ComplEx", !why && w == std::vector<int64_t>({0, 0, 195, 0}) && off[4] == 195);
  why = kp_keyed_words_host(KP_MODEL_DISTMULT, &hp, 4, row_off.data(), w.data(), nullptr);
  report("words DistMult", !why && w == std::vector<int64_t>({0, 0, 195, 0}));
  expect_msg("words ConvE", kp_keyed_words_host(KP_MODEL_CONVE, &hp, 4, row_off.data(), w.data(), nullptr),
             "keyed draws serve TransE, ComplEx and DistMult");
  const std::vector<int32_t> bad = {0, 5, 3};
  expect_msg("words decreasing row_off", kp_keyed_words_host(KP_MODEL_TRANSE, &hp, 2, bad.data(), w.data(), nullptr),
             "bad row_off");
  const std::vector<int32_t> huge = {0, 2147483647};
  kp_hp big = hp;
  big.epochs = 2147483647;
  expect_msg("words beyond int64", kp_keyed_words_host(KP_MODEL_TRANSE, &big, 1, huge.data(), w.data(), nullptr),
             "word count beyond int64");
  big.batch_size = 1;
  why = kp_keyed_words_host(KP_MODEL_COMPLEX, &big, 1, huge.data(), w.data(), nullptr);
  report("words 2^62 fit", !why && w[0] == (int64_t)2147483647 * 2147483647);
  kp_hp neg = hp;
  neg.epochs = -1;
  expect_msg("words negative epochs", kp_keyed_words_host(KP_MODEL_TRANSE, &neg, 4, row_off.data(), w.data(), nullptr),
             "negative epochs");
  neg = hp;
  neg.batch_size = 0;
  expect_msg("words batch_size 0", kp_keyed_words_host(KP_MODEL_COMPLEX, &neg, 4, row_off.data(), w.data(), nullptr),
             "batch_size must be positive");

  // the request check: a good request, then each rule broken alone
  const std::vector<uint64_t> ik(4, INIT_KEY), sk(4, SLOT_KEY);
  kp_keyed k;
  std::memset(&k, 0, sizeof(k));
  k.n_slots = 4;
  k.init_key = ik.data();
  k.slot_key = sk.data();
  k.x0_scale = 1e-3f;
  k.neg_bound = 518;
  int code = 0;
  why = kp_check_keyed(KP_MODEL_TRANSE, &hp, 4, row_off.data(), &k, &code);
  std::printf("good: %s\n", why ? why : "ok");
  if (why) ++failures;
  expect_msg("null request", kp_check_keyed(KP_MODEL_TRANSE, &hp, 4, row_off.data(), nullptr, &code), "missing request");
  kp_keyed b = k;
  b.n_slots = 3;
  expect_msg("wrong n_slots", kp_check_keyed(KP_MODEL_TRANSE, &hp, 4, row_off.data(), &b, &code),
             "n_slots differs from the batch's");
  report("wrong n_slots code", code == KP_EINVAL);
  b = k;
  b.slot_key = nullptr;
  expect_msg("null slot_key", kp_check_keyed(KP_MODEL_COMPLEX, &hp, 4, row_off.data(), &b, &code), "missing keys");
  b = k;
  b.init_key = nullptr;
  expect_msg("null init_key", kp_check_keyed(KP_MODEL_COMPLEX, &hp, 4, row_off.data(), &b, &code), "missing keys");
  expect_msg("ConvE", kp_check_keyed(KP_MODEL_CONVE, &hp, 4, row_off.data(), &k, &code),
             "keyed draws serve TransE, ComplEx and DistMult");
  report("ConvE code", code == KP_ENOTSUP);
  b = k;
  b.neg_bound = 0;
  expect_msg("neg_bound 0", kp_check_keyed(KP_MODEL_TRANSE, &hp, 4, row_off.data(), &b, &code),
             "neg_bound must be in [1, 2^31]");
  b.neg_bound = ((int64_t)1 << 31) + 1;
  expect_msg("neg_bound 2^31 + 1", kp_check_keyed(KP_MODEL_TRANSE, &hp, 4, row_off.data(), &b, &code),
             "neg_bound must be in [1, 2^31]");
  b.neg_bound = 0;
  why = kp_check_keyed(KP_MODEL_COMPLEX, &hp, 4, row_off.data(), &b, &code);
  report("neg_bound unread by ComplEx", !why);
  b = k;
  b.n_slots = 1;
  big.batch_size = 64;
  expect_msg("int64", kp_check_keyed(KP_MODEL_TRANSE, &big, 1, huge.data(), &b, &code), "word count beyond int64");
  // the extremes of the integer streams
  report("neg extremes", kp_keyed_neg(0xFFFFFFFFu, (uint64_t)1 << 31) == 2147483647 && kp_keyed_neg(0u, 517) == 0 &&
                             kp_keyed_neg(0xFFFFFFFFu, 517) == 516 && kp_keyed_neg(0xFFFFFFFFu, 1) == 0);
  report("hot extremes", kp_keyed_hot(0x7FFFFFFFu) == 0 && kp_keyed_hot(0x80000000u) == 1);
  report("uniform below 1", kp_keyed_uniform(0xFFFFFFFFu, 1.f) < 1.f && kp_keyed_uniform(0u, 1.f) == 0.f);
  const float far = kp_keyed_normal(0u, 0u, 1.f);  // u1 = 2^-32: the largest radius, finite
  report("normal finite", far == far && far > 6.6f && far < 6.7f);
}

int sweep(const char* path) {
  std::vector<int32_t> all;
  kp_hp hp;
  std::memset(&hp, 0, sizeof(hp));
  hp.batch_size = 64;
  for (int32_t R : {0, 1, 2, 63, 64, 65, 4096, 4097})
    for (int E : {0, 1, 3}) {
      hp.epochs = E;
      const uint64_t key = SLOT_KEY + (uint64_t)1000003 * (uint64_t)R + (uint64_t)E;
      const int32_t row_off[2] = {0, R};
      int64_t w = 0;
      for (int64_t n : {1, 2, 517}) {
        if (kp_keyed_words_host(KP_MODEL_TRANSE, &hp, 1, row_off, &w, nullptr)) return 1;
        std::vector<int32_t> out((size_t)w);  // exactly the slot's words: the sanitizers see a write past them
        kp_keyed_slot_host(KP_MODEL_TRANSE, &hp, R, key, n, out.data());
        all.insert(all.end(), out.begin(), out.end());
      }
      if (kp_keyed_words_host(KP_MODEL_COMPLEX, &hp, 1, row_off, &w, nullptr)) return 1;
      std::vector<int32_t> out((size_t)w);
      kp_keyed_slot_host(KP_MODEL_COMPLEX, &hp, R, key, 0, out.data());
      all.insert(all.end(), out.begin(), out.end());
    }
  for (int d : {3, 50, 260})
    for (int model : {KP_MODEL_COMPLEX, KP_MODEL_TRANSE}) {
      std::vector<float> x((size_t)d);
      const float scale = model == KP_MODEL_TRANSE ? (float)std::sqrt(2.0 / (double)(d + 1)) : 1e-3f;
      kp_keyed_x0_host(model, d, INIT_KEY + (uint64_t)d, scale, x.data());
      const size_t at = all.size();
      all.resize(at + (size_t)d);
      std::memcpy(all.data() + at, x.data(), sizeof(float) * (size_t)d);
    }
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return 1;
  const bool ok = std::fwrite(all.data(), sizeof(int32_t), all.size(), f) == all.size();
  std::fclose(f);
  std::printf("sweep: %zu values\n", all.size());
  return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  known_answers();
  counts_and_check();
  if (argc > 1 && sweep(argv[1]) != 0) {
    std::printf("sweep: FAIL\n");
    ++failures;
  }
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
