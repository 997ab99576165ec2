// kp_cv_plan.hpp -- host planning of the ConvE post-training steps: each slot's training
// rows grouped into (h, r) pairs with their tails (er_vocab, bce_optimizer.py:92-96:
// insertion order, NOT shuffled, minibatches of batch_size pairs), the keep-bit offsets of
// every dropout draw, and the per-step instance, encoder-row, shared-encoder-row and
// frozen-chunk lists with their offsets.  The step loop of kp_conve.hip adds these offsets
// to device pointers and its kernels index with the stored ids, so everything is decided
// here.  No HIP in here: tests/native/step_plan_driver.cpp builds this header alone
// (make step_plan_asan).
#pragma once

#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../include/kelpie_hip.h"

// bit offsets of one pair's dropout keep bits in a batch's draws (-1: that dropout is
// not drawn): input image (2 d bits, row-major 40 x d/20), feature-map channels (32),
// hidden units (d)
struct CvBits {
  long long in, fm, hid;
};
struct CvInst {  // one kelpie pair in one step
  int slot, rel, b, pos;
  CvBits mb;
  int tail_begin, tail_count;
};
struct CvFInst {  // one frozen-head pair in one step
  int slot, fp, b, pos;  // fp: its FC row (per batch), or its encoded row in the step's Q (fr_step)
  CvBits mb;
};
// one active slot of a step: its kelpie / frozen-head instances within the step's lists,
// and (pad0, pad1) its first kp_cv_fgrad chunk of the step and their count
struct CvAct {
  int slot, k_begin, k_count, f_begin, f_count, pad0, pad1, pad2;
};
// the device lists' element types, laid out as HIP's int2 / int4 (kp_conve.hip asserts it)
struct alignas(8) CvI2 {
  int x, y;
};
struct alignas(16) CvI4 {
  int x, y, z, w;
};
// frozen-head pairs per kp_cv_fgrad workgroup
constexpr int FCH = 16;

struct CvStepPlan {
  std::vector<CvI2> fpairs;     // distinct frozen (h, r) of the batch -> FC precompute
  std::vector<int32_t> tails;   // the kelpie pairs' distinct tails, first-seen order
  std::vector<CvInst> kinst;    // [kin_off[t], kin_off[t+1]) per step
  std::vector<CvFInst> finst;   // [fin_off[t], ..)
  std::vector<CvAct> acts;      // [act_off[t], ..)
  // the step's encoder rows (kelpie pairs, then with fr_step the frozen-head pairs) with
  // their keep-bit offsets: [enc_off[t], ..); a kelpie row X[s] is source (-s - 1, rel)
  std::vector<CvI2> enc_src;
  std::vector<CvBits> enc_bits;
  // the shared-encoder path's kelpie rows per step, [sr_off[t], ..): one per slot with a
  // kelpie pair in the step, its source and its pairs' range in the step's list; and per
  // kelpie pair (parallel to kinst) its kelpie row and whether it is that row's first pair
  std::vector<CvI2> sr_src, sr_rng, psr;
  // the frozen-head pairs' chunks per step (kp_cv_fgrad), [fch_off[t], ..): (the slot's act
  // within the step, first pair, pair count <= FCH, 0)
  std::vector<CvI4> fchunks;
  std::vector<int> kin_off, fin_off, act_off, enc_off, sr_off, fch_off;  // [T + 1]
  int T = 0;  // steps of the longest slot
  int max_k = 0, max_enc = 0, max_sr = 0, max_fch = 0;  // most rows of one step
};

struct CvPair {
  int h, r;
  std::vector<int> tails;
  int tail_begin = -1, tail_count = 0;  // kelpie pair: its distinct tails in `tails`; frozen: its FC row
};
// a slot's pairs in first-seen order, cut into nb minibatches of batch_size pairs
struct CvSlotPlan {
  std::vector<CvPair> pairs;
  int nb = 0;
};
// word offsets of one step's keep-bit runs (-1: not drawn)
struct CvStepBits {
  long long in, fm, hid;
};

struct CvPlanBuilder {
  CvStepPlan& sp;
  const int K, n_rel2, dim, batch_size, epochs;
  const bool has_in, has_fm, has_mask, fr_step;
  const kp_batch* bt;
  std::vector<CvSlotPlan> slots;
  std::unordered_map<long long, int> fp_id;    // h * n_rel2 + r -> fpairs
  std::vector<std::vector<CvStepBits>> moff;   // [slot][step]
  std::vector<CvI2> fr_hr;                      // the current step's frozen-head (h, r), with fr_step

  // er_vocab of slot s; registers its frozen pairs
  const char* group_pairs(int s) {
    std::unordered_map<long long, int> idx;
    auto& P = slots[s].pairs;
    for (int j = bt->row_off[s]; j < bt->row_off[s + 1]; ++j) {
      const int h = bt->rows[3 * j], r = bt->rows[3 * j + 1], t = bt->rows[3 * j + 2];
      const long long key = (long long)h * n_rel2 + r;
      auto it = idx.find(key);
      if (it == idx.end()) {
        idx.emplace(key, (int)P.size());
        P.push_back(CvPair{h, r, {t}});
      } else {
        P[it->second].tails.push_back(t);
      }
    }
    slots[s].nb = P.empty() ? 0 : (int)((P.size() + batch_size - 1) / batch_size);
    sp.T = std::max(sp.T, epochs * slots[s].nb);
    for (auto& pr : P)
      if (pr.h != K) {
        for (int tt : pr.tails)
          if (tt != K) return "a training row does not involve the kelpie entity";
        const long long key = (long long)pr.h * n_rel2 + pr.r;
        if (!fp_id.count(key)) {
          fp_id.emplace(key, (int)sp.fpairs.size());
          sp.fpairs.push_back(CvI2{pr.h, pr.r});
        }
      }
    return nullptr;
  }

  // keep-bit offsets of slot s: steps in order; per step one word-aligned run per drawn
  // dropout, in the forward's order (input b x 2d, feature map b x 32, hidden b x d)
  const char* bit_offsets(int s) {
    const int nb = slots[s].nb;
    const int P = (int)slots[s].pairs.size();
    long long off = bt->rng_off[s];
    for (int t = 0; t < epochs * nb; ++t) {
      const int j = t % nb;
      const long long b = std::min(batch_size, P - j * batch_size);
      CvStepBits sb{-1, -1, -1};
      if (has_in) { sb.in = off; off += (b * 2 * dim + 31) / 32; }
      if (has_fm) { sb.fm = off; off += (b * 32 + 31) / 32; }
      if (has_mask) { sb.hid = off; off += (b * dim + 31) / 32; }
      moff[s].push_back(sb);
    }
    return off <= bt->rng_off[s + 1] ? nullptr : "missing dropout keep bits";
  }

  CvBits pair_bits(const CvStepBits& sb, int pos) const {
    return CvBits{sb.in < 0 ? -1 : 32 * sb.in + (long long)pos * 2 * dim,
                  sb.fm < 0 ? -1 : 32 * sb.fm + (long long)pos * 32,
                  sb.hid < 0 ? -1 : 32 * sb.hid + (long long)pos * dim};
  }

  // slot s's minibatch of step t appended to the step's lists; local_k counts the step's
  // kelpie pairs so far
  void add_slot_step(int t, int s, int& local_k) {
    auto& P = slots[s].pairs;
    const int j = t % slots[s].nb;
    const int p0 = j * batch_size, p1 = std::min((int)P.size(), p0 + batch_size);
    const int b = p1 - p0;
    CvAct A{};
    A.slot = s;
    A.k_begin = local_k;
    A.f_begin = (int)sp.finst.size() - sp.fin_off[t];
    int my_sr = -1;
    for (int q = p0; q < p1; ++q) {
      auto& pr = P[q];
      if (pr.h == K) {
        const bool first = my_sr < 0;
        if (first) {
          my_sr = (int)sp.sr_src.size() - sp.sr_off[t];
          sp.sr_src.push_back(CvI2{-s - 1, 0});
        }
        sp.psr.push_back(CvI2{my_sr, first ? 1 : 0});
        CvInst I{};
        I.slot = s;
        I.rel = pr.r;
        I.b = b;
        I.pos = q - p0;
        I.mb = pair_bits(moff[s][t], I.pos);
        if (pr.tail_begin < 0) {  // the pair's distinct tails, stored once for every step
          pr.tail_begin = (int)sp.tails.size();
          for (int tt : pr.tails)
            if (std::find(sp.tails.begin() + pr.tail_begin, sp.tails.end(), tt) == sp.tails.end())
              sp.tails.push_back(tt);
          pr.tail_count = (int)sp.tails.size() - pr.tail_begin;
        }
        I.tail_begin = pr.tail_begin;
        I.tail_count = pr.tail_count;
        sp.kinst.push_back(I);
        ++local_k;
      } else {
        CvFInst F{};
        F.slot = s;
        if (!fr_step && pr.tail_begin < 0) pr.tail_begin = fp_id.at((long long)pr.h * n_rel2 + pr.r);
        F.fp = fr_step ? (int)sp.finst.size() - sp.fin_off[t] : pr.tail_begin;  // (frozen pair: its FC row)
        F.b = b;
        F.pos = q - p0;
        F.mb = pair_bits(moff[s][t], F.pos);
        sp.finst.push_back(F);
        if (fr_step) fr_hr.push_back(CvI2{pr.h, pr.r});
      }
    }
    A.k_count = local_k - A.k_begin;
    A.f_count = (int)sp.finst.size() - sp.fin_off[t] - A.f_begin;
    A.pad0 = (int)sp.fchunks.size() - sp.fch_off[t];
    A.pad1 = (A.f_count + FCH - 1) / FCH;
    for (int f = 0; f < A.f_count; f += FCH)
      sp.fchunks.push_back(CvI4{(int)sp.acts.size() - sp.act_off[t], f, std::min(FCH, A.f_count - f), 0});
    sp.acts.push_back(A);
    if (my_sr >= 0) sp.sr_rng.push_back(CvI2{A.k_begin, A.k_begin + A.k_count});
  }

  // step t's lists: every slot still running, then the step's encoder rows
  void add_step(int t) {
    sp.kin_off[t] = (int)sp.kinst.size();
    sp.fin_off[t] = (int)sp.finst.size();
    sp.act_off[t] = (int)sp.acts.size();
    sp.enc_off[t] = (int)sp.enc_src.size();
    sp.sr_off[t] = (int)sp.sr_src.size();
    sp.fch_off[t] = (int)sp.fchunks.size();
    fr_hr.clear();
    int local_k = 0;
    for (int s = 0; s < (int)slots.size(); ++s)
      if (slots[s].nb != 0 && t < epochs * slots[s].nb) add_slot_step(t, s, local_k);
    sp.max_sr = std::max(sp.max_sr, (int)sp.sr_src.size() - sp.sr_off[t]);
    sp.max_fch = std::max(sp.max_fch, (int)sp.fchunks.size() - sp.fch_off[t]);
    for (int i = sp.kin_off[t]; i < (int)sp.kinst.size(); ++i) {
      sp.enc_src.push_back(CvI2{-sp.kinst[i].slot - 1, sp.kinst[i].rel});
      sp.enc_bits.push_back(sp.kinst[i].mb);
    }
    if (fr_step)
      for (int i = sp.fin_off[t]; i < (int)sp.finst.size(); ++i) {
        sp.finst[i].fp += local_k;  // its row in the step's encoder output, after the kelpie pairs
        sp.enc_src.push_back(fr_hr[i - sp.fin_off[t]]);
        sp.enc_bits.push_back(sp.finst[i].mb);
      }
    sp.max_k = std::max(sp.max_k, local_k);
    sp.max_enc = std::max(sp.max_enc, (int)sp.enc_src.size() - sp.enc_off[t]);
  }
};

// Fills `sp` for a batch that kp_check_batch accepted (every row id in range).  nullptr
// when the plan is good, else the rule the batch breaks.
inline const char* cv_step_plan(int n_ent, int n_rel2, int dim, int batch_size, int epochs, bool has_in, bool has_fm,
                                bool has_mask, bool fr_step, const kp_batch* bt, CvStepPlan& sp) {
  sp = CvStepPlan{};
  const int ns = bt->n_slots;
  CvPlanBuilder pb{sp, n_ent, n_rel2, dim, batch_size, epochs, has_in, has_fm, has_mask, fr_step, bt};
  pb.slots.resize(ns);
  pb.moff.resize(ns);
  for (int s = 0; s < ns; ++s)
    if (const char* why = pb.group_pairs(s)) return why;
  for (int s = 0; s < ns; ++s)
    if (const char* why = pb.bit_offsets(s)) return why;
  const int T = sp.T;
  for (std::vector<int>* off : {&sp.kin_off, &sp.fin_off, &sp.act_off, &sp.enc_off, &sp.sr_off, &sp.fch_off})
    off->assign(T + 1, 0);
  for (int t = 0; t < T; ++t) pb.add_step(t);
  sp.kin_off[T] = (int)sp.kinst.size();
  sp.fin_off[T] = (int)sp.finst.size();
  sp.act_off[T] = (int)sp.acts.size();
  sp.enc_off[T] = (int)sp.enc_src.size();
  sp.sr_off[T] = (int)sp.sr_src.size();
  sp.fch_off[T] = (int)sp.fchunks.size();
  return nullptr;
}
