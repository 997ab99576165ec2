// kp_margins_check.hpp -- the rank margins' request check and threshold rule
// (include/kelpie_hip.h, "Rank margins").  Pure host code, shared with the device: the
// threshold function is the one kp_rank.hip's margin kernels call, so a native driver
// (tests/native/margins_driver.cpp, `make margins margins_asan`) exercises the very statement
// the device compiles.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/kelpie_hip.h"

#if defined(__HIPCC__)
#define KP_MG_HD __host__ __device__
#else
#define KP_MG_HD
#endif

// the kinds of compared value (launch_rank_f64's score kinds, restated: kp_common.hpp)
enum { KP_MG_DOT = 0, KP_MG_SIGMOID = 1, KP_MG_DIST = 2, KP_MG_DIST1 = 3 };

// a set of outputs is wanted when any of its pointers is given
inline bool kp_margin_wanted(const kp_margin_out& o) {
  return o.rank_lo || o.rank_hi || o.ties || o.gap_better || o.gap_worse || o.id_better || o.id_worse;
}

// The check of a margins request, after the marks check and before any upload: nullptr, or the
// first rule broken.  `n_probes` / `n_marks`: what the call's probes / marks requests carry (0:
// none).  `rank64` false: the context ranks in fp32, *code becomes KP_ENOTSUP (else KP_EINVAL).
inline const char* kp_check_margins(const kp_margins* m, int n_probes, int n_marks, bool rank64, int* code) {
  *code = KP_EINVAL;
  if (!m) return "missing request";
  if (std::isnan(m->tol)) return "tol is NaN";
  if (m->tol < 0.0) return "negative tol";
  if (!(m->tol <= 1.0)) return "tol above 1";
  for (const kp_margin_out* o : {&m->slots, &m->probes, &m->marks})
    if ((o->rank_lo == nullptr) != (o->rank_hi == nullptr)) return "rank_lo and rank_hi go together";
  if (kp_margin_wanted(m->probes) && n_probes <= 0) return "probe outputs without probes";
  if (kp_margin_wanted(m->marks) && n_marks <= 0) return "mark outputs without marks";
  if (!rank64) {
    *code = KP_ENOTSUP;
    return "margins need the fp64 rank (the fp32 rank switch is set)";
  }
  return nullptr;
}

// a compared value in score units: the L2 family compares squared distances
KP_MG_HD inline double kp_margin_units(int mode, double c) { return mode == KP_MG_DIST ? sqrt(c) : c; }

// The thresholds of a row in compared units, from the target's compared value c_t and the
// call's tol: delta = tol * max(1, |v_t|) with v_t = c_t in score units.
//   maximizers: thr_lo = c_t + delta, thr_hi = c_t - delta
//   L1:         thr_lo = c_t - delta, thr_hi = c_t + delta
//   L2:         thr_lo = min(max(v_t - delta, 0)^2, c_t), thr_hi = max((v_t + delta)^2, c_t)
// tol == 0: both are c_t itself (no square of a square root).  Every operation is rounded on
// its own (no contraction), so the host and the device agree bit for bit.
KP_MG_HD inline void kp_margin_thresholds(int mode, double c_t, double tol, double* thr_lo, double* thr_hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (tol == 0.0) {
    *thr_lo = *thr_hi = c_t;
    return;
  }
  const double v_t = kp_margin_units(mode, c_t);
  const double a = fabs(v_t);
  const double delta = tol * (a > 1.0 ? a : 1.0);
  if (mode == KP_MG_DIST) {
    const double lo = v_t - delta > 0.0 ? v_t - delta : 0.0;
    const double hi = v_t + delta;
    // the square of a rounded root may miss c_t by an ulp when delta is below v_t's rounding:
    // the thresholds never cross c_t, so the band always holds the rank
    *thr_lo = lo * lo < c_t ? lo * lo : c_t;
    *thr_hi = hi * hi > c_t ? hi * hi : c_t;
  } else if (mode == KP_MG_DIST1) {
    *thr_lo = c_t - delta;
    *thr_hi = c_t + delta;
  } else {
    *thr_lo = c_t + delta;
    *thr_hi = c_t - delta;
  }
}
