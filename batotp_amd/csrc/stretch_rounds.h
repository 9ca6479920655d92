// stretch_rounds.h -- what a round of batotp_hip_output_stretch_audit and batotp_hip_output_stretch_torques decides for one path,
// as plain C++ (include/batotp_hip_stretch.h and include/batotp_hip_tscale.h have the definition): from the records of the round's
// evaluation, is the path done, and if not, how many points does it get.  Nothing here touches the device: hipcc compiles this
// header into the library (stretch_api.inc, tscale_api.inc run the rounds) and a plain g++ -std=c++11 compiles it into
// tests/drivers/range_plan_main.cpp, which replays the records of the numpy references (tests/test_range_plan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "batotp_hip_duty.h"

namespace bk
{

// a path between the rounds; its point count is kept beside it (the counts of a batch are one array: the next stretch reads it)
struct StretchState
{
   int32_t rounds = 0, status = BATOTP_STRETCH_PASSES;
   bool capped = false;
};

// One path after a round.  a: its audit record; t: its scale record, or nullptr where the torque family takes no part (then the
// audit's TRQ peak is not read).  A peak of -1 -- not audited, or nothing to evaluate -- passes.  n_in: points of the path before
// the first round, n2: now.  d: its duty record (include/batotp_hip_duty.h), or nullptr where the RMS family takes no part.
// true: stretch it again, to the new n2.
inline bool stretchDecide(const batotp_path_audit &a, const batotp_path_tscale *t, double target, int32_t max_rounds, double max_factor, int64_t n_in,
                          int64_t &n2, StretchState &s, const batotp_path_duty *d = nullptr)
{
   const int velFam[2] = {BATOTP_AUDIT_JNT_VEL, BATOTP_AUDIT_CART_VEL}, accFam[2] = {BATOTP_AUDIT_JNT_ACC, BATOTP_AUDIT_CART_ACC};
   double need = 1.0;
   bool pass = true;
   for (int f : velFam)
      if (!(a.fam[f].peak <= target)) { pass = false; need = std::max(need, a.fam[f].peak / target); }
   for (int f : accFam)
      if (!(a.fam[f].peak <= target)) { pass = false; need = std::max(need, std::sqrt(a.fam[f].peak / target)); }
   const bool kinPass = pass, trqPass = !t || a.fam[BATOTP_AUDIT_TRQ].peak <= target;
   if (!trqPass)
   {
      pass = false;
      if (t->n_static == 0 && t->s < 1.0) need = std::max(need, 1.0 / t->s);
   }
   const bool rmsPass = !d || d->util <= target || d->util == -1.0;
   if (!rmsPass)
   {
      pass = false;
      if (d->n_hold == 0 && d->s < 1.0) need = std::max(need, 1.0 / d->s);
   }
   if (pass) { s.status = BATOTP_STRETCH_PASSES; return false; }
   if (kinPass && ((!trqPass && t->n_static > 0) || (!rmsPass && d->n_hold > 0))) { s.status = BATOTP_STRETCH_STATIC; return false; }
   if (s.capped) { s.status = BATOTP_STRETCH_CAPPED; return false; }
   if (s.rounds >= max_rounds) { s.status = BATOTP_STRETCH_ROUNDS; return false; }
   const int64_t m = n2 - 1;
   double intervals = std::max(std::ceil((double)m * need), (double)(m + 1));
   const double bound = std::min(std::floor((double)(n_in - 1) * max_factor), (double)(BATOTP_STRETCH_MAX_POINTS - 1));
   if (intervals > bound) { intervals = bound; s.capped = true; s.status = BATOTP_STRETCH_CAPPED; }
   const int64_t nNew = (int64_t)intervals + 1;
   if (nNew == n2) return false; // capped where it stands
   n2 = nNew;
   ++s.rounds;
   return true;
}

inline void stretchReport(int64_t n_in, int64_t n2, const StretchState &s, batotp_path_stretch &r)
{
   r.n_in = n_in; r.n_out = n2;
   r.factor = n_in < 2 ? 1.0 : (double)(n2 - 1) / (double)(n_in - 1);
   r.rounds = s.rounds; r.status = s.status;
}

} // namespace bk
