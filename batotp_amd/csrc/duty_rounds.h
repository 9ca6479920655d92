// duty_rounds.h -- the host rule of include/batotp_hip_duty.h as plain C++: the record of a path from the sums the kernels wrote
// for it.  Nothing here touches the device: hipcc compiles this header into the library (duty_api.inc) and a plain g++ -std=c++11
// compiles it into tests/drivers/duty_plan_main.cpp, which replays the sums of the numpy reference (tests/test_duty_cpu.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "batotp_hip_duty.h"

namespace bk
{

// what a call forms once of its ratings: rr_j = 1.0 / rated_j and lim_j = target * rated_j
struct DutyRating
{
   int n_links;
   double rr[BATOTP_MAX_LINKS], lim[BATOTP_MAX_LINKS];
};

inline void dutyRating(int n_links, const double *rated, double target, DutyRating &R)
{
   R.n_links = n_links;
   for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
   {
      R.rr[j] = j < n_links ? 1.0 / rated[j] : 0.0;
      R.lim[j] = j < n_links ? target * rated[j] : 0.0;
   }
}

// h: the time step of the path
inline void dutyRecord(const batotp_path_duty_sums &S, const DutyRating &R, double h, batotp_path_duty &d)
{
   const double n = (double)S.n_pts;
   d.util = -1.0; d.row = -1; d.n_hold = 0;
   d.s = std::numeric_limits<double>::infinity(); d.s_row = -1; d.reserved = 0;
   for (int j = 0; j < BATOTP_MAX_LINKS; ++j) d.rms[j] = 0.0;
   for (int j = 0; j < R.n_links && S.n_pts > 0; ++j)
   {
      const double *m = S.S[j];
      d.rms[j] = std::sqrt(m[6] / n);
      const double u = d.rms[j] * R.rr[j];
      if (std::isfinite(u) && u > d.util) { d.util = u; d.row = j; }
      const double L = (R.lim[j] * R.lim[j]) * n;
      const double c4 = m[0], c3 = 2.0 * m[1], c2 = m[2] + 2.0 * m[3], c1 = 2.0 * m[4], c0 = m[5];
      if (!(c0 < L)) { ++d.n_hold; continue; }
      auto P = [=](double x) { return (((c4 * x + c3) * x + c2) * x + c1) * x + c0; };
      if (P(1.0) <= L) continue;
      double lo = 0.0, hi = 1.0;
      for (int pass = 0; pass < 64; ++pass)
      {
         const double mid = 0.5 * (lo + hi);
         if (P(mid) <= L) lo = mid; else hi = mid;
      }
      if (lo < d.s) { d.s = lo; d.s_row = j; }
   }
   d.energy = h * S.W;
   d.peak_power = S.peak_power; d.power_at = S.power_at; d.n_pts = S.n_pts;
}

} // namespace bk
