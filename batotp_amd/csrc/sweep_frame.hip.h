// sweep_frame.hip.h -- what surrounds the stage loop of a sweep kernel, once for all four of them: k_sweep (sweep_general.hip.h),
// k_sweep1 (sweep1.hip.h), k_sweep8 (sweep8.hip.h) and k_sweep8_lock (sweep8_fwd.hip.h).
//
// The kernels differ in their stage loops, on purpose.  Everything here runs once per path, never per stage, and transcribes the
// parts of BA::sweep that are easiest to get subtly wrong: the entry of a path (the forward sweep of a path without a reverse
// curve, the margin of curves kept in place, the step limit, the bootstrap of ba.cpp:1021-1041), the Butcher tableau, and the
// ending of a path (ba.cpp:1096-1184: error row, end snap, elapsed time, a curve of fewer than four points made four, result row).
// The order of the floating-point operations inside every function is the reference's; the kernels keep what lies between these
// steps (the store of the snapped point, the flush of the 8-lane kernels' group of four from LDS).
#pragma once
#include "kernels.hip.h"

namespace bk
{

// K4, the sweep.  Wavefront = 64 lanes = up to 64/G paths (a.ppw of them are used: with few paths in the batch it is faster to
// spread them over more wavefronts than to fill every lane).
struct SweepArgs
{
   DevProblem P;
   const DevProblem *dP;
   const PathInfo *pinfo;
   const double *sC;
   const double *coef;
   const double *km; // compact splines (FEAT == -1): [N][Cin][2] (value, second derivative) per path
   double2 *rev;  // [B][cap]
   double2 *fwd;  // [B][cap]
   batotp_path_result *res;
   int *sink;     // [B] consumer of the prefetch touches
   double *prof;  // diagnostic build (BK_PROFILE_SECTIONS): 4 doubles per path
   int64_t cap;
   int B;
   int dir;
   int ppw;       // paths per wavefront, 1 .. 64/G
   int hold;      // FLAT kernels: a stage is started once hold/8 of the wavefront's live paths wait for one
   int touch;     // software prefetch: bit 0 = spline rows ahead of the cursor, bit 1 = reverse curve ahead of its cursor (forward sweep)
   int ff;        // k_sweep1: certified fast-forward of the bisection (sweep1.hip.h), batotp_hip_set_fast_forward; k_sweep8: bit 0 forward, bit 1 reverse sweep
   int holdc;     // k_sweep8, reverse sweep: the certificate block serves the paths waiting for it once holdc/8 of the wavefront's live paths do
   // Ragged batches: launch slot k of the sweep processes path order[k] -- the paths sorted by knot count, longest
   // first.  The hardware hands workgroups to the SIMDs in launch order as slots free up, so this is longest-processing-time-first
   // scheduling for the kernels with a wavefront per path, and it puts paths of similar length into the same wavefront of the
   // kernels that carry several (a wavefront lasts as long as its longest path).  nullptr: paths in the order given (all equally
   // long, or batotp_hip_set_path_order(ctx, 0)).  Nothing in a path's own arithmetic or memory depends on its slot.
   const int *order;
};

// Butcher tableau of ba.cpp:58-63 (_B[k][j]; stage j+1 uses column j)
#define BK_B00 (1. / 5)
#define BK_B01 (3. / 40)
#define BK_B02 (44. / 45)
#define BK_B03 (19372. / 6561)
#define BK_B04 (9017. / 3168)
#define BK_B05 (35. / 384)
#define BK_B11 (9. / 40)
#define BK_B12 (-56. / 15)
#define BK_B13 (-25360. / 2187)
#define BK_B14 (-355. / 33)
#define BK_B15 (0.)
#define BK_B22 (32. / 9)
#define BK_B23 (64448. / 6561)
#define BK_B24 (46732. / 5247)
#define BK_B25 (500. / 1113)
#define BK_B33 (-212. / 729)
#define BK_B34 (49. / 176)
#define BK_B35 (125. / 192)
#define BK_B44 (-5103. / 18656)
#define BK_B45 (-2187. / 6784)
#define BK_B55 (11. / 84)

// The tableau as an LDS table for the kernels that index it with a stage number held in a register (k_sweep FLAT, k_sweep8):
// rk[st][k] = weight of stage value k in stage st (column st-1 of ba.cpp:58-63), 0 for k >= st.  Written by the first 42 threads of
// the workgroup; the caller's next __syncthreads (stage_limits) publishes it.
__device__ __forceinline__ void sweep_tableau_lds(double (&rk)[7][6])
{
   if (threadIdx.x < 42)
   {
      const double tab[42] = {0, 0, 0, 0, 0, 0,
                              BK_B00, 0, 0, 0, 0, 0,
                              BK_B01, BK_B11, 0, 0, 0, 0,
                              BK_B02, BK_B12, BK_B22, 0, 0, 0,
                              BK_B03, BK_B13, BK_B23, BK_B33, 0, 0,
                              BK_B04, BK_B14, BK_B24, BK_B34, BK_B44, 0,
                              BK_B05, BK_B15, BK_B25, BK_B35, BK_B45, BK_B55};
      (&rk[0][0])[threadIdx.x] = tab[threadIdx.x];
   }
}

// ---- the entry of a path -------------------------------------------------------------------------------------------------------

// The forward sweep of a path whose reverse sweep left no curve to follow (n_rev < 2: it ended with an error status): nothing to
// integrate.  The caller returns.
__device__ __forceinline__ void sweep_no_reverse_curve(batotp_path_result *__restrict__ r, bool writer)
{
   if (writer) { r->n_fwd = 0; r->steps_fwd = 0; r->t_total = 0; r->status_fwd = r->status_rev | BATOTP_ST_CAPACITY; r->n_bisect_fail_fwd = 0; }
}

// BATOTP_F_CURVES_IN_PLACE (forward sweep, a.fwd == a.rev): point i of the forward curve goes to slot i, reverse point m sits in
// slot cap - nRev + m.  The forward curve has at least as many points up to any s as the reverse curve, so slot i has been
// left behind by the reverse-curve cursor -- checked every step with 64 points of margin (the cursor's back-steps, the
// prefetch and the windows of k_sweep1 stay within 32; the register window of k_sweep8 / k_sweep8_lock, mvc_window.h, reads one
// point behind the cursor's segment and two ahead of it); a path that would run into live reverse points ends as if out of capacity.
// sweep_rev_start: the slot of reverse point 0 (beyond every slot when the curves have buffers of their own, or in the reverse sweep).
__device__ __forceinline__ int64_t sweep_rev_start(const SweepArgs &a, int nMvc, int dir)
{
   return (dir == 1 && a.fwd == a.rev) ? a.cap - (int64_t)nMvc : ((int64_t)1 << 62);
}
// the same for the kernels that count steps in an int (the launcher keeps cap below 2^30)
__device__ __forceinline__ int sweep_rev_start_int(const SweepArgs &a, int nMvc, int dir)
{
   const int64_t revStart = sweep_rev_start(a, nMvc, dir);
   return (revStart > 0x3fffffff) ? 0x3fffffff : (int)revStart;
}
// slot i cannot be written: the curve is full, or the slot is within the margin of the reverse-curve cursor (on segment segMVC)
template <typename I>
__device__ __forceinline__ bool sweep_curve_full(I i, I cap, I revStart, I segMVC)
{
   return i >= cap || i + 64 >= revStart + segMVC;
}

// steps after which a sweep ends with BATOTP_ST_MAX_INTEG_TIME (ba.cpp:1117-1122), and the same for an int counter
__device__ __forceinline__ int64_t sweep_max_steps(const DevProblem &P, const PathInfo &pi)
{
   return (int64_t)floor(P.max_integ_time / pi.integ_res) + 1;
}
__device__ __forceinline__ int sweep_max_steps_int(const DevProblem &P, const PathInfo &pi)
{
   const int64_t maxIntegSteps = sweep_max_steps(P, pi);
   return (maxIntegSteps > 0x3ffffff0) ? 0x3ffffff0 : (int)maxIntegSteps;
}

// Bootstrap, ba.cpp:1021-1041, for the kernels that start through Pt<>: both cursors on the path end the sweep starts from (s0v),
// then two passes of [bisection, velocity limit].  Kept as a loop so that the point evaluation is instantiated once here and once
// in the stage loop.  w0 comes in as the caller initialised it (a failed bisection keeps it).
template <int G, int FEAT, bool UNI>
__device__ __forceinline__ void pt_bootstrap(Pt<G, FEAT, UNI> &t, int j, int dir, int n, double h, double s0v, double &v0, double &w0)
{
   if (dir == 1) { t.segC = 0; t.tauC = 0; t.segMVC = 0; t.tauMVC = 0; }
   else { t.segC = n - 2; t.tauC = 1; t.segMVC = n - 2; t.tauMVC = 1; }
   t.sCur = s0v;
   t.sdotCur = 0;
#pragma unroll 1
   for (int pass = 0; pass < 2; ++pass)
   {
      accel_pt(t, j, w0);
      if (pass == 0) { v0 = .1 * h * w0; t.sdotMin = v0; }
      else v0 = t.sdotCur;
      sdot_lim(t, j, v0);
      if (pass == 0) { t.sdotMin = v0; t.sdotCur = v0; }
   }
}

// ---- the ending of a path ------------------------------------------------------------------------------------------------------

// A sweep that ended with an error status (capacity, time limit) after i steps: no curve.  The reverse sweep's row keeps the
// BATOTP_ST_SEG_ERROR the precompute may have left in status_rev.  The caller returns.
__device__ __forceinline__ void sweep_end_error(batotp_path_result *__restrict__ r, bool writer, int dir, int64_t i, unsigned status, int nfail)
{
   if (writer)
   {
      if (dir == 1) { r->n_fwd = 0; r->steps_fwd = i; r->t_total = 0; r->status_fwd = status; r->n_bisect_fail_fwd = nfail; }
      else { r->n_rev = 0; r->steps_rev = i; r->t_rev = 0; r->status_rev = (r->status_rev & BATOTP_ST_SEG_ERROR) | status; r->n_bisect_fail_rev = nfail; }
   }
}

// End snap onto sLast, ba.cpp:1132-1134: the last point (sCurPt, sdCurPt) moves onto the path end along the line from the point
// before it; forward sweep: its sdot is then the reverse curve's last one (lastRevSdot), ba.cpp:1140.
__device__ __forceinline__ void sweep_end_snap(int dir, double sLast, double sPrev, double sdPrev, double &sCurPt, double &sdCurPt, double lastRevSdot)
{
   const double sRat = (sLast - sPrev) / (sCurPt - sPrev);
   sdCurPt = sdPrev + sRat * (sdCurPt - sdPrev);
   sCurPt = sLast;
   if (dir == 1) sdCurPt = lastRevSdot;
}

// ba.cpp:1171-1184: a curve of nPts < 4 points is re-interpolated linearly in time to four.  pt: its points in integration order
// (the last one snapped; an entry beyond them holds any value); a reverse curve is turned round first, as the reference has done by then (ba.cpp:1145-1146).  The four
// points go where a curve of four ends up: out[0..3] forward, out[cap-4..cap-1] reverse.  One lane (the writer) calls this.
__device__ __forceinline__ void sweep_short_to_four(int dir, int nPts, double absh, const double2 (&pt)[3], double2 *out, int64_t cap)
{
   double ps[3], pd[3], tIn[3];
   // (all three entries, whatever nPts is: with constant indices pt stays in the caller's registers)
#pragma unroll
   for (int k = 0; k < 3; ++k)
   {
      ps[k] = pt[k].x; pd[k] = pt[k].y;
      tIn[k] = absh * (double)k; // ascending in time == integration order
   }
   if (dir != 1)
   {
      for (int k = 0; k < nPts / 2; ++k)
      {
         swap_d(ps[k], ps[nPts - 1 - k]);
         swap_d(pd[k], pd[nPts - 1 - k]);
      }
   }
   const double tResNew = tIn[nPts - 1] / 3.;
   int cur = 0;
   for (int k = 0; k < 4; ++k)
   {
      const double tn = tResNew * (double)k;
      while (!(tn < tIn[cur + 1] || cur == nPts - 2)) ++cur;
      const double tau = (tn - tIn[cur]) / (tIn[cur + 1] - tIn[cur]);
      out[dir == 1 ? k : cap - 4 + k] = make_double2(ps[cur] + (ps[cur + 1] - ps[cur]) * tau, pd[cur] + (pd[cur + 1] - pd[cur]) * tau);
   }
}

// The row of a sweep that reached the path end with nPts points, of which nOut are in the curve (4 for a short one, whose status
// the caller has marked BATOTP_ST_SHORT); the time is that of the integration, ba.cpp:1112.
__device__ __forceinline__ void sweep_end_result(batotp_path_result *__restrict__ r, bool writer, int dir, int64_t nOut, int64_t nPts, double absh,
                                                 unsigned status, int nfail)
{
   const double tElapsed = absh * (double)(nPts - 1);
   if (writer)
   {
      if (dir == 1)
      {
         r->n_fwd = nOut; r->steps_fwd = nPts - 1; r->t_total = tElapsed; r->status_fwd = status; r->n_bisect_fail_fwd = nfail;
      }
      else
      {
         r->n_rev = nOut; r->steps_rev = nPts - 1; r->t_rev = tElapsed;
         r->status_rev = (r->status_rev & BATOTP_ST_SEG_ERROR) | status; r->n_bisect_fail_rev = nfail;
      }
   }
}

} // namespace bk
