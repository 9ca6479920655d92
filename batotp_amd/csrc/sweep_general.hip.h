// sweep_general.hip.h -- k_sweep, the general sweep kernel: every constraint family and every lane layout of Pt<> (kernels.hip.h),
// as nested stage / bisection loops or as one flat loop (FLAT).  The kernels written for one regime each are k_sweep1
// (sweep1.hip.h: a wavefront per path), k_sweep8 (sweep8.hip.h: batches of velocity / acceleration-only problems) and
// k_sweep8_lock (sweep8_fwd.hip.h: its forward sweep in lockstep); what surrounds the stage loop is shared with them
// (sweep_frame.hip.h).
#pragma once
#include "sweep_frame.hip.h"

namespace bk
{

// Software prefetch: the walk over the spline rows (and over the reverse curve) is monotone, so
// every stage of the reverse sweep each lane of the group touches one 128-byte line of the next
// kilobyte ahead of (below) the cursor.  The loaded word is consumed one stage later (t.sink), which keeps the load alive without
// ever waiting on it, and by then the line sits in the vector L1 / L2 instead of HBM.
template <int G, int FEAT, bool UNI>
__device__ __forceinline__ int touch_ahead(const Pt<G, FEAT, UNI> &t, int j)
{
   const int linesAhead = 1 + (j & 7);
   const int rowDoubles = t.C * 4;
   int v = 0;
   if (FEAT < 0)
   {
      // compact splines: rows of Cin pairs; same scheme as below on the pair stream
      const int rowD = t.nIn * 2;
      int off = t.segC * rowD + t.dir * linesAhead * 16;
      const int hi = (t.n - 1) * rowD;
      off = off < 0 ? 0 : (off > hi ? hi : off);
      v = reinterpret_cast<const int *>(t.km)[2 * (unsigned)off];
   }
   else
   {
      // spline rows: byte offset of the current row, then +/- (1..8) lines
      const int lastRow = t.n - 1;
      int off = t.segC * rowDoubles + t.dir * linesAhead * 16; // in doubles (16 doubles = 128 B)
      const int hi = lastRow * rowDoubles;
      off = off < 0 ? 0 : (off > hi ? hi : off);
      v = reinterpret_cast<const int *>(t.coef)[2 * (unsigned)off];
   }
   return v;
}

// the same for the reverse curve the forward sweep follows: (s, sdot) pairs, 8 points per 128-byte line, ascending walk
template <int G, int FEAT, bool UNI>
__device__ __forceinline__ int touch_curve_ahead(const Pt<G, FEAT, UNI> &t, int j)
{
   int off = t.segMVC * 2 + (1 + (j & 7)) * 16; // in doubles
   const int hi = (t.nMvc - 1) * 2;
   off = off > hi ? hi : off;
   return reinterpret_cast<const int *>(t.mvc)[2 * (unsigned)off];
}

// A workgroup is 4 wavefronts (one per SIMD of a CU): with one-wavefront workgroups the dispatcher was
// observed to stack several of them on the SIMDs of one CU while other CUs stayed empty.
constexpr int K4_BLOCK = 256;
constexpr int BK_SWEEP_WPE = 2; // waves per SIMD the register allocation of the narrow (FEAT <= 1) sweep kernels is tuned for
// FLAT: the stage loop and the bisection loop are one loop in which every path of the wavefront is either
// waiting for its next stage or inside a constraint check (see the comment at the loop).
template <int G, int FEAT, bool UNI, bool FLAT = false>
__global__ void __launch_bounds__(K4_BLOCK, (G > 1 && G < 8) ? 1 : (FEAT <= 1 && G > 1) ? BK_SWEEP_WPE : 2) k_sweep(SweepArgs a)
{
   __shared__ double lim[6][8];
   __shared__ double rk[7][6]; // FLAT: the tableau by stage number (sweep_tableau_lds)
   if (FLAT) sweep_tableau_lds(rk);
   stage_limits(a.dP, lim);

   const int lane = threadIdx.x & 63;
   const int wave = blockIdx.x * (K4_BLOCK / 64) + (threadIdx.x >> 6);
   constexpr bool SPLIT = Pt<G, FEAT, UNI>::SPLIT;
   constexpr bool SPEC = Pt<G, FEAT, UNI>::SPEC;
   const int j = (SPLIT || SPEC) ? (lane & 7) : lane % G;   // joint owned by this lane
   const int slot = lane / G;
   const int pslot = wave * a.ppw + slot;
   if (slot >= a.ppw || pslot >= a.B) return; // whole groups leave together; DPP never crosses groups
   const int p = a.order ? a.order[pslot] : pslot;
   const bool writer = (lane % G == 0);
   const int dir = a.dir;
   const PathInfo pi = a.pinfo[p];
   const int n = (int)pi.n;
   const int64_t cap = a.cap;

   Pt<G, FEAT, UNI> t;
   pt_init(t, a.P, pi, a.sC, a.coef, a.km, lim, j, dir);
   t.side = SPLIT ? ((lane >> 3) & 1) : 0;
   t.cslot = SPEC ? ((lane >> 3) & 3) : 0;
   t.pbase = lane & ~(G - 1);

   double2 *out = (dir == 1 ? a.fwd : a.rev) + (int64_t)p * cap; // may alias t.mvc (curves in place): no __restrict__
   batotp_path_result *__restrict__ r = a.res + p;
   if (dir == 1)
   {
      const int64_t nRev = r->n_rev;
      if (nRev < 2)
      {
         sweep_no_reverse_curve(r, writer);
         return;
      }
      t.mvc = reinterpret_cast<const double *>(a.rev + (int64_t)p * cap + (cap - nRev));
      t.nMvc = (int)nRev;
   }
   const int64_t revStart = sweep_rev_start(a, t.nMvc, dir);

   const double absh = pi.integ_res;
   const double h = dir * absh;
   const int64_t maxIntegSteps = sweep_max_steps(a.P, pi);
   const double sEnd = UNI ? pi.sres_c * (double)(n - 1) : t.sC[n - 1];
   const double sLast = (dir == 1) ? sEnd : 0;
   double s0v = (dir == 1) ? 0 : sEnd, s6v = 0;     // sArr[0], sArr[6] (the other stage positions are not reused)
   double v0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0, v6 = 0;   // sdotArr
   double w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, w6 = 0; // sddotArr
   pt_bootstrap(t, j, dir, n, h, s0v, v0, w0);

   // point 0
   double sPrev = s0v, sdPrev = v0; // last two published points, for the end snap
   double sCurPt = s0v, sdCurPt = v0;
   if (writer) out[dir == 1 ? 0 : cap - 1] = make_double2(s0v, v0);

   // ba.cpp:1050-1051: dsMin uses sArr.back() == 0, hence every dsMinV[j]/absh is +0
   const double floorV = 0.0 / absh;

#ifdef BK_PROFILE_SECTIONS
   const unsigned long long tstart = __builtin_readcyclecounter();
#endif
   int64_t nPts = 0, i = 1;
   unsigned endStatus = 0;
   int pf = 0, pf2 = 0;
   if constexpr (FLAT)
   {
      // One loop instead of {stages {bisection iterations}}.  In the nested form a wavefront stays in the bisection
      // loop of a stage as long as ANY of its paths does (24 % of the path-stages of a reverse sweep bisect, for
      // 5-15 iterations; with 8 paths per wavefront nearly every stage has such a path) while the paths whose first
      // check passed idle.  Here a path is either waiting for its next stage or inside a check, every pass of the
      // loop runs one check for all paths that are inside one, and the stage prologue (tableau combination, velocity
      // limit, spline evaluation) runs when a.hold/8 of the live paths are waiting for it, so that its cost is shared.
      // Paths of a wavefront drift apart in stage and step; nothing in a path's own arithmetic or order changes.
      int st = (dir == 1) ? 0 : 1;
      // state of this lane's path: one integer in a vector register on purpose (separate booleans become lane masks in
      // scalar registers that are merged under ever-changing exec masks across this loop)
      constexpr int PH_FIRST = 0, PH_ENDED = 1, PH_CHECK = 2, PH_DEAD = 3; // waiting for its first stage / a stage has ended / inside a check / finished
      int phase = PH_FIRST;
      if (sweep_curve_full(i, cap, revStart, (int64_t)t.segMVC)) { endStatus = BATOTP_ST_CAPACITY; phase = PH_DEAD; }
      double sN = 0, wN = 0;
      double lowFact = .01, sdotGood = 0, sdotL = 0, sdotH = 0, sdotTry = 0;
      int nGood = 0; // feasible points seen by the current bisection (anyGoodIter of ba.cpp:1254 == nGood > 0)
      int nIter = 0;
      for (;;)
      {
         const unsigned long long mAlive = __ballot(phase != PH_DEAD);
         if (mAlive == 0) break;
         const unsigned long long mWait = __ballot(phase < PH_CHECK);
         const bool startNow = (mWait == mAlive) || (__popcll(mWait) * 8 >= __popcll(mAlive) * a.hold);
         if (startNow && phase < PH_CHECK)
         {
            if (phase == PH_ENDED)
            {
               // the stage that just ended: keep its values (done here, once for all paths that wait, rather than
               // path by path at the pass in which each one's check ended)
               phase = PH_FIRST;
               const double vN = t.sdotCur;
               v1 = (st == 1) ? vN : v1; w1 = (st == 1) ? wN : w1;
               v2 = (st == 2) ? vN : v2; w2 = (st == 2) ? wN : w2;
               v3 = (st == 3) ? vN : v3; w3 = (st == 3) ? wN : w3;
               v4 = (st == 4) ? vN : v4; w4 = (st == 4) ? wN : w4;
               v5 = (st == 5) ? vN : v5; w5 = (st == 5) ? wN : w5;
               if (a.touch & 1)
               {
                  t.sink += pf;
                  pf = touch_ahead(t, j);
               }
               if (st < 6) ++st;
               else
               {
                  // FSAL shift and publish, ba.cpp:1096-1100 (stage 6: position sN, values vN, wN)
                  s0v = sN; v0 = vN; w0 = wN; w6 = wN;
                  sPrev = sCurPt; sdPrev = sdCurPt;
                  sCurPt = s0v; sdCurPt = v0;
                  if (writer) out[dir == 1 ? i : cap - 1 - i] = make_double2(s0v, v0);
                  st = (dir == 1) ? 0 : 1;
                  if (t.sCur * dir > sLast) { nPts = i + 1; phase = PH_DEAD; } // ba.cpp:1109-1115
                  else if (i > maxIntegSteps) { endStatus = BATOTP_ST_MAX_INTEG_TIME; phase = PH_DEAD; } // ba.cpp:1117-1122
                  else if (++i, sweep_curve_full(i, cap, revStart, (int64_t)t.segMVC)) { endStatus = BATOTP_ST_CAPACITY; phase = PH_DEAD; }
               }
            }
            if (phase != PH_DEAD)
            {
               if (st == 0)
               {
                  // forward predictor (ba.cpp:1055-1065): only the move of the reverse-curve cursor survives
                  t.sCur = s0v + h * v0;
                  mvc_walk(t);
                  st = 1;
               }
               const double *bc = rk[st];
               double sdotT = 0, sddotT = 0;
               // stage st adds the terms k < st only (a stale stage value may be infinite: 0 * inf must not enter the sum)
               sdotT += bc[0] * v0; sddotT += bc[0] * w0;
               { const double a1 = sdotT + bc[1] * v1, b1 = sddotT + bc[1] * w1; sdotT = (st > 1) ? a1 : sdotT; sddotT = (st > 1) ? b1 : sddotT; }
               { const double a2 = sdotT + bc[2] * v2, b2 = sddotT + bc[2] * w2; sdotT = (st > 2) ? a2 : sdotT; sddotT = (st > 2) ? b2 : sddotT; }
               { const double a3 = sdotT + bc[3] * v3, b3 = sddotT + bc[3] * w3; sdotT = (st > 3) ? a3 : sdotT; sddotT = (st > 3) ? b3 : sddotT; }
               { const double a4 = sdotT + bc[4] * v4, b4 = sddotT + bc[4] * w4; sdotT = (st > 4) ? a4 : sdotT; sddotT = (st > 4) ? b4 : sddotT; }
               { const double a5 = sdotT + bc[5] * v5, b5 = sddotT + bc[5] * w5; sdotT = (st > 5) ? a5 : sdotT; sddotT = (st > 5) ? b5 : sddotT; }
               sN = s0v + h * sdotT;
               double vN = v0 + h * sddotT;
               vN = dmax(vN, floorV); // ba.cpp:1085
               t.sCur = sN;
               sdot_lim(t, j, vN);
               t.sdotCur = vN;
               // sddotArr[st] keeps its previous value when the bisection fails (ba.cpp:1091 ignores the code)
               wN = (st == 1) ? w1 : (st == 2) ? w2 : (st == 3) ? w3 : (st == 4) ? w4 : (st == 5) ? w5 : w6;
               // applyAccelConstraintsBisectionPt, ba.cpp:1250-1265
               lowFact = .01; sdotGood = 0; nGood = 0; sdotL = 0; sdotH = vN; sdotTry = vN; nIter = 0;
               eval_partials(t, j);
               phase = PH_CHECK;
            }
         }
         if (phase == PH_CHECK)
         {
            // one pass of the loop of ba.cpp:1267-1321: the statements of apply_accel_bisection above, written as selects
            // (no divergent branches around the few operations of the update)
            const bool isViol = verify_second_order(t, j, sdotTry);
            const bool first = (nIter == 0);
            const bool good = !isViol && !first;                 // a feasible point after at least one violated one
            const bool shrink = isViol && nGood == 0;            // ba.cpp:1281-1285: no feasible point known yet
            const double lowFact2 = lowFact * 2.0;
            const double sdotLShrunk = dmax(.999 * 0.0, (1.0 - lowFact2) * sdotTry);
            // ba.cpp:1294-1303: two successive feasible points closer than 1e-3 (relative), or a negative one
            const bool conv = good && (ratio_lt(fabs(sdotTry - sdotGood), sdotTry, .001) || sdotTry < 0.0);
            const bool fin = (!isViol && first) || conv;
            lowFact = shrink ? lowFact2 : lowFact;
            sdotH = isViol ? sdotTry : sdotH;
            sdotL = shrink ? sdotLShrunk : ((good && !conv) ? sdotTry : sdotL);
            sdotGood = good ? sdotTry : sdotGood;
            nGood += good ? 1 : 0;
            t.sdotCur = conv ? sdotTry : t.sdotCur;
            // ba.cpp:1305-1320
            const bool collapsed = (nGood == 0) && ratio_lt(sdotH - sdotL, sdotH, 1e-20);
            const bool failed = !fin && (nIter + 1 > 100 || sdotTry < 0.0 || collapsed);
            nIter += fin ? 0 : 1;
            sdotTry = (fin || failed) ? sdotTry : .5 * (sdotH + sdotL);
            wN = fin ? ((dir == 1) ? t.sddotH : t.sddotL) : wN;
            t.status |= failed ? (unsigned)BATOTP_ST_BISECT_FAIL : 0u;
            t.nfail += failed ? 1 : 0;
            phase = (fin || failed) ? PH_ENDED : phase;
         }
      }
   }
   else
   {
      // the nested form: stages, and inside every stage the bisection loop of accel_pt
      bool done = false;
      while (!done)
      {
         if (sweep_curve_full(i, cap, revStart, (int64_t)t.segMVC)) { endStatus = BATOTP_ST_CAPACITY; break; }
         const double sStart = t.sCur;
         // st == 0: Euler predictor (ba.cpp:1055-1065).  Its sdot is overwritten by stage 6; all that
         // survives is the move of the reverse-curve cursor inside evalsdot (forward sweep only).
         // st == 1..6: the six stages of ba.cpp:1068-1094.  A real loop (not unrolled) keeps the
         // kernel inside the instruction cache.
#pragma unroll 1
         for (int st = (dir == 1 ? 0 : 1); st < 7; ++st)
         {
            double sN, vN, sdotT = 0, sddotT = 0;
            switch (st)
            {
            case 0: break;
            case 1: sdotT += BK_B00 * v0; sddotT += BK_B00 * w0; break;
            case 2: sdotT += BK_B01 * v0; sdotT += BK_B11 * v1; sddotT += BK_B01 * w0; sddotT += BK_B11 * w1; break;
            case 3:
               sdotT += BK_B02 * v0; sdotT += BK_B12 * v1; sdotT += BK_B22 * v2;
               sddotT += BK_B02 * w0; sddotT += BK_B12 * w1; sddotT += BK_B22 * w2;
               break;
            case 4:
               sdotT += BK_B03 * v0; sdotT += BK_B13 * v1; sdotT += BK_B23 * v2; sdotT += BK_B33 * v3;
               sddotT += BK_B03 * w0; sddotT += BK_B13 * w1; sddotT += BK_B23 * w2; sddotT += BK_B33 * w3;
               break;
            case 5:
               sdotT += BK_B04 * v0; sdotT += BK_B14 * v1; sdotT += BK_B24 * v2; sdotT += BK_B34 * v3; sdotT += BK_B44 * v4;
               sddotT += BK_B04 * w0; sddotT += BK_B14 * w1; sddotT += BK_B24 * w2; sddotT += BK_B34 * w3; sddotT += BK_B44 * w4;
               break;
            default:
               sdotT += BK_B05 * v0; sdotT += BK_B15 * v1; sdotT += BK_B25 * v2; sdotT += BK_B35 * v3; sdotT += BK_B45 * v4; sdotT += BK_B55 * v5;
               sddotT += BK_B05 * w0; sddotT += BK_B15 * w1; sddotT += BK_B25 * w2; sddotT += BK_B35 * w3; sddotT += BK_B45 * w4; sddotT += BK_B55 * w5;
               break;
            }
            if (st == 0)
            {
               // forward predictor: evalsdot's cursor walk at s0 + h*sdot0, nothing else is kept
               t.sCur = s0v + h * v0;
               mvc_walk(t);
               t.sCur = sStart;
               continue;
            }
            sN = s0v + h * sdotT;
            vN = v0 + h * sddotT;
            vN = dmax(vN, floorV); // ba.cpp:1085
            t.sCur = sN;
            BK_TICK(ta0);
            sdot_lim(t, j, vN);
            BK_TICK(ta1);
            BK_ACC(t.cycA, ta0, ta1);
            t.sdotCur = vN;
            // sddotArr[st] keeps its previous value when the bisection fails (ba.cpp:1091 ignores the code)
            double wN = (st == 1) ? w1 : (st == 2) ? w2 : (st == 3) ? w3 : (st == 4) ? w4 : (st == 5) ? w5 : w6;
            BK_TICK(tc0);
            accel_pt(t, j, wN);
            BK_TICK(tc1);
            BK_ACC(t.cycC, tc0, tc1);
            vN = t.sdotCur;
            switch (st)
            {
            case 1: v1 = vN; w1 = wN; break;
            case 2: v2 = vN; w2 = wN; break;
            case 3: v3 = vN; w3 = wN; break;
            case 4: v4 = vN; w4 = wN; break;
            case 5: v5 = vN; w5 = wN; break;
            default: s6v = sN; v6 = vN; w6 = wN; break;
            }
            // reverse sweep only (descending addresses; measured: -17 % there, +5 % on the forward sweep,
            // whose ascending walk finds the next lines already on their way): consume last stage's touch,
            // issue the next one
            if (a.touch & 1)
            {
               t.sink += pf;
               pf = touch_ahead(t, j);
            }
            if (dir == 1 && (a.touch & 2))
            {
               t.sink += pf2;
               pf2 = touch_curve_ahead(t, j);
            }
         }

         // FSAL shift and publish, ba.cpp:1096-1100
         s0v = s6v; v0 = v6; w0 = w6;
         sPrev = sCurPt; sdPrev = sdCurPt;
         sCurPt = s0v; sdCurPt = v0;
         if (writer) out[dir == 1 ? i : cap - 1 - i] = make_double2(s0v, v0);

         if (t.sCur * dir > sLast) { nPts = i + 1; done = true; } // ba.cpp:1109-1115
         else if (i > maxIntegSteps) { endStatus = BATOTP_ST_MAX_INTEG_TIME; break; } // ba.cpp:1117-1122
         else ++i;
      }
   }
   if (writer) a.sink[p] = t.sink + pf + pf2;
#ifdef BK_PROFILE_SECTIONS
   if (writer) { const unsigned long long tend = __builtin_readcyclecounter(); a.prof[4 * p + 0] = (double)t.cycA; a.prof[4 * p + 1] = (double)t.cycB; a.prof[4 * p + 2] = (double)(t.cycC - t.cycB); a.prof[4 * p + 3] = (double)(tend - tstart); }
#endif

   unsigned status = t.status | endStatus;
   if (endStatus != 0)
   {
      sweep_end_error(r, writer, dir, i, status, t.nfail);
      return;
   }

   sweep_end_snap(dir, sLast, sPrev, sdPrev, sCurPt, sdCurPt, dir == 1 ? t.mvc[(t.nMvc - 1) * 2 + 1] : 0.0);
   if (writer) out[dir == 1 ? nPts - 1 : cap - nPts] = make_double2(sCurPt, sdCurPt);
   int64_t nOut = nPts;
   if (nPts < 4)
   {
      status |= BATOTP_ST_SHORT; nOut = 4;
      if (writer)
      {
         // the points before the snapped one, from the curve
         double2 pt[3];
         for (int k = 0; k < 3; ++k) pt[k] = (k < (int)nPts - 1) ? out[dir == 1 ? k : cap - 1 - k] : make_double2(sCurPt, sdCurPt);
         sweep_short_to_four(dir, (int)nPts, absh, pt, out, cap);
      }
   }
   sweep_end_result(r, writer, dir, nOut, nPts, absh, status, t.nfail);
}

} // namespace bk
