// sweep8_fwd.hip.h -- the forward sweep of k_sweep8<8, FEAT, 1> (sweep8.hip.h) at hold 8, in lockstep.
//
// With hold 8 every live path of a wavefront starts every stage together and a path only dies at the end of a step, so the stage
// index is the same in all live lanes at all times.  k_sweep8's flat loop was built for paths that drift apart (the reverse sweep)
// and keeps the stage index and the phase per lane; this kernel keeps the lane mapping, SweepArgs, the bootstrap, every fp64
// operation and the termination conditions of k_sweep8<8, FEAT, 1> and replaces the control structure around them:
//   * an outer loop over integration steps, an inner loop over the stages 1..6, unrolled: the stage index is a constant in every
//     copy of the stage body and no lane-dependent value is ever assigned to it;
//   * one per-lane flag `alive` instead of the phase; a wavefront leaves when no lane is alive;
//   * the predictor (the move of the reverse-curve cursor) and the step end run once per step, without a ballot;
//   * the tableau combination has exactly the terms k < st with literal weights -- no zero weights, hence no sticky "a non-finite
//     stage value has been kept" flag and no guard for it.  (The rolled form -- `st` in a scalar register, the row of weights as one
//     scalar load from a constant table, `if (st > k)` around each term -- measured no faster than k_sweep8: the compiler turns those
//     uniform branches into selects and the stage-value copies into moves, 12 % MORE vector instructions; profiles/fwd_lockstep_*);
//   * the stage values v1..v5, w1..w6 stay in registers across stages and steps (k_sweep8 writes them to LDS at the end of a stage
//     and reads all five back at the start of the next one); a failed bisection leaves w_st of the previous step as it was;
//   * after the prologue of a stage ONE constraint check runs for all live paths; only if one of them is violated does the
//     bisection loop run, until every path of the wavefront has ended the stage.
// Kept as they are: the knot-cursor walk, the segment change over its window of two knots (knot_window.h, shared with k_sweep8: the
// load of the knot beyond is issued by every live lane and first read by the wavefront's next segment change), sweep8_mvcwalk.inc (the walk
// of the reverse-curve cursor over its register window, mvc_window.h: the one fragment both kernels include), the margin for curves in
// place, the staging of four curve points in LDS and the certified fast-forward (s8_certify); the entry of a path, the bootstrap and
// the ending of a path are sweep_frame.hip.h's, as in every sweep kernel.
// The arithmetic is a COPY of k_sweep8's with G = 8, DIR = +1 (shared are the walk's fragment and the two window headers, mvc_window.h and
// knot_window.h; a shared fragment of anything else would have to leave k_sweep8's code as it is).  A change on either side belongs on both:
//   here                                        sweep8.hip.h, k_sweep8
//   setup, loop state                           "stage_limits" .. "const int hold = a.hold" (lane mapping to the S8_PROFILE block)
//   checkPass                                   the block `if (phase == PH_CHECK)`: check, one pass of the bisection, s8_certify
//   tableau combination                         the `odd` (literal) branch of "tableau combination"
//   sdotLim, cursor walk, segment change,       the same-named sections of the prologue block (`if (phase < PH_CHECK)`)
//   theta' / theta''
//   "the stage that ended", step end            "the stage that ended: keep its values", `if (stepEnd)`
//   flush of the last group of four             `if (nPts >= 4)` after the loop
// Results are bit-identical to k_sweep8's and the oracle's (tests/test_gpu_sweep8_lockstep.py, and every test
// that drives forward hold 8).
#pragma once
#include "sweep8.hip.h"
#include <type_traits>

namespace bk
{

template <int FEAT>
__global__ void __launch_bounds__(S8_BLOCK, 2) k_sweep8_lock(SweepArgs a)
{
   static_assert(FEAT == -1 || FEAT == 0, "velocity / acceleration-only problems");
   constexpr int G = 8, DIR = 1;
   __shared__ double lim[6][8];
   __shared__ double2 pts[S8_BLOCK / G][4];    // curve points of a path waiting for their 64-byte store
   // rkB[st - 1][k] = weight of stage value k in stage st = 1..6 (column st-1 of ba.cpp:58-63); the stage loop is unrolled, so these
   // are literals in the code, and the entries k >= st (written 0 to fill the rows) are never read
   const double rkB[6][6] = {{BK_B00, 0, 0, 0, 0, 0},
                             {BK_B01, BK_B11, 0, 0, 0, 0},
                             {BK_B02, BK_B12, BK_B22, 0, 0, 0},
                             {BK_B03, BK_B13, BK_B23, BK_B33, 0, 0},
                             {BK_B04, BK_B14, BK_B24, BK_B34, BK_B44, 0},
                             {BK_B05, BK_B15, BK_B25, BK_B35, BK_B45, BK_B55}};
   stage_limits(a.dP, lim);

   const int lane = threadIdx.x & 63;
   const int wave = blockIdx.x * (S8_BLOCK / 64) + (threadIdx.x >> 6);
   const int j = lane % G;
   const int slot = lane / G;
   const int pslot = wave * a.ppw + slot;
   if (slot >= a.ppw || pslot >= a.B) return; // whole groups leave together; DPP never crosses groups
   const int p = a.order ? a.order[pslot] : pslot;
   const bool writer = (j == 0);
   const PathInfo pi = a.pinfo[p];
   const int n = (int)pi.n;
   const int64_t cap = a.cap;
   double2 *mypts = pts[threadIdx.x / G];

   // bootstrap (ba.cpp:1021-1041) through the general kernel's device functions; the loop below carries its own state
   Pt<G, FEAT, true> t;
   pt_init(t, a.P, pi, a.sC, a.coef, a.km, lim, j, DIR);

   double2 *out = a.fwd + (int64_t)p * cap; // may alias the reverse curve (curves in place)
   batotp_path_result *__restrict__ r = a.res + p;
   const int64_t nRev = r->n_rev;
   if (nRev < 2)
   {
      sweep_no_reverse_curve(r, writer);
      return;
   }
   const double2 *mvc = a.rev + (int64_t)p * cap + (cap - nRev); // the reverse curve the forward sweep follows
   const int nMvc = (int)nRev;
   t.mvc = reinterpret_cast<const double *>(mvc);
   t.nMvc = nMvc;

   const double absh = pi.integ_res;
   const double h = absh;
   const double sres = pi.sres_c;
   const double sEnd = sres * (double)(n - 1);
   double s0v = 0.0;
   double v0, w0 = 0;
   pt_bootstrap(t, j, DIR, n, h, s0v, v0, w0);
   const double vBoot = v0;

   // ---- the loop's own state (k_sweep8's, one joint per lane) -------------------------------------
   const bool jOn = j < t.nJ;
   const int jAt = jOn ? j : 0;
   const double vmax = t.vmax[0], amax = t.amax[0];
   // this lane's coefficients on the cursor's segment: c1, 2 c2, 3 c3, 6 c3; theta', theta'' of the last evaluation point; the
   // refined reciprocal of theta' (sdiv_rcp) and whether theta' lies in the window in which it may be used
   double c1 = jOn ? t.rowTh[0].c1 : 0.0, c2x2 = jOn ? 2 * t.rowTh[0].c2 : 0.0;
   double c3x3 = jOn ? 3 * t.rowTh[0].c3 : 0.0, c3x6 = jOn ? 6 * t.rowTh[0].c3 : 0.0;
   double thD = t.thD[0], thD2 = t.thD2[0];
   bool rOk = sdiv_window(thD);
   double rD = sdiv_rcp(thD);
   // the lane masks the guards of a stage combine (S8_MASK, sweep8.hip.h): per-lane constants once, rOk beside the bool
   s8_mask mROk = S8_MASK_WINDOW(thD);
   const s8_mask mJOn = S8_MASK(j < t.nJ), mVmaxOk = S8_MASK_WINDOW(vmax);
   const bool accOn = (t.flags & BATOTP_F_JNT_ACC_ON) != 0;
   const double thrV = t.thrV, thrA = t.thrA, vfact = t.vfact, afact = t.afact;
   const double sdotCap = t.sdotCap, sddotMax = t.sddotMax, sdotMin = t.sdotMin;
   const bool capOk = (sddotMax == sddotMax); // the acceleration cap is not a NaN (otherwise every bound takes the literal form)
   const int lastSeg = n - 2;
   const int nIn = t.nIn;
   const double2 *__restrict__ km = t.km;
   const double *__restrict__ coef = t.coef;
   const int rowStride = t.C * 4;
   int seg = t.segC, rowSeg = t.rowSeg;
   // knot window (compact pairs, knot_window.h): knot rowSeg + 1 and the one beyond it, as (y, y'') each
   double kEdgeY = 0, kEdgeSol = 0, kPreY = 0, kPreSol = 0;
   int preIdx = KNOT_WINDOW_NONE; // knot index the prefetch pair holds (and the edge pair holds preIdx - 1): none yet
   // reverse-curve cursor: segment, its two points and the window's two neighbours (mvc_window.h; indices clamped to the curve)
   int segM = t.segMVC;
   double mS0, mD0, mS1, mD1, mSLo, mDLo, mSHi, mDHi;
   {
      const double2 qa = mvc[segM], qb = mvc[segM + 1], ql = mvc[mvc_window_lo(segM)], qh = mvc[mvc_window_hi(segM, nMvc)];
      mS0 = qa.x; mD0 = qa.y; mS1 = qb.x; mD1 = qb.y;
      mSLo = ql.x; mDLo = ql.y; mSHi = qh.x; mDHi = qh.y;
   }
   unsigned status = t.status;
   int nfail = t.nfail;
   double sdotCur = t.sdotCur;
   double sddotH = t.sddotH;

   double v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0;
   double w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, w6 = 0;
   double sCur = s0v; // traj.sCur

   const int iMax = sweep_max_steps_int(a.P, pi);
   const int capI = (int)cap;
   const int revStartI = sweep_rev_start_int(a, nMvc, DIR); // curves in place: slot i must have been left behind by the reverse-curve cursor

   // point 0: straight to HBM, and into the group of four it belongs to
   if (writer) { out[0] = make_double2(s0v, v0); mypts[0] = make_double2(s0v, v0); }

   const double floorV = 0.0 / absh; // ba.cpp:1050-1051,1085
   // the clamp chain of the prologue may take its one-instruction form (device_math.h, clamp_chain_fast): the path's part of the condition
   // (clamp_consts_ok's comparisons, as the mask the stage's guard combines)
   const s8_mask mClampLit = ~(S8_MASK(floorV == floorV) & S8_MASK(sdotMin > 0.0) & S8_MASK(sdotCap == sdotCap));
   int i = 1;   // the step in progress; a path that reaches its end has i + 1 points
   unsigned endStatus = 0;
   bool alive = true;
   if (sweep_curve_full(i, capI, revStartI, segM)) { endStatus = BATOTP_ST_CAPACITY; alive = false; }
   double sN = 0, wN = 0;
   double lowFact = .01, sdotGood = 0, sdotL = 0, sdotH = 0, sdotTry = 0;
   int nGood = 0, nIter = 0;
   bool stageFailed = false; // the bisection of the stage failed: sddotArr[st] keeps its previous value (ba.cpp:1091 ignores the code)
#ifdef S8_PROFILE
   // as in k_sweep8; a "pass" here is a constraint check of the wavefront (the first one of a stage follows its prologue directly)
   double pc[16];
   for (int k = 0; k < 16; ++k) pc[k] = 0;
   const unsigned long long tLoop0 = __builtin_readcyclecounter();
#endif

   // One pass of the loop of ba.cpp:1267-1321 for the active lanes: the constraint check at sdotTry and the bisection update
   // (k_sweep8's check block).  FIRST: the first check of the stage, nIter == 0 in every lane; a lane in any later pass has
   // nIter >= 1 (the first pass counts it, the fast-forward only counts up).  Returns whether the lane's stage has ended;
   // `more` (FIRST only, wavefront-uniform): some lane's stage goes on.
   auto checkPass = [&](auto firstTag, bool &more) -> bool {
      constexpr bool FIRST = decltype(firstTag)::value;
      const double lowFact2 = lowFact * 2.0;
      const double sdotLShrunk = dmax(.999 * 0.0, (1.0 - lowFact2) * sdotTry);
      bool dec1, dec2;
      const double num1 = fabs(sdotTry - sdotGood), num2 = sdotTry - sdotLShrunk;
      bool close, tiny;
      s8_ratio_lt_pair(num1, num2, sdotTry, close, dec1, tiny, dec2);
      // ---- verifySecondOrderConstraints, ba.cpp:1514-1534, at sdotTry ---------------------------------
      const double sdotSQ = sdotTry * sdotTry;
      double H = sddotMax, L = -sddotMax;
      bool force = false;
      if (accOn)
      {
         const bool slow = fabs(thD) < thrV;
         const double vTerm = thD2 * sdotSQ;
         const double sa = (thD < 0.0) ? -amax : amax;   // amax with the sign of theta' (ba.cpp:1526-1531)
         const double nH = sa - vTerm, nL = -sa - vTerm; // (theta' = 0 lies outside the window: the literal form below)
         const bool fast = capOk & rOk & sdiv_window(nH) & sdiv_window(nL);
         const double qH = sdiv_by(nH, thD, rD);
         const double qL = sdiv_by(nL, thD, rD);
         const bool use = jOn & !slow & fast;
         const double Hm = vmin_f64(H, qH), Lm = vmax_f64(L, qL);
         H = use ? Hm : H;
         L = use ? Lm : L;
         // a joint that stands still, or a quotient outside the window of the shared reciprocal
         if (S8_RARE(jOn & (slow | !fast)))
         {
            S8_CNT(12, 1);
            const int svpt = sgn(thD);
            const double nHl = svpt * amax - vTerm, nLl = -svpt * amax - vTerm;
            if (jOn && !slow && !fast)
            {
               H = dmin(H, nHl / thD);
               L = dmax(L, nLl / thD);
            }
            // a joint that stands still (ba.cpp:1519-1524)
            if (jOn && slow && !(fabs(thD2) < thrA)) force |= sdotSQ > amax / fabs(thD2);
         }
      }
      double Hred = force ? -kInf : H;
      grp_min_max<G>(Hred, L);
      sddotH = Hred;
      const bool isViol = L > Hred;

      const bool fin0 = !isViol && FIRST; // the first check passes: the stage is done, nothing else happens
      bool fin = fin0, failed = false;
      more = false;
      // 99 % of the first checks end here
      if (!FIRST || S8_ANY(!fin0))
      {
         const bool good = !isViol && !FIRST;      // a feasible point after at least one violated one
         const bool shrink = isViol && nGood == 0; // ba.cpp:1281-1285: no feasible point known yet
         // the two threshold tests of the loop (computed above), behind ONE guard for the quotients they may need
         if (S8_RARE((good & !dec1) | (shrink & !dec2)))
         {
            close = dec1 ? close : (num1 / sdotTry < .001);
            tiny = dec2 ? tiny : (num2 / sdotTry < 1e-20);
         }
         const bool conv = good && (close || sdotTry < 0.0);
         fin = fin0 || conv;
         lowFact = shrink ? lowFact2 : lowFact;
         sdotH = isViol ? sdotTry : sdotH;
         sdotL = shrink ? sdotLShrunk : ((good && !conv) ? sdotTry : sdotL);
         sdotGood = good ? sdotTry : sdotGood;
         nGood += good ? 1 : 0;
         sdotCur = conv ? sdotTry : sdotCur;
         // ba.cpp:1305-1320
         const bool collapsed = shrink && tiny;
         failed = !fin && (nIter + 1 > 100 || sdotTry < 0.0 || collapsed);
         nIter += fin ? 0 : 1;
         sdotTry = (fin || failed) ? sdotTry : .5 * (sdotH + sdotL);
         status |= failed ? (unsigned)BATOTP_ST_BISECT_FAIL : 0u;
         nfail += failed ? 1 : 0;
         stageFailed = failed;
         // the certified fast-forward of the bisection (s8_certify): the first check of the stage was violated and the loop goes on
         if (FIRST && accOn)
         {
            const bool ffWant = ((a.ff & 1) != 0) && isViol && !failed;
            if (S8_ANY(ffWant))
            {
               S8_CNT(11, 1);
               if (ffWant)
                  s8_certify(jOn, thD, thD2, rD, rOk, amax, thrV, thrA, sddotMax, lowFact, sdotH, sdotL, sdotTry, sdotGood, nGood, nIter);
            }
         }
         if (FIRST) more = S8_ANY(!(fin || failed));
      }
      wN = fin ? sddotH : wN;
      return fin || failed;
   };

   for (;;)
   {
      if (!S8_ANY(alive)) break;
      if (alive)
      {
         // ---- forward predictor (ba.cpp:1055-1065): only the move of the reverse-curve cursor survives ----
         sCur = s0v + h * v0;
#include "sweep8_mvcwalk.inc"
#pragma unroll
         for (int st = 1; st <= 6; ++st)
         {
            S8_TICK(tA);
            S8_CNT(1, 1); S8_CNT(2, __popcll(__ballot(1)) / G);
            // ---- tableau combination, ba.cpp:1073-1085: the terms k < st ------------------------------
            const double *bc = rkB[st - 1];
            const double b0 = bc[0], b1 = bc[1], b2 = bc[2], b3 = bc[3], b4 = bc[4], b5 = bc[5];
            double sdotT = 0, sddotT = 0;
            sdotT += b0 * v0; sddotT += b0 * w0;
            if (st > 1) { sdotT += b1 * v1; sddotT += b1 * w1; }
            if (st > 2) { sdotT += b2 * v2; sddotT += b2 * w2; }
            if (st > 3) { sdotT += b3 * v3; sddotT += b3 * w3; }
            if (st > 4) { sdotT += b4 * v4; sddotT += b4 * w4; }
            if (st > 5) { sdotT += b5 * v5; sddotT += b5 * w5; }
            sN = s0v + h * sdotT;
            const double vRaw = v0 + h * sddotT;
            sCur = sN;

            // ---- the floor of ba.cpp:1085 and sdotLim, ba.cpp:1204-1236 (theta' of the PREVIOUS evaluation point) -----------------
            // evalsdot, ba.cpp:1590-1607
#include "sweep8_mvcwalk.inc"
            const double tauM = (sCur - mS0) / (mS1 - mS0);
            const double sdotRev = mD0 + tauM * (mD1 - mD0);
            // max(., floorV), the reverse curve's speed (itself at least sdotMin), sdotCap, sdotMin: four v_max / v_min (device_math.h)
            double vN = clamp_chain_fast<true>(vRaw, sdotRev, floorV, sdotMin, sdotCap);
            {
               double lim1 = kInf;
               const bool on = jOn && fabs(thD) > thrV;
               const bool fast = rOk & sdiv_window(vmax);
               const double qv = fabs(sdiv_by(vmax, thD, rD));
               lim1 = (on & fast) ? dmin(lim1, qv) : lim1;
               // the straight-line code first: the reduction and the last clamp for the ordinary case ...
               vN = vmin_f64(vN, grp_min<G>(lim1));
               // ... and ONE guard for what is rare here, which then forms vN again: a velocity-limit quotient outside the window of the shared
               // reciprocal, and a clamp chain that must run literally (a NaN among its operands, sdotMin <= 0); the literal chain is right
               // for every lane, so all lanes take it
               const s8_mask mRareV = (mJOn & S8_MASK(fabs(thD) > thrV) & ~(mROk & mVmaxOk)) | (mClampLit & S8_EXEC()) | S8_MASK(!clamp_raw_ok(vRaw, sdotRev));
               if (__builtin_expect(mRareV != 0, 0))
               {
                  if (on && !fast) lim1 = dmin(lim1, fabs(vmax / thD));
                  vN = dmin(clamp_chain_literal<true>(vRaw, sdotRev, floorV, sdotMin, sdotCap), grp_min<G>(lim1));
               }
            }
            sdotCur = vN;
            // applyAccelConstraintsBisectionPt, ba.cpp:1250-1265
            lowFact = .01; sdotGood = 0; nGood = 0; sdotL = 0; sdotH = vN; sdotTry = vN; nIter = 0; stageFailed = false;

            // ---- evalSplinePartials, ba.cpp:1341-1413: updateCurSeg (ba.cpp:1617-1652) on the sites sres*k ----
            // (the sites of the cursor's segment are formed anew in every stage, here: two products against four registers held throughout
            //  -- k_sweep8 keeps them; the walk below forms them again only after the cursor has moved, as k_sweep8's does)
            double sSeg = sres * (double)seg, sNext = sres * (double)(seg + 1);
            if (S8_ANY(!((sCur >= sSeg) & (sCur <= sNext))))
            {
               S8_CNT(10, 1);
               for (;;)
               {
                  sSeg = sres * (double)seg;
                  sNext = sres * (double)(seg + 1);
                  const bool inside = (sCur >= sSeg) & (sCur <= sNext);
                  const bool up = !inside & (sCur > sSeg), down = !inside & (sCur < sSeg);
                  status |= (!inside & !up & !down) ? (unsigned)BATOTP_ST_NONFINITE : 0u;
                  const bool mvUp = up & (seg < lastSeg), mvDn = down & (seg > 0);
                  seg = mvUp ? seg + 1 : (mvDn ? seg - 1 : seg);
                  if (!S8_ANY(mvUp | mvDn)) break;
               }
            }
            const double tau = (sCur - sSeg) / (sNext - sSeg);
            const bool chg = (seg != rowSeg);
            if (S8_ANY(chg))
            {
               S8_CNT(9, 1);
               if (chg)
               {
                  if (FEAT < 0)
                  {
                     const unsigned at = (unsigned)(seg * nIn + jAt);
                     // one segment further in the direction of the sweep: both knots (seg and seg + 1 of this joint) are in registers
                     // (as four scalars: selecting between double2 values sends them through scratch)
                     double yL = kEdgeY, solL = kEdgeSol, yR = kPreY, solR = kPreSol;
                     bool literal = !knot_window_hit(preIdx, seg, DIR); // the knots are not the window's, or a sixth lies outside div6's window
                     // emit_segment's formulas (spline.cpp:203-209); x / 6 as div6 computes it inside its window, and ONE
                     // wavefront-uniform guard for everything that is rare here (a missed prefetch, a sixth outside the window)
                     const double xa = solR - solL, xb = solR + 2 * solL;
                     literal |= !((fabs(xa) > 1e-280) & (fabs(xa) < 1e280) & (fabs(xb) > 1e-280) & (fabs(xb) < 1e280));
                     double c3, sixthB;
                     {
                        const double qa = xa * (1.0 / 6.0), qb = xb * (1.0 / 6.0);
                        c3 = __builtin_fma(__builtin_fma(-6.0, qa, xa), 1.0 / 6.0, qa);
                        sixthB = __builtin_fma(__builtin_fma(-6.0, qb, xb), 1.0 / 6.0, qb);
                     }
                     if (S8_RARE(literal))
                     {
                        const bool hit = knot_window_hit(preIdx, seg, DIR);
                        const double2 dl = km[at], dr = km[at + nIn];
                        yL = hit ? yL : dl.x; solL = hit ? solL : dl.y;
                        yR = hit ? yR : dr.x; solR = hit ? solR : dr.y;
                        c3 = div6(solR - solL);
                        sixthB = div6(solR + 2 * solL);
                     }
                     knot_window_shift(true, DIR, yL, solL, yR, solR, kEdgeY, kEdgeSol);
                     const double c2 = solL / 2.0;
                     c1 = yR - yL - sixthB;
                     c2x2 = 2 * c2; c3x3 = 3 * c3; c3x6 = 6 * c3;
                     preIdx = knot_window_mark(seg, lastSeg, DIR);
                  }
                  else
                  {
                     const Coef4 k = *reinterpret_cast<const Coef4 *>(coef + (unsigned)(seg * rowStride) + jAt * 4);
                     c1 = k.c1; c2x2 = 2 * k.c2; c3x3 = 3 * k.c3; c3x6 = 6 * k.c3;
                  }
                  rowSeg = seg;
               }
               if (FEAT < 0)
               {
                  // the window's load (knot_window.h): every live lane, changed or not, straight into the prefetch registers; the next
                  // segment-change block of the wavefront is the first to read them
                  const double2 kq = km[(unsigned)(knot_window_load(seg, lastSeg, DIR) * nIn + jAt)];
                  kPreY = kq.x; kPreSol = kq.y;
               }
            }
            {
               const double tau2 = tau * tau;
               thD = (c3x3 * tau2 + c2x2 * tau + c1) * vfact;
               thD2 = (c3x6 * tau + c2x2) * afact;
               rOk = sdiv_window(thD);
               // (a wavefront-wide mask assigned inside `if (alive)` and carried across steps: only the bits of the lanes active HERE are
               //  renewed, the bits of a lane that has died are stale from then on.  That is harmless because a dead lane never comes back
               //  and every use ANDs the mask with a comparison taken on the spot, which holds active lanes only -- keep it so.)
               mROk = S8_MASK_WINDOW(thD);
               rD = sdiv_rcp(thD);
            }
            S8_TICK(tB);
            S8_CYC(5, tA, tB);

            // ---- the stage's constraint check; the bisection loop only if some path is violated ----------
            S8_CNT(0, 1); S8_CNT(3, 1); S8_CNT(4, __popcll(__ballot(1)) / G); S8_CNT(13, __popcll(__ballot(1)) / G);
            bool more;
            bool ended = checkPass(std::true_type(), more);
            while (more)
            {
               S8_CNT(0, 1); S8_CNT(3, 1); S8_CNT(4, __popcll(__ballot(!ended)) / G); S8_CNT(13, __popcll(__ballot(1)) / G);
               if (!ended)
               {
                  bool unused;
                  ended = checkPass(std::false_type(), unused);
               }
               more = S8_ANY(!ended);
            }
            S8_TICK(tC);
            S8_CYC(6, tB, tC);

            // ---- the stage that ended: keep its values (a failed bisection leaves sddotArr[st] as it was) ----
            if (st == 1) { v1 = sdotCur; w1 = stageFailed ? w1 : wN; }
            if (st == 2) { v2 = sdotCur; w2 = stageFailed ? w2 : wN; }
            if (st == 3) { v3 = sdotCur; w3 = stageFailed ? w3 : wN; }
            if (st == 4) { v4 = sdotCur; w4 = stageFailed ? w4 : wN; }
            if (st == 5) { v5 = sdotCur; w5 = stageFailed ? w5 : wN; }
         }
         // ---- step end: FSAL shift and publish, ba.cpp:1096-1100 (stage 6: position sN, values sdotCur, wN or the stale sddotArr[6])
         {
            S8_CNT(8, 1);
            const double vN = sdotCur;
            const double wE = stageFailed ? w6 : wN;
            s0v = sN; v0 = vN; w0 = wE; w6 = wE;
            const int idx = i;
            mypts[idx & 3] = make_double2(s0v, v0); // every lane of the group holds the same pair
            const bool fin = sCur > sres * (double)(lastSeg + 1); // ba.cpp:1109-1115 (the path end sres (n - 1), as below)
            const bool late = !fin && (i > iMax);     // ba.cpp:1117-1122
            i = (fin || late) ? i : i + 1;
            const bool full = !fin && !late && sweep_curve_full(i, capI, revStartI, segM);
            endStatus = late ? (unsigned)BATOTP_ST_MAX_INTEG_TIME : (full ? (unsigned)BATOTP_ST_CAPACITY : endStatus);
            alive = !(fin || late || full);
            // a complete group of four points: one 64-byte store (not for the step that ends the path: its last point is
            // still to be snapped onto the path end)
            const bool chunk = !fin && ((idx & 3) == 3);
            if (chunk)
            {
               const int base = idx & ~3;
               const int at = base + j;
               if (j < 4 && at >= base && at <= idx) out[at] = mypts[j];
            }
         }
      }
   }
#ifdef S8_PROFILE
   pc[7] = (double)(__builtin_readcyclecounter() - tLoop0);
   if (lane == 0 && a.prof)
      for (int k = 0; k < 16; ++k) a.prof[(int64_t)wave * 16 + k] = pc[k];
#endif

   status |= endStatus;
   if (endStatus != 0)
   {
      sweep_end_error(r, writer, DIR, i, status, nfail);
      return;
   }

   // The last two published points: (s0v, v0), and the one before it, which is still in the group of four in LDS (point 0 went
   // there too)
   const int nPts = i + 1;
   double sCurPt = s0v, sdCurPt = v0;
   const double2 qPrev = mypts[(nPts - 2) & 3];
   const double sPrev = qPrev.x, sdPrev = qPrev.y;
   sweep_end_snap(DIR, sEnd, sPrev, sdPrev, sCurPt, sdCurPt, mvc[nMvc - 1].y);
   int64_t nOut = nPts;

   if (nPts >= 4)
   {
      // the snapped point joins the points still waiting in LDS; what has not reached HBM yet goes now
      const int idxLast = nPts - 1;
      mypts[idxLast & 3] = make_double2(sCurPt, sdCurPt);
      const int base = idxLast & ~3;
      const int at = base + j;
      if (j < 4 && at <= idxLast) out[at] = mypts[j]; // (complete groups of four have gone: everything below `base` is in HBM)
   }
   else
   {
      // The points of so short a curve are all still here: point 0 = the start, point nPts-2 = (sPrev, sdPrev), point nPts-1 = the
      // snapped end.
      status |= BATOTP_ST_SHORT; nOut = 4;
      if (writer)
      {
         const double2 snapped = make_double2(sCurPt, sdCurPt);
         const double2 pt[3] = {make_double2(0.0, vBoot), nPts == 2 ? snapped : make_double2(sPrev, sdPrev), snapped};
         sweep_short_to_four(DIR, nPts, absh, pt, out, cap);
      }
   }
   sweep_end_result(r, writer, DIR, nOut, nPts, absh, status, nfail);
}

} // namespace bk
