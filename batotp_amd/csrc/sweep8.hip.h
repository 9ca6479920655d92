// sweep8.hip.h -- K4 for large batches of velocity / acceleration-only problems (round 4): the flat stage / bisection loop of
// k_sweep<8, FEAT <= 0, true, true> (sweep_general.hip.h) written for the instruction count.
//
// Same decomposition: a path = 8 lanes (lane j = joint j), up to 8 paths per wavefront, every path of a wavefront is either
// waiting for its next stage or inside a constraint check; a pass of the loop runs the stage prologue for the waiting paths
// once `hold`/8 of the live paths wait, then one constraint check + bisection update for every path inside one.  Same
// arithmetic: every fp64 operation of BA::sweep (ba.cpp:979-1195), sdotLim (:1204-1236), evalsdot (:1590-1607), updateCurSeg
// (:1617-1652), applyAccelConstraintsBisectionPt (:1248-1332), evalSplinePartials (:1341-1413) and
// verifySecondOrderConstraints (:1514-1534, joint acceleration family) in the reference's order, uncontracted.
//
// What differs from the general kernel is the code around the arithmetic (profiles/r03_c: a third of its loop was exec-mask
// bookkeeping the compiler generated for nested divergent branches and loops with several exits):
//   * one level of divergence per block (waiting paths / checking paths); everything inside is straight-line select code;
//   * the segment walks are wavefront-uniform loops ("while any lane moved") over select-form steps;
//   * rare cases (a joint that stands still, a threshold test that needs its true quotient, a segment change, the end of a
//     step) sit behind wavefront-uniform branches on ballots and cost nothing when no lane needs them;
//   * the reverse-curve segment of the forward sweep and its two neighbouring points are kept in registers (mvc_window.h): a move
//     takes the entering point from there, and a pass of the walk in which some path moves issues two 16-byte loads in every lane,
//     of the two neighbours of the lane's (new) segment, that nothing reads before the next such pass;
//   * curve points leave through LDS, four at a time: one 64-byte store per path and four steps instead of four 16-byte
//     stores (the reverse sweep's 16 384 descending streams lost their partly written lines from the L2 between the stores:
//     3.0x the curve bytes written, profiles/r03_e).
// Results are bit-identical to k_sweep's (every sweep test runs both; tests/test_gpu_parity.py, tests/test_gpu_fuzz.py).
// The entry of a path, the tableau and the ending of a path are sweep_frame.hip.h's.
#pragma once
#include "sweep_frame.hip.h"
#include "mvc_window.h"
#include "knot_window.h"

// diagnostic build (-DS8_PROFILE): what a wavefront of k_sweep8 spends its passes and cycles on, 16 doubles per wavefront in
// SweepArgs::prof (tools/sweep8_sections.py); no effect otherwise
#ifdef S8_PROFILE
#define S8_CNT(k, v) pc[k] += (double)(v)
#define S8_TICK(var) const unsigned long long var = __builtin_readcyclecounter()
#define S8_CYC(k, a, b) pc[k] += (double)((b) - (a))
#else
#define S8_CNT(k, v)
#define S8_TICK(var)
#define S8_CYC(k, a, b)
#endif

namespace bk
{

constexpr int S8_BLOCK = 256;
// "does any active lane ...": the i1 ballot intrinsic (HIP's __ballot goes through an integer compare: a v_cndmask + v_cmp per use)
#define S8_ANY(x) (__builtin_amdgcn_ballot_w64(x) != 0)
#define S8_RARE(x) __builtin_expect(S8_ANY(x), 0) // a guard whose block is off the straight-line code
// The lane mask of ONE COMPARISON over the active lanes, as a 64-bit scalar.  The ballot of a comparison is the v_cmp itself; the ballot of
// anything else (a & b, a bool that was assigned earlier, a bool that also feeds integer arithmetic) is lowered to v_cndmask_b32 v, 0, 1, mask
// -> v_cmp_ne_u32 0, v: two vector instructions and their latency in front of a branch the whole wavefront waits for.  So a guard on several
// conditions combines the masks of its comparisons with scalar & and | -- (S8_MASK(a) & S8_MASK(b)) != 0 -- and the per-lane bools serve the
// selects only.  Every S8_MASK holds active lanes only; a mask carried from a place where more lanes were active (a per-lane constant, a
// value of the previous stage) is always ANDed with one taken on the spot.
typedef unsigned long long s8_mask;
#define S8_MASK(cmp) __builtin_amdgcn_ballot_w64(cmp)
#define S8_EXEC() __builtin_amdgcn_ballot_w64(true) // the active lanes
// sdiv_window(x) (device_math.h) as a mask: the same two comparisons, so the compiler emits them once for the bool and the mask
#define S8_MASK_WINDOW(x) (S8_MASK(fabs(x) >= SDIV_LO) & S8_MASK(fabs(x) <= SDIV_HI))
// Measured and settled, no longer switches (DESIGN.md 4 has the numbers):
//   kept: tableau combination without selects, stage values in LDS, walk pre-check, knot prefetch (round 4, profiles/r04_a_*)
//   kept: the certified fast-forward in both directions (profiles/r04_j_*), in the reverse sweep as a phase of its own (profiles/r06_a_*)
//   removed: the cursor quotients through cached reciprocals, 4-7 % slower (profiles/r05_e_*, r06_a_*)
//   removed: both next candidates beside the test in the certificate's replay, 2.3 % slower (profiles/r06_p_*)
//   kept: the reverse curve around the cursor in registers, its loads off the stage's dependent chain (mvc_window.h; forward launch of
//         the headline 1655 -> 1537 ms in k_sweep8_lock, profiles/fwd_curve_window_*).  (Round 4's prefetch of the next point alone, selected
//         into place per lane, had measured 5 % slower -- 440 against 419 ms: the select waits for the load where it stands.)
//   kept: the knots of the compact layout as a register window around the knot cursor, the load of the knot beyond issued by every lane
//         of a segment-change block and first read by the next such block (knot_window.h; both directions, G = 8 and 4, and k_sweep8_lock:
//         headline reverse launch 3015 -> 2854 ms, forward launch 1538 -> 1410 ms, profiles/knot_window_*).  The knots are held as four
//         scalars: the double2 selects of the literal route had cost the FEAT -1 kernels 80 bytes of scratch and two scratch stores per change.
//   kept: the clamps of the prologue (floor, reverse curve's speed, sdotCap, sdotMin, lim1) as single v_max_f64 / v_min_f64 where no operand is
//         a NaN and sdotMin > 0, the literal chain behind the rare guard the section already had (device_math.h, clamp_chain_fast; converted
//         and unconverted clamps site by site: DESIGN.md 4, "The stage's clamps as single instructions"); in k_sweep8_lock also the exit test of the
//         reverse-curve walk and that rare guard on the lane masks of their comparisons (S8_MASK above): headline forward launch 1408 -> 1337 ms
//         (development builds: clamps 1407 -> 1359, guards -> 1342), the reverse launch does not move with the clamps; profiles/stage_chain_*
//   kept: the replay loops of s8_certify with exit tests on the masks of their comparisons and no `more` carried between passes: headline reverse
//         launch 2850 -> 2832 ms, 13 - 19 ms over two visits against a gate of 14 ms: at the edge of what a launch time tells, not claimed
//   removed: the same treatment of the flat loop's own guards (threshold quotients, the check's rare guard, standing joint, chunk test): reverse
//         launch 2852 -> 2892 ms, 41 ms SLOWER with four round trips fewer per pass (three to ten scalar instructions for each v_cndmask / v_cmp_ne
//         pair); `odd` and the guards inside k_sweep8_lock's bisection block cost VGPRs in mask form (163 / 193 against 161 / 185) and stayed bools

// (num / den) < thr as ratio_lt (kernels.hip.h) decides it, in two parts: the product form, and whether it was decisive
__device__ __forceinline__ bool s8_ratio_lt_fast(double num, double den, double thr, bool &decided)
{
   const double p = thr * den;
   // thr > 0: p > 1e-290 implies den > 0, and for a positive divisor the product form is right for a numerator of either sign
   const bool ok = (p > 1e-290) & (p < 1e290);
   const bool lt = num < p * (1.0 - 1e-14), gt = num > p * (1.0 + 1e-14);
   decided = ok & (lt | gt);
   return lt;
}
// The two threshold tests of one bisection pass divide by the same den: num1 / den < THR1 and num2 / den < THR2 with the
// thresholds of ba.cpp:1294 and 1313 (1e-3, 1e-20).  A test is decided when the numerator lies outside the band
// den * thr * (1 -+ 1e-14): the quotient's rounding error (2^-53) cannot carry it across thr from there.  (The bounds of the band
// are single products with constants; where exactly the band ends is immaterial, inside it the literal quotient decides.)
// den in (1e-260, 1e260): positive, and every product is a normal number.
__device__ __forceinline__ void s8_ratio_lt_pair(double num1, double num2, double den, bool &lt1, bool &dec1, bool &lt2, bool &dec2)
{
   constexpr double T1 = .001, T2 = 1e-20;
   const bool ok = (den > 1e-260) & (den < 1e260);
   lt1 = num1 < den * (T1 * (1.0 - 1e-14));
   lt2 = num2 < den * (T2 * (1.0 - 1e-14));
   dec1 = ok & (lt1 | (num1 > den * (T1 * (1.0 + 1e-14))));
   dec2 = ok & (lt2 | (num2 > den * (T2 * (1.0 + 1e-14))));
}
// (the shared refined reciprocal of theta' -- sdiv_window / sdiv_rcp / sdiv_by -- lives in device_math.h.  In k_sweep1, the
// one-path-per-wavefront kernel, the same technique measured 3-10 % SLOWER -- cfg 4: 961 against 874 ms -- and is not used there:
// its window tests and ballot guards cost a lone wavefront more than the shorter quotients save; profiles/r04_b_*)

// known-answer test of the shared-reciprocal division against `/` (batotp_hip_fp64_kat)
__global__ void k_kat_sdiv(int64_t n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ q, int *__restrict__ inWindow)
{
   const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   const bool ok = sdiv_window(a[i]) & sdiv_window(b[i]);
   inWindow[i] = ok ? 1 : 0;
   q[i] = ok ? sdiv_by(a[i], b[i], sdiv_rcp(b[i])) : a[i] / b[i];
}

// known-answer test of the prologue's clamp chain (device_math.h; batotp_hip_clamp_kat, include/batotp_hip_clamp_kat.h): the forward chain
// with the floor +0 of every sweep, literally and through the one-instruction forms, and the condition under which the kernels take the latter
__global__ void k_kat_clamp(int64_t n, const double *__restrict__ raw, const double *__restrict__ interp, const double *__restrict__ cap,
                            const double *__restrict__ smin, const double *__restrict__ lim1, double *__restrict__ literal,
                            double *__restrict__ fast, int *__restrict__ valid)
{
   const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   const double floorV = 0.0;
   valid[i] = (clamp_consts_ok(floorV, smin[i], cap[i]) & clamp_raw_ok(raw[i], interp[i])) ? 1 : 0;
   literal[i] = dmin(clamp_chain_literal<true>(raw[i], interp[i], floorV, smin[i], cap[i]), lim1[i]);
   fast[i] = vmin_f64(clamp_chain_fast<true>(raw[i], interp[i], floorV, smin[i], cap[i]), lim1[i]);
}

// ---- CERTIFIED FAST-FORWARD of the bisection on the 8 lanes of a path (the certificate of k_sweep1, sweep1.hip.h: its derivation
// and error analysis are there) ---------------------------------------------------------------------------------------------
// Called for paths whose first check of the stage was violated, after the loop's first update (ba.cpp:1281-1285: nIter = 1,
// sdotH = the first candidate, sdotTry = the second one).  In x = sdot^2 every bound of the check is a line: joint q allows
// sddot in [-au_q - m_q x, au_q - m_q x] with au = amax_q / |theta'_q|, m = theta''_q / theta'_q, and [-sddotMax, sddotMax] is the
// line au = sddotMax, m = 0.  They stop intersecting at
//    x* = min over the pairs of lines (i, j) of (au_i + au_j) / |m_i - m_j|
// (of the two orientations of a pair -- i above, j below, or the other way round -- the one with a positive slope difference
// crosses), and a candidate c of the loop is violated iff c^2 > x* -- for certain when |c^2 - x*| exceeds the band 2^-40 R x*
// (R = E / Smin: the rounding errors of the check against the width of the interval at x = 0).  The loop of ba.cpp:1267-1321 is
// advanced with its own update statements through every iteration whose outcome is certain and that neither ends it nor can take
// a failure exit; it stops in front of the first candidate inside the band, or the one that would end the loop: that one gets
// the real check in the next pass.  Anything unusual (a standing joint's threshold inside the band, non-finite or extreme values)
// leaves the state as it is.
// Round 6: written for the instruction count -- theta' already has its refined reciprocal (rD: two Newton steps, 2 eps, the
// accuracy the analysis asks for), the partner lines arrive by DPP moves (quad permutations, the half-row mirror and their
// products reach every lane of the group) instead of LDS-crossbar shuffles, a pair costs one reciprocal whatever its orientation
// (|m_i - m_j|), lines that do not exist are the line u = 1e300, m = 0 (every quantity stays finite without a select per pair),
// and the standing joints' true quotient sits behind a guard.  All lanes of a group are active together (the caller's condition
// is a path-level value), and the permutations never leave the group.
constexpr int DPP_QUAD_XOR3 = 0x1B; // quad_perm [3,2,1,0]
__device__ __forceinline__ double s8_rcp2(double d)
{
   double r = __builtin_amdgcn_rcp(d);
   r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
   return __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
}
// max(|x|, floor): one instruction
__device__ __forceinline__ double s8_absmax(double x, double floorv)
{
   double r;
   asm("v_max_f64 %0, |%1|, %2" : "=v"(r) : "v"(x), "v"(floorv));
   return r;
}
__device__ __forceinline__ void s8_certify(bool jOn, double thD, double thD2, double rD, bool rOk, double amaxq, double thrV, double thrA,
                                           double sddotMax, double &lowFact, double &sdotH, double &sdotL, double &sdotTry,
                                           double &sdotGood, int &nGood, int &nIter)
{
   constexpr double BIG = 1e300, TINY = 1e-300;
   const double xTop = sdotH * sdotH;                 // the first candidate: no later one is larger
   const bool use = jOn && !(fabs(thD) < thrV);       // a moving joint (ba.cpp:1526-1531)
   const double aur = amaxq * fabs(rD), mr = thD2 * rD;
   const double er = aur + fabs(mr) * xTop;
   // a line with a coefficient that is not an ordinary number stops the fast-forward (eMax = inf fails `sane`); NaNs fail every test
   const bool lineOk = rOk & (aur < 1e100) & (fabs(mr) < 1e100) & (er < 1e100);
   const bool have = use & lineOk;
   const double au = have ? aur : BIG;
   const double mj = have ? mr : 0.0;
   const double ej = use ? (lineOk ? er : kInf) : 0.0;
   const double uMin = grp_min<8>(au);
   const double eMax = grp_max<8>(ej);
   const double sMin2 = dmin(uMin, sddotMax);         // half the width of the interval at x = 0
   const bool standing = jOn && !use && !(fabs(thD2) < thrA);
   double xForce = kInf;
   if (S8_RARE(standing)) xForce = grp_min<8>(standing ? amaxq / fabs(thD2) : kInf);   // the check's own quotient (ba.cpp:1519-1524)
   // this lane's line against [-sddotMax, sddotMax] ...
   double xs = (au + sddotMax) * s8_rcp2(s8_absmax(mj, TINY));
   // ... and against the line of every other lane of the group
#define S8_PAIR(AUI, MI) xs = vmin_f64(xs, (au + (AUI)) * s8_rcp2(s8_absmax(mj - (MI), TINY)))
   {
      const double a1 = dpp_mov<DPP_QUAD_XOR1>(au), m1 = dpp_mov<DPP_QUAD_XOR1>(mj);
      S8_PAIR(a1, m1);
      const double a2 = dpp_mov<DPP_QUAD_XOR2>(au), m2 = dpp_mov<DPP_QUAD_XOR2>(mj);
      S8_PAIR(a2, m2);
      const double a3 = dpp_mov<DPP_QUAD_XOR3>(au), m3 = dpp_mov<DPP_QUAD_XOR3>(mj);
      S8_PAIR(a3, m3);
      const double a7 = dpp_mov<DPP_ROW_HALF_MIRROR>(au), m7 = dpp_mov<DPP_ROW_HALF_MIRROR>(mj);   // lane ^ 7
      S8_PAIR(a7, m7);
      const double a6 = dpp_mov<DPP_QUAD_XOR1>(a7), m6 = dpp_mov<DPP_QUAD_XOR1>(m7);               // lane ^ 6
      S8_PAIR(a6, m6);
      const double a5 = dpp_mov<DPP_QUAD_XOR2>(a7), m5 = dpp_mov<DPP_QUAD_XOR2>(m7);               // lane ^ 5
      S8_PAIR(a5, m5);
      const double a4 = dpp_mov<DPP_QUAD_XOR3>(a7), m4 = dpp_mov<DPP_QUAD_XOR3>(m7);               // lane ^ 4
      S8_PAIR(a4, m4);
   }
#undef S8_PAIR
   xs = grp_min<8>(xs);
   const double xstar = dmin(xs, 4.0 * xTop);          // beyond 4 xTop: "never violated by the lines" just as well
   const double R = eMax * s8_rcp2(sMin2 > 0.0 ? sMin2 : 1.0);
   const double band = (R * 0x1p-40) * xstar;
   // a standing joint's threshold below the band around x* decides alone, and exactly; one above the band never matters; one
   // inside the band: no fast-forward
   const bool forceFirst = xForce < xstar - band;
   const double xThr = forceFirst ? xForce : xstar;
   const double bandThr = forceFirst ? -1.0 : band;
   const bool sane = (sddotMax == sddotMax) & (eMax == eMax) & (xstar == xstar) & (R == R) & (R < 0x1p30) & (sMin2 > 1e-100) & (eMax < 1e100) &
                     (xTop > 1e-100) & (xTop < 1e100) & (xstar > 1e-100) & (forceFirst | (xForce > xstar + band));
   if (sane)
   {
      // Both loops of the replay are wavefront-uniform loops ("while any lane goes on") with BRANCH-FREE bodies: a per-lane loop with a
      // break, or an exec-masked update inside a uniform loop, makes the compiler structurize the whole loop as divergent and spend
      // twice as many scalar instructions on mask bookkeeping as the loop has vector instructions (18 against 7 per iteration in the
      // first round-6 build).  A lane that has stopped keeps its state through selects; its tests are re-evaluated on that unchanged
      // state and give what they gave.  Invariant used below: sdotTry == .5 * (sdotH + sdotL) in every lane at every point (the check
      // block's update, ba.cpp:1320, leaves it so, and every update here ends with that statement), so the midpoint needs no select.
      // The exit tests of both loops combine the masks of their comparisons (S8_MASK above): mMore holds the lanes that go on and is what
      // `more` is over the active lanes.  (S8_ANY(more) read the lane mask back from the 0/1 register that `it += more ? 1 : 0` had made of
      // it: v_cndmask -> v_cmp_ne in front of the branch of a loop that is one dependent chain.)
      // Neither `more` nor its mask is carried from pass to pass: a lane that has stopped keeps its state, so the comparisons that stopped
      // it come out the same in every later pass (the invariant above) and `more & ...` is `...`.
      int it = nIter;
      bool inBand = false;
      // the search for a first feasible speed (ba.cpp:1281-1285): the bracket shrinks below every violated candidate
      for (;;)
      {
         const double c = sdotTry, d = c * c - xThr;   // c * c: sdotSQ of the check
         inBand = !((fabs(d) > bandThr) & (c > 1e-100));
         const bool more = (fabs(d) > bandThr) & (c > 1e-100) & (d > 0.0) & (it < 90);
         const s8_mask mMore = S8_MASK(fabs(d) > bandThr) & S8_MASK(c > 1e-100) & S8_MASK(d > 0.0) & S8_MASK(it < 90);
         if (mMore == 0) break;
         const double lf2 = lowFact * 2.0;
         const double lo = dmax(.999 * 0.0, (1.0 - lf2) * c);
         lowFact = more ? lf2 : lowFact;
         sdotH = more ? c : sdotH;
         sdotL = more ? lo : sdotL;
         sdotTry = .5 * (sdotH + sdotL);
         it += more ? 1 : 0;
      }
      // sdotTry is feasible for certain and the first such speed: ba.cpp:1294 compares it with sdotGood = 0 and goes on.  From
      // here the plain bisection (ba.cpp:1286-1303): sdotGood == sdotL throughout
      const bool bisect = !inBand & (it < 90);
      // (its mask: inBand as the first loop left it is the comparisons of its last pass; a lane outside `bisect` stays out of the second loop.
      //  The mask and the bool must never disagree: sdotTry * sdotTry - xThr here is the `d` of that last pass bit for bit -- the same two
      //  operations on the same operands, and the translation unit is compiled with -ffp-contract=off, so neither can become an FMA -- and
      //  the compiler emits the comparisons once for both, as it does inside the loops.)
      const s8_mask mBisect = S8_MASK(fabs(sdotTry * sdotTry - xThr) > bandThr) & S8_MASK(sdotTry > 1e-100) & S8_MASK(it < 90);
      sdotGood = bisect ? sdotTry : sdotGood;
      nGood = bisect ? 1 : nGood;
      sdotL = bisect ? sdotTry : sdotL;
      it += bisect ? 1 : 0;
      sdotTry = .5 * (sdotH + sdotL);
      // ba.cpp:1294 is false for certain when |c - sdotGood| > 1e-3 c (1 + 3e-14); otherwise this candidate is, or may be, the
      // last one and gets the real check and the real test
      const double convThr = 1e-3 * (1.0 + 3e-14);
      for (;;)
      {
         const double c = sdotTry, d = c * c - xThr;
         const bool viol = d > 0.0;
         const double gap = fabs(c - sdotL), thr = convThr * c;
         const bool goesOn = viol | (gap > thr);
         const bool more = bisect & (fabs(d) > bandThr) & goesOn & (it < 90);
         const s8_mask mMore = mBisect & S8_MASK(fabs(d) > bandThr) & (S8_MASK(d > 0.0) | S8_MASK(gap > thr)) & S8_MASK(it < 90);
         if (mMore == 0) break;
         sdotH = (more & viol) ? c : sdotH;
         sdotL = (more & !viol) ? c : sdotL;
         sdotTry = .5 * (sdotH + sdotL);
         it += more ? 1 : 0;
      }
      sdotGood = bisect ? sdotL : sdotGood;
      nIter = it;
   }
}

// G lanes per path (8: one joint per lane, 4: joints j and j + 4 in lane j), up to 64 / G paths per wavefront
template <int G, int FEAT, int DIR>
__global__ void __launch_bounds__(S8_BLOCK, G == 8 ? 2 : 1) k_sweep8(SweepArgs a)
{
   static_assert(FEAT == -1 || FEAT == 0, "velocity / acceleration-only problems");
   static_assert(G == 8 || G == 4, "lanes per path");
   constexpr int PER = 8 / G;
   __shared__ double lim[6][8];
   __shared__ double rk[7][6];                 // the tableau by stage number (sweep_tableau_lds)
   __shared__ double2 pts[S8_BLOCK / G][4];    // curve points of a path waiting for their 64-byte store
   __shared__ double2 vw[S8_BLOCK / G][8];     // (v_k, w_k) of stage k = 1..5 of every path; slot 0 and 7: writes that must not land
   sweep_tableau_lds(rk);
   stage_limits(a.dP, lim);

   const int lane = threadIdx.x & 63;
   const int wave = blockIdx.x * (S8_BLOCK / 64) + (threadIdx.x >> 6);
   const int j = lane % G;
   const int slot = lane / G;
   const int pslot = wave * a.ppw + slot;
   if (slot >= a.ppw || pslot >= a.B) return; // whole groups leave together; DPP never crosses groups
   const int p = a.order ? a.order[pslot] : pslot;   // ragged batches: paths of similar length share a wavefront (SweepArgs::order)
   const bool writer = (j == 0);
   const PathInfo pi = a.pinfo[p];
   const int n = (int)pi.n;
   const int64_t cap = a.cap;
   double2 *mypts = pts[threadIdx.x / G];
   double2 *myvw = vw[threadIdx.x / G];
   for (int k = j; k < 8; k += G) myvw[k] = make_double2(0.0, 0.0);

   // bootstrap (ba.cpp:1021-1041) through the general kernel's device functions; the loop below carries its own state
   Pt<G, FEAT, true> t;
   pt_init(t, a.P, pi, a.sC, a.coef, a.km, lim, j, DIR);

   double2 *out = (DIR == 1 ? a.fwd : a.rev) + (int64_t)p * cap; // may alias the reverse curve (curves in place)
   batotp_path_result *__restrict__ r = a.res + p;
   const double2 *mvc = nullptr; // the reverse curve the forward sweep follows
   int nMvc = 0;
   if (DIR == 1)
   {
      const int64_t nRev = r->n_rev;
      if (nRev < 2)
      {
         sweep_no_reverse_curve(r, writer);
         return;
      }
      mvc = a.rev + (int64_t)p * cap + (cap - nRev);
      nMvc = (int)nRev;
      t.mvc = reinterpret_cast<const double *>(mvc);
      t.nMvc = nMvc;
   }

   const double absh = pi.integ_res;
   const double h = DIR * absh;
   const double sres = pi.sres_c;
   const double sEnd = sres * (double)(n - 1);
   const double sLast = (DIR == 1) ? sEnd : 0.0;
   double s0v = (DIR == 1) ? 0.0 : sEnd;
   double v0, w0 = 0;
   pt_bootstrap(t, j, DIR, n, h, s0v, v0, w0);
   const double vBoot = v0;

   // ---- the loop's own state -------------------------------------------------------------------
   // lane constants: joints jj[q] = j + q G of this lane
   bool jOn[PER];
   int jAt[PER];
   double vmax[PER], amax[PER];
   // this lane's coefficients on the cursor's segment: c1, 2 c2, 3 c3, 6 c3 (the products the reference forms first:
   // (3*c3)*tau2, (2*c2)*tau, (6*c3)*tau, ba.cpp:1358-1360); theta', theta'' of the last evaluation point; the refined
   // reciprocal of theta' (sdiv_rcp) and whether theta' lies in the window in which it may be used
   double c1[PER], c2x2[PER], c3x3[PER], c3x6[PER], thD[PER], thD2[PER], rD[PER];
   double sa[PER]; // sgn(theta') * amax of ba.cpp:1526-1531 where theta' != 0: amax with the sign of theta' (1.0 * amax and -1.0 * amax are exact)
   bool rOk[PER];
#pragma unroll
   for (int q = 0; q < PER; ++q)
   {
      jOn[q] = (j + q * G) < t.nJ;
      jAt[q] = jOn[q] ? j + q * G : 0;
      vmax[q] = t.vmax[q]; amax[q] = t.amax[q];
      c1[q] = jOn[q] ? t.rowTh[q].c1 : 0.0; c2x2[q] = jOn[q] ? 2 * t.rowTh[q].c2 : 0.0;
      c3x3[q] = jOn[q] ? 3 * t.rowTh[q].c3 : 0.0; c3x6[q] = jOn[q] ? 6 * t.rowTh[q].c3 : 0.0;
      thD[q] = t.thD[q]; thD2[q] = t.thD2[q];
      rOk[q] = sdiv_window(thD[q]);
      rD[q] = sdiv_rcp(thD[q]);
      sa[q] = (thD[q] < 0.0) ? -amax[q] : amax[q];
   }
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
   // knot window (compact pairs, knot_window.h): the knot on the side the cursor moves to (reverse: knot rowSeg, forward: knot
   // rowSeg + 1) and the one beyond it, as (y, y'') each -- a segment change one step further forms its coefficients from registers;
   // every segment-change block of the wavefront issues the load of the knot beyond, which nothing reads before the next such block
   double kEdgeY[PER], kEdgeSol[PER], kPreY[PER], kPreSol[PER];
   int preIdx = KNOT_WINDOW_NONE; // knot index the prefetch pair holds (and the edge pair holds preIdx - DIR): none yet
#pragma unroll
   for (int q = 0; q < PER; ++q) { kEdgeY[q] = 0; kEdgeSol[q] = 0; kPreY[q] = 0; kPreSol[q] = 0; }
   double sSeg = sres * (double)seg, sNext = sres * (double)(seg + 1); // sites of the cursor's segment
   // reverse-curve cursor (forward sweep): segment, its two points and the window's two neighbours (mvc_window.h; indices clamped
   // to the curve)
   int segM = 0;
   double mS0 = 0, mD0 = 0, mS1 = 0, mD1 = 0, mSLo = 0, mDLo = 0, mSHi = 0, mDHi = 0;
   if (DIR == 1)
   {
      segM = t.segMVC;
      const double2 qa = mvc[segM], qb = mvc[segM + 1], ql = mvc[mvc_window_lo(segM)], qh = mvc[mvc_window_hi(segM, nMvc)];
      mS0 = qa.x; mD0 = qa.y; mS1 = qb.x; mD1 = qb.y;
      mSLo = ql.x; mDLo = ql.y; mSHi = qh.x; mDHi = qh.y;
   }
   unsigned status = t.status;
   int nfail = t.nfail;
   double sdotCur = t.sdotCur;
   double sddotL = t.sddotL, sddotH = t.sddotH;

   double v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0;
   double w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, w6 = 0;
   double sPrev = s0v, sdPrev = v0, sCurPt = s0v, sdCurPt = v0; // last two published points, for the end snap
   double sCur = s0v; // traj.sCur

   const int iMax = sweep_max_steps_int(a.P, pi);
   const int capI = (int)cap;
   // curves in place: slot i must have been left behind by the reverse-curve cursor (the reverse sweep follows no curve and only
   // tests the capacity in its loop)
   const int revStartI = sweep_rev_start_int(a, nMvc, DIR);
   const auto curveFull = [&](int at) { return DIR == 1 ? sweep_curve_full(at, capI, revStartI, segM) : at >= capI; };

   // point 0: straight to HBM, and into the group of four it belongs to
   {
      const int idx0 = (DIR == 1) ? 0 : capI - 1;
      if (writer) { out[idx0] = make_double2(s0v, v0); mypts[idx0 & 3] = make_double2(s0v, v0); }
   }
   int flushedTo = (DIR == 1) ? 0 : capI; // forward: points [0, flushedTo) are in HBM; reverse: points [flushedTo, cap)

   const double floorV = 0.0 / absh; // ba.cpp:1050-1051,1085
   int nPts = 0, i = 1;
   unsigned endStatus = 0;
   // A path starts as if the stage before its first one had just ended (st one lower, PH_ENDED): the stores of that stage
   // go to slots nothing reads, and the loop needs no separate state for the first stage.
   int st = (DIR == 1) ? -1 : 0;
   constexpr int PH_FIRST = 0, PH_ENDED = 1, PH_CHECK = 2, PH_DEAD = 3, PH_CERT = 4;
   // reverse sweep: a path whose first check was violated waits in PH_CERT for the certificate block at the top of the loop, which
   // runs once holdC/8 of the live paths have gathered there (or nothing else can run in this pass)
   constexpr bool CERT = DIR == -1 && PER == 1;
   const int holdC = a.holdc;
   int phase = PH_ENDED;
   if (curveFull(i)) { endStatus = BATOTP_ST_CAPACITY; phase = PH_DEAD; }
   double sN = 0, wN = 0;
   double lowFact = .01, sdotGood = 0, sdotL = 0, sdotH = 0, sdotTry = 0;
   int nGood = 0, nIter = 0;
   // A stage value that is not an ordinary number has been kept (sticky; see the tableau combination).  "Ordinary" ends at 1e290, well
   // inside the finite range: then every partial sum of the tableau combination is finite (six terms with weights below 12), and
   // v0 + h * sum is not a NaN for a finite h -- what the one-instruction clamps of the prologue need (device_math.h, clamp_chain_fast).
   // The per-path part of their condition (sdotMin > 0, no NaN among the constants) rides in the same flag.
   constexpr double S8_ORDINARY = 1e290;
   // (The flag stays a per-lane bool and `odd` the ballot of a bool: kept as a sticky lane mask it costs the reverse kernel two VGPRs,
   //  profiles/stage_chain_code_object.txt.)
   bool wild = !(fabs(v0) < S8_ORDINARY) | !(fabs(w0) < S8_ORDINARY) | !(fabs(h) < kInf) | !clamp_consts_ok(floorV, sdotMin, sdotCap);
   bool stageFailed = false; // the bisection of the stage that ended failed: sddotArr[st] keeps its previous value (ba.cpp:1091 ignores the code)
   const int hold = a.hold;
#ifdef S8_PROFILE
   // [0] passes of the loop, [1] prologue blocks, [2] paths they served, [3] check blocks, [4] paths inside them, [5] cycles in
   // prologue blocks, [6] cycles in check blocks, [7] cycles in the loop, [8] step-end blocks, [9] segment-change blocks,
   // [10] knot-cursor walks, [11] fast-forward blocks, [12] literal-form (rare) blocks of the check, [13] live paths summed over passes
   double pc[16];
   for (int k = 0; k < 16; ++k) pc[k] = 0;
   const unsigned long long tLoop0 = __builtin_readcyclecounter();
#endif

   for (;;)
   {
      const unsigned long long mAlive = __ballot(phase != PH_DEAD);
      if (mAlive == 0) break;
      const unsigned long long mWait = __ballot(phase < PH_CHECK);
      const bool startNow = (mWait == mAlive) || (__popcll(mWait) * 8 >= __popcll(mAlive) * hold);
      S8_CNT(0, 1); S8_CNT(13, __popcll(mAlive) / G);
      if (CERT)
      {
         const unsigned long long mCert = __ballot(phase == PH_CERT);
         if (mCert != 0)
         {
            // (will a prologue or a check run in this pass?  If not, the waiting certificates are all there is to do)
            const bool progress = (startNow && mWait != 0) || ((mAlive & ~mWait & ~mCert) != 0);
            if (__popcll(mCert) * 8 >= __popcll(mAlive) * holdC || !progress)
            {
               S8_TICK(tF0);
               S8_CNT(11, 1); S8_CNT(15, __popcll(mCert) / G);
               if (phase == PH_CERT)
               {
                  s8_certify(jOn[0], thD[0], thD2[0], rD[0], rOk[0], amax[0], thrV, thrA, sddotMax, lowFact, sdotH, sdotL, sdotTry, sdotGood,
                             nGood, nIter);
                  phase = PH_CHECK;
               }
               S8_TICK(tF1);
               S8_CYC(14, tF0, tF1);
            }
         }
      }
      S8_TICK(tA);
      if (startNow && mWait != 0)
      {
         S8_CNT(1, 1); S8_CNT(2, __popcll(mWait) / G);
         if (phase < PH_CHECK)
         {
            // ---- the stage that ended: keep its values --------------------------------------------
            {
               phase = PH_FIRST;
               const double vN = sdotCur;
               wild |= !(fabs(vN) < S8_ORDINARY) | !(fabs(wN) < S8_ORDINARY);
               // slot st keeps (vN, wN); a failed bisection leaves sddotArr[st] as it was (the w half goes to the spare slot 7);
               // stage 6 is kept in registers by the step end below (its writes go to the spare slot 7 as well)
               {
                  double *slotV = reinterpret_cast<double *>(myvw + ((unsigned)st < 6u ? st : 7));
                  double *slotW = reinterpret_cast<double *>(myvw + (((unsigned)st < 6u && !stageFailed) ? st : 7)) + 1;
                  *slotV = vN;
                  *slotW = wN;
               }
               const bool stepEnd = (st == 6);
               st = stepEnd ? st : st + 1;
               if (S8_ANY(stepEnd))
               {
                  S8_CNT(8, 1);
                  if (stepEnd)
                  {
                     // FSAL shift and publish, ba.cpp:1096-1100 (stage 6: position sN, values vN, wN or the stale sddotArr[6])
                     const double wE = stageFailed ? w6 : wN;
                     s0v = sN; v0 = vN; w0 = wE; w6 = wE;
                     sPrev = sCurPt; sdPrev = sdCurPt;
                     sCurPt = s0v; sdCurPt = v0;
                     const int idx = (DIR == 1) ? i : capI - 1 - i;
                     mypts[idx & 3] = make_double2(s0v, v0); // every lane of the group holds the same pair
                     st = (DIR == 1) ? 0 : 1;
                     const bool fin = sCur * DIR > sLast;      // ba.cpp:1109-1115
                     const bool late = !fin && (i > iMax);     // ba.cpp:1117-1122
                     nPts = fin ? i + 1 : nPts;
                     i = (fin || late) ? i : i + 1;
                     const bool full = !fin && !late && curveFull(i);
                     endStatus = late ? (unsigned)BATOTP_ST_MAX_INTEG_TIME : (full ? (unsigned)BATOTP_ST_CAPACITY : endStatus);
                     phase = (fin || late || full) ? PH_DEAD : phase;
                     // a complete group of four points: one 64-byte store (not for the step that ends the path: its last
                     // point is still to be snapped onto the path end)
                     const bool chunk = !fin && ((DIR == 1) ? ((idx & 3) == 3) : ((idx & 3) == 0));
                     if (S8_ANY(chunk))
                     {
                        if (chunk)
                        {
                           const int base = idx & ~3;
                           const int lo = (DIR == 1) ? base : idx, hi = (DIR == 1) ? idx : ((base + 3 < capI) ? base + 3 : capI - 1);
                           const int at = base + j;
                           if (j < 4 && at >= lo && at <= hi) out[at] = mypts[j];
                           flushedTo = (DIR == 1) ? idx + 1 : idx;
                        }
                     }
                  }
               }
            }
            if (phase != PH_DEAD)
            {
               if (DIR == 1)
               {
                  // forward predictor (ba.cpp:1055-1065): only the move of the reverse-curve cursor survives
                  const bool pred = (st == 0);
                  if (S8_ANY(pred))
                  {
                     if (pred)
                     {
                        sCur = s0v + h * v0;
#include "sweep8_mvcwalk.inc"
                        st = 1;
                     }
                  }
               }
               // ---- tableau combination, ba.cpp:1073-1085 ---------------------------------------------
               const double *bc = rk[st];
               double sdotT = 0, sddotT = 0;
               {
                  const double2 q1 = myvw[1], q2 = myvw[2], q3 = myvw[3], q4 = myvw[4], q5 = myvw[5];
                  v1 = q1.x; w1 = q1.y; v2 = q2.x; w2 = q2.y; v3 = q3.x; w3 = q3.y; v4 = q4.x; w4 = q4.y; v5 = q5.x; w5 = q5.y;
               }
               // Stage st adds the terms k < st only.  The weights of the others are +0 in the table, and adding their products
               // changes nothing as long as every stage value is finite (x + (+-0) = x: a partial sum starts as 0 + b0 v0 and
               // is therefore never -0); a path that ever kept a non-finite stage value (0 * inf = NaN) takes the literal form.
               // Two rare situations share ONE wavefront-uniform guard (a ballot costs three vector instructions and a branch that
               // waits for it): a non-finite stage value (below), and a velocity-limit quotient outside the window of the shared
               // reciprocal (further down: `odd` is then a scalar condition)
               bool slowDiv = false;
#pragma unroll
               for (int q = 0; q < PER; ++q) slowDiv |= jOn[q] && fabs(thD[q]) > thrV && !(rOk[q] & sdiv_window(vmax[q]));
               const bool odd = S8_RARE(wild | slowDiv);
               if (!odd)
               {
                  sdotT += bc[0] * v0; sddotT += bc[0] * w0;
                  sdotT += bc[1] * v1; sddotT += bc[1] * w1;
                  sdotT += bc[2] * v2; sddotT += bc[2] * w2;
                  sdotT += bc[3] * v3; sddotT += bc[3] * w3;
                  sdotT += bc[4] * v4; sddotT += bc[4] * w4;
                  sdotT += bc[5] * v5; sddotT += bc[5] * w5;
               }
               else
               {
                  sdotT += bc[0] * v0; sddotT += bc[0] * w0;
                  { const double a1 = sdotT + bc[1] * v1, b1 = sddotT + bc[1] * w1; sdotT = (st > 1) ? a1 : sdotT; sddotT = (st > 1) ? b1 : sddotT; }
                  { const double a2 = sdotT + bc[2] * v2, b2 = sddotT + bc[2] * w2; sdotT = (st > 2) ? a2 : sdotT; sddotT = (st > 2) ? b2 : sddotT; }
                  { const double a3 = sdotT + bc[3] * v3, b3 = sddotT + bc[3] * w3; sdotT = (st > 3) ? a3 : sdotT; sddotT = (st > 3) ? b3 : sddotT; }
                  { const double a4 = sdotT + bc[4] * v4, b4 = sddotT + bc[4] * w4; sdotT = (st > 4) ? a4 : sdotT; sddotT = (st > 4) ? b4 : sddotT; }
                  { const double a5 = sdotT + bc[5] * v5, b5 = sddotT + bc[5] * w5; sdotT = (st > 5) ? a5 : sdotT; sddotT = (st > 5) ? b5 : sddotT; }
               }
               sN = s0v + h * sdotT;
               const double vRaw = v0 + h * sddotT;
               sCur = sN;

               // ---- the floor of ba.cpp:1085 and sdotLim, ba.cpp:1204-1236 (theta' of the PREVIOUS evaluation point) -----------------
               // The clamps with sdotCap, sdotMin, the floor and lim1 take their one-instruction forms (device_math.h, clamp_chain_fast) unless
               // `odd`: vRaw is not a NaN when every stage value is below 1e290 (`wild` is false), and the path's constants are part of
               // `wild`.  The two clamps of the forward sweep that involve the reverse curve's speed stay compare-and-select: whether that
               // speed is a NaN is only known after the walk below, behind `odd`'s ballot, and a guard of its own costs more than they do
               // (k_sweep8_lock, whose guard comes after the walk, converts them too).
               double vN = vmax_f64(vRaw, floorV);
               double sdotRev = 0;
               if (DIR == 1)
               {
                  // evalsdot, ba.cpp:1590-1607
#include "sweep8_mvcwalk.inc"
                  const double tauM = (sCur - mS0) / (mS1 - mS0);
                  sdotRev = mD0 + tauM * (mD1 - mD0);
                  const double sdotMVC = dmax(sdotRev, sdotMin);
                  vN = (vN > sdotMVC) ? sdotMVC : vN;
               }
               vN = vmin_f64(vN, sdotCap);
               vN = vmax_f64(vN, sdotMin);
               double lim1 = kInf;
               {
#pragma unroll
                  for (int q = 0; q < PER; ++q)
                  {
                     const bool on = jOn[q] && fabs(thD[q]) > thrV;
                     const bool fast = rOk[q] & sdiv_window(vmax[q]);
                     const double qv = fabs(sdiv_by(vmax[q], thD[q], rD[q]));
                     lim1 = (on & fast) ? dmin(lim1, qv) : lim1;
                  }
                  if (odd)
                  {
                     // the chain as the reference writes it, for every lane of the block
                     vN = clamp_chain_literal<DIR == 1>(vRaw, sdotRev, floorV, sdotMin, sdotCap);
#pragma unroll
                     for (int q = 0; q < PER; ++q)
                     {
                        const bool on = jOn[q] && fabs(thD[q]) > thrV;
                        const bool fast = rOk[q] & sdiv_window(vmax[q]);
                        if (on && !fast) lim1 = dmin(lim1, fabs(vmax[q] / thD[q]));
                     }
                     lim1 = grp_min<G>(lim1);
                     vN = dmin(vN, lim1);
                  }
                  else
                  {
                     lim1 = grp_min<G>(lim1);
                     vN = vmin_f64(vN, lim1);
                  }
               }
               sdotCur = vN;
               // applyAccelConstraintsBisectionPt, ba.cpp:1250-1265
               lowFact = .01; sdotGood = 0; nGood = 0; sdotL = 0; sdotH = vN; sdotTry = vN; nIter = 0; stageFailed = false;

               // ---- evalSplinePartials, ba.cpp:1341-1413: updateCurSeg (ba.cpp:1617-1652) on the sites sres*k ----
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
               double tau = (sCur - sSeg) / (sNext - sSeg);
               const bool chg = (seg != rowSeg);
               if (S8_ANY(chg))
               {
                  S8_CNT(9, 1);
                  if (chg)
                  {
#pragma unroll
                     for (int q = 0; q < PER; ++q)
                     {
                        if (FEAT < 0)
                        {
                           const unsigned at = (unsigned)(seg * nIn + jAt[q]);
                           // one segment further in the direction of the sweep: both knots (seg and seg + 1 of this joint) are in registers
                           // (as four scalars: selecting between double2 values sends them through scratch)
                           double yL = (DIR == 1) ? kEdgeY[q] : kPreY[q], solL = (DIR == 1) ? kEdgeSol[q] : kPreSol[q];
                           double yR = (DIR == 1) ? kPreY[q] : kEdgeY[q], solR = (DIR == 1) ? kPreSol[q] : kEdgeSol[q];
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
                           knot_window_shift(true, DIR, yL, solL, yR, solR, kEdgeY[q], kEdgeSol[q]);
                           const double c2 = solL / 2.0;
                           c1[q] = yR - yL - sixthB;
                           c2x2[q] = 2 * c2; c3x3[q] = 3 * c3; c3x6[q] = 6 * c3;
                        }
                        else
                        {
                           const Coef4 k = *reinterpret_cast<const Coef4 *>(coef + (unsigned)(seg * rowStride) + jAt[q] * 4);
                           c1[q] = k.c1; c2x2[q] = 2 * k.c2; c3x3[q] = 3 * k.c3; c3x6[q] = 6 * k.c3;
                        }
                     }
                     if (FEAT < 0) preIdx = knot_window_mark(seg, lastSeg, DIR);
                     rowSeg = seg;
                  }
                  if (FEAT < 0)
                  {
                     // the window's load (knot_window.h): every lane of the block, changed or not, straight into the prefetch registers;
                     // the next segment-change block of the wavefront is the first to read them
                     const int at = knot_window_load(seg, lastSeg, DIR) * nIn;
#pragma unroll
                     for (int q = 0; q < PER; ++q)
                     {
                        const double2 kq = km[(unsigned)(at + jAt[q])];
                        kPreY[q] = kq.x; kPreSol[q] = kq.y;
                     }
                  }
               }
               {
                  const double tau2 = tau * tau;
#pragma unroll
                  for (int q = 0; q < PER; ++q)
                  {
                     thD[q] = (c3x3[q] * tau2 + c2x2[q] * tau + c1[q]) * vfact;
                     thD2[q] = (c3x6[q] * tau + c2x2[q]) * afact;
                     rOk[q] = sdiv_window(thD[q]);
                     rD[q] = sdiv_rcp(thD[q]);
                     sa[q] = (thD[q] < 0.0) ? -amax[q] : amax[q];
                  }
               }
               phase = PH_CHECK;
            }
         }
      }
      S8_TICK(tB);
      S8_CYC(5, tA, tB);
#ifdef S8_PROFILE
      {
         const unsigned long long mChk = __ballot(phase == PH_CHECK);
         S8_CNT(3, mChk != 0 ? 1 : 0); S8_CNT(4, __popcll(mChk) / G);
      }
#endif
      if (phase == PH_CHECK)
      {
         // (what the bisection update below needs and the constraint check does not produce is computed first: it fills the
         //  wait of the check's wavefront-uniform guard for its ballot)
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
            bool rare = false; // a joint that stands still, or a quotient outside the window of the shared reciprocal
#pragma unroll
            for (int q = 0; q < PER; ++q)
            {
               const bool slow = fabs(thD[q]) < thrV;
               const double vTerm = thD2[q] * sdotSQ;
               const double nH = sa[q] - vTerm, nL = -sa[q] - vTerm; // (theta' = 0 lies outside the window: the literal form below)
               const bool fast = capOk & rOk[q] & sdiv_window(nH) & sdiv_window(nL);
               const double qH = sdiv_by(nH, thD[q], rD[q]);
               const double qL = sdiv_by(nL, thD[q], rD[q]);
               const bool use = jOn[q] & !slow & fast;
               // inside the window both quotients are finite and the bound is not a NaN (capOk): the one-instruction min / max
               // returns what the compare-and-select form returns (device_math.h: up to the sign of a zero that nothing reads)
               const double Hm = vmin_f64(H, qH), Lm = vmax_f64(L, qL);
               H = use ? Hm : H;
               L = use ? Lm : L;
               rare |= jOn[q] & (slow | !fast);
            }
            if (S8_RARE(rare))
            {
               S8_CNT(12, 1);
#pragma unroll
               for (int q = 0; q < PER; ++q)
               {
                  const bool slow = fabs(thD[q]) < thrV;
                  const int svpt = sgn(thD[q]);
                  const double vTerm = thD2[q] * sdotSQ;
                  const double nH = svpt * amax[q] - vTerm, nL = -svpt * amax[q] - vTerm;
                  const bool fast = capOk & rOk[q] & sdiv_window(sa[q] - vTerm) & sdiv_window(-sa[q] - vTerm);
                  if (jOn[q] && !slow && !fast)
                  {
                     H = dmin(H, nH / thD[q]);
                     L = dmax(L, nL / thD[q]);
                  }
                  // a joint that stands still (ba.cpp:1519-1524)
                  if (jOn[q] && slow && !(fabs(thD2[q]) < thrA)) force |= sdotSQ > amax[q] / fabs(thD2[q]);
               }
            }
         }
         double Hred = force ? -kInf : H;
         // (Reducing only the side the stage keeps and reading the other side's verdict off the ballot of "my bound is crossed"
         //  saves six instructions and measured 4 % SLOWER -- 716 against 690 ms: the ballot's way through the scalar registers
         //  sits on the critical path of the pass.)
         grp_min_max<G>(Hred, L);
         sddotH = Hred; sddotL = L;
         const bool isViol = L > Hred;

         // (The same pass as four exec-masked blocks by situation -- first check passed / violated without a feasible point / violated with
         //  one / feasible after a violation -- measured 5 % SLOWER than this one block of selects: the guards of four blocks cost more than
         //  the selects they save, profiles/r04_b_*; that variant is not kept in the source.)
         // ---- one pass of the loop of ba.cpp:1267-1321, as selects -----------------------------------------
         const bool first = (nIter == 0);
         const bool fin0 = !isViol && first; // the first check passes: the stage is done, nothing else happens
         bool fin = fin0, failed = false, toCert = false;
         // forward sweep: 99 % of the checks end here and the block is skipped; reverse sweep: three quarters of the time a
         // path is inside a bisection, the guard would nearly always be taken and only cost its ballot
         if (DIR == -1 || S8_ANY(!fin0))
         {
            const bool good = !isViol && !first;      // a feasible point after at least one violated one
            const bool shrink = isViol && nGood == 0; // ba.cpp:1281-1285: no feasible point known yet
            // the two threshold tests of the loop (computed above), behind ONE guard for the quotients they may need:
            //   ba.cpp:1294-1303: two successive feasible points closer than 1e-3 (relative)   -- matters for `good` paths
            //   ba.cpp:1313: the bracket [sdotL, sdotH] has collapsed                          -- matters while no feasible point is
            //   known, i.e. for `shrink` paths, whose bracket after this pass is [sdotLShrunk, sdotTry] whatever the other test says
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
            // (the next candidate computed for both verdicts ahead of the reduction, then one select: 1.5 % SLOWER, 691 against 681 ms)
            sdotTry = (fin || failed) ? sdotTry : .5 * (sdotH + sdotL);
            status |= failed ? (unsigned)BATOTP_ST_BISECT_FAIL : 0u;
            nfail += failed ? 1 : 0;
            stageFailed = failed;
            // ---- CERTIFIED FAST-FORWARD of the bisection (s8_certify above) -------------------------------------------------------
            // The first check of the stage was violated and the loop goes on.  Forward sweep: the 8 paths of a wavefront run in
            // lockstep and 0.6 % of the stages bisect -- a dozen passes in which seven paths wait for one: the certificate runs
            // right here.  Reverse sweep: 22 % of the stages bisect and the passes are shared by several paths; run per arriving
            // path the block costs more than the passes it removes (profiles/r03_g_*, r04_j_*: +27 %), so there the path moves to
            // the phase PH_CERT and the block at the top of the loop serves the paths that have gathered in it (round 6).
            if (PER == 1 && accOn)
            {
               const bool ffWant = (((DIR == 1) ? (a.ff & 1) : (a.ff & 2)) != 0) && first && isViol && !failed;
               if (CERT) toCert = ffWant;
               else if (S8_ANY(ffWant))
               {
                  S8_CNT(11, 1);
                  if (ffWant)
                     s8_certify(jOn[0], thD[0], thD2[0], rD[0], rOk[0], amax[0], thrV, thrA, sddotMax, lowFact, sdotH, sdotL, sdotTry, sdotGood,
                                nGood, nIter);
               }
            }
         }
         wN = fin ? ((DIR == 1) ? sddotH : sddotL) : wN;
         phase = (fin || failed) ? PH_ENDED : (toCert ? PH_CERT : phase);
      }
      S8_TICK(tC);
      S8_CYC(6, tB, tC);
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

   sweep_end_snap(DIR, sLast, sPrev, sdPrev, sCurPt, sdCurPt, DIR == 1 ? mvc[nMvc - 1].y : 0.0);
   int64_t nOut = nPts;

   if (nPts >= 4)
   {
      // the snapped point joins the points still waiting in LDS; what has not reached HBM yet goes now
      const int idxLast = (DIR == 1) ? nPts - 1 : capI - nPts;
      mypts[idxLast & 3] = make_double2(sCurPt, sdCurPt);
      const int base = idxLast & ~3;
      const int at = base + j;
      const int lo = (DIR == 1) ? (flushedTo > base ? flushedTo : base) : idxLast;
      const int hi = (DIR == 1) ? idxLast : ((flushedTo - 1 < base + 3) ? flushedTo - 1 : base + 3);
      if (j < 4 && at >= lo && at <= hi) out[at] = mypts[j];
   }
   else
   {
      // The points of so short a curve are all still here: point 0 = the start, point nPts-2 = (sPrev, sdPrev), point nPts-1 = the
      // snapped end.
      status |= BATOTP_ST_SHORT; nOut = 4;
      if (writer)
      {
         const double2 snapped = make_double2(sCurPt, sdCurPt);
         const double2 pt[3] = {make_double2(DIR == 1 ? 0.0 : sEnd, vBoot), nPts == 2 ? snapped : make_double2(sPrev, sdPrev), snapped};
         sweep_short_to_four(DIR, nPts, absh, pt, out, cap);
      }
   }
   sweep_end_result(r, writer, DIR, nOut, nPts, absh, status, nfail);
}

} // namespace bk
