// output_plan.h -- the host-side plan of the output stage (batotp_hip_output, output_api.inc) as plain C++: which stages every path
// of a range passes, how many points each stage gives it, where the range is cut into chunks and where the paths of a launch
// sequence lie in its buffers.  All of it follows from the result rows of the forward sweep and the parameters of the call, so
// nothing here touches the device: hipcc compiles this header into the library and a plain g++ -std=c++11 compiles it into
// tests/drivers/output_plan_main.cpp, which compares the plan with the CPU checker (tests/test_output_plan.py).
// cutRanges and pathBlocks -- the cut of a batch into ranges that fit a budget and the (path, block) grid of a range -- also serve the
// outputs made from an output (range_run.inc), the audit and the resampler; tests/drivers/range_plan_main.cpp drives them alone.
// The arithmetic is fp64 and (int) truncation of the reference's formulas (ba.cpp:1668-1683, 1841, 1876), in their order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "batotp_hip.h"

namespace bk
{

// read by the kernels of output.hip.h: layout and field order are part of the device code
struct OutPath
{
   int64_t off1;    // first point of this path in the stage-1 arrays (sOut, seg, th1)
   int64_t off2;    // ... in the down-sampled arrays (th2, sol2)
   int64_t offF;    // ... in the final-stage arrays of the launch (dense over the paths of the launch)
   int64_t offD;    // ... in the result of the chunk, which stays in path order (= offF unless the chunk is staged)
   int64_t offS;    // first element of this path's s(t) second derivatives
   int32_t p;       // path of the batch
   int32_t nFwd;    // points of the forward curve
   int32_t n1;      // nOut of ba.cpp:1683
   int32_t n2;      // points after smoothing + down-sampling (= n1 without smoothing)
   int32_t nF;      // final points
   int32_t window;  // (int)smoothing factor of this path when it is smoothed, else 0
   double tStep;    // time step of the forward curve (tMVC[i] = tStep*i)
   double vfactT, afactT; // 1/tfact and its square, tfact = (output resolution)/(smoothing factor) of this path (ba.cpp:1754)
};

// ba.cpp:1668-1675: never sample finer than the integration step; smooth + re-interpolate afterwards.  All of it follows from
// the step, so it is a property of the path; `route` (re-interpolated or not, smoothed or not) decides which stages a path
// passes and which buffers they need.  A NaN step compares false: such a path has no forward curve and takes no route at all.
struct OutStep { double h, outRes, smoothFact; bool reinterp, smoothing; int route; };

inline OutStep outStepOf(double h, double outResUser, double smoothFactUser)
{
   OutStep s{h, outResUser, smoothFactUser, false, false, 0};
   if (s.outRes < h)
   {
      s.reinterp = true;
      s.outRes = h;
      s.smoothFact *= std::max(outResUser / s.outRes, 1.);
   }
   s.smoothing = s.smoothFact > 1.5;
   s.route = (s.reinterp ? 2 : 0) | (s.smoothing ? 1 : 0);
   return s;
}

struct OutPlan
{
   std::vector<OutPath> all;    // sizes of every path; offF = its first point in the result of the call, the other offsets 0
   std::vector<OutStep> step;
   std::vector<int64_t> n, off; // final points per path, first point of the path in the result (a failed path keeps its place)
   std::vector<double> sres;
   int64_t totF = 0;
   bool mixedCall = false;      // more than one route in the range: the chunks that mix them stage their results
   std::vector<int> cuts;       // chunk c holds the paths [cuts[c], cuts[c + 1]) of the range
   size_t maxChunk = 0;         // scratch bytes of the largest chunk
};

// res: result rows of the K paths of the range (path0 = the first one's place in the batch), h: the integration step of each
inline void planOutput(const batotp_path_result *res, const double *h, int K, int32_t path0, double outResUser, double smoothFactUser, OutPlan &pl)
{
   pl.all.resize(K); pl.step.resize(K);
   pl.n.assign(K, 0); pl.off.assign(K, 0); pl.sres.assign(K, 0.0);
   int64_t totF = 0;
   unsigned routesLive = 0; // routes taken by the paths of the range that have a trajectory
   for (int k = 0; k < K; ++k)
   {
      OutPath &q = pl.all[k];
      const OutStep &S = pl.step[k] = outStepOf(h[k], outResUser, smoothFactUser);
      const double outRes = S.outRes, smoothFact = S.smoothFact;
      const bool reinterp = S.reinterp, smoothing = S.smoothing;
      memset(&q, 0, sizeof(q));
      const batotp_path_result &r = res[k];
      const uint32_t stt = r.status_rev | r.status_fwd;
      q.p = path0 + k;
      q.offF = totF;
      pl.off[k] = totF;
      if (r.n_fwd < 4 || !(S.h > 0) || (stt & (BATOTP_ST_MAX_INTEG_TIME | BATOTP_ST_CAPACITY | BATOTP_ST_NONFINITE))) continue;
      q.nFwd = (int32_t)r.n_fwd;
      q.tStep = (r.status_fwd & BATOTP_ST_SHORT) ? r.t_total / 3. : S.h;
      const double tLast = q.tStep * (double)(q.nFwd - 1);
      int nOut = (int)(smoothFact * std::ceil(tLast / outRes + 1.)); // ba.cpp:1683
      nOut = std::max(nOut, 4);
      q.n1 = nOut;
      q.n2 = smoothing ? std::max((int)((nOut - 1) / smoothFact) + 1, 4) : nOut; // ba.cpp:1841
      q.nF = reinterp ? std::max((int)(std::ceil(tLast / outResUser)), 4) : q.n2;  // ba.cpp:1876
      pl.n[k] = q.nF;
      pl.sres[k] = reinterp ? outResUser : outRes;
      q.window = smoothing ? (int)smoothFact : 0;
      const double tfact = outRes / smoothFact; // traj.sres/_outSmoothFact, ba.cpp:1754
      q.vfactT = 1.0 / tfact;
      q.afactT = q.vfactT * q.vfactT;
      routesLive |= 1u << S.route;
      totF += q.nF;
   }
   pl.totF = totF;
   pl.mixedCall = (routesLive & (routesLive - 1)) != 0;
}

// What the scratch estimate reads besides the path: R, the rows per point the stage works with; torqueStep: the cable robot's or
// a serial robot's torque recomputation follows the evaluation; pose: the Cartesian rows are a pose that is converted at the end.
struct OutRows { int R; bool torqueStep, pose; };

// scratch of one path: s(t) second derivatives | sOut, segment | th1 (unless final) | th2 (if a middle stage) | sol2
inline size_t outScratchOf(const OutPath &q, const OutStep &S, const OutRows &m, bool mixedCall)
{
   const bool smoothing = S.smoothing, reinterp = S.reinterp;
   const int R = m.R;
   size_t by = 8 * (size_t)q.nFwd + 12 * (size_t)q.n1 + 8 * 256 + sizeof(OutPath) + 2 * sizeof(int64_t) * (1 + R) + 2 * sizeof(int) * (1 + R);
   if (smoothing || reinterp) by += 8 * (size_t)R * q.n1;
   if (smoothing && reinterp) by += 8 * (size_t)R * q.n2;
   if (reinterp) by += 8 * (size_t)R * q.n2;
   if (m.torqueStep) by += 2 * 8 * (size_t)R * q.n1;     // samples before the torque step and their second derivatives
   if (m.pose) by += 8 * (size_t)(R + 3) * q.nF + 1024;  // final rows before the pose conversion, (norm, q0) pairs, atan2 table
   else if (mixedCall) by += 8 * (size_t)R * q.nF;       // staged final rows of a chunk that mixes routes
   return by;
}

// Ranges of consecutive items 0 .. K-1 whose scratch, need(k) bytes each, fits `budget` bytes, at least one item each: range c holds
// the items [cuts[c], cuts[c + 1]).  Returns the bytes of the largest range.
template <class Need> inline size_t cutRanges(int K, Need need, double budget, std::vector<int> &cuts)
{
   cuts.assign(1, 0);
   size_t bytes = 0, maxRange = 0;
   for (int k = 0; k < K; ++k)
   {
      const size_t by = need(k);
      if (k > cuts.back() && (double)(bytes + by) > budget) { cuts.push_back(k); bytes = 0; }
      bytes += by;
      maxRange = std::max(maxRange, bytes);
   }
   cuts.push_back(K);
   return maxRange;
}

// The chunks of the range.  (Apart from planOutput because the budget follows from the memory that is free once the result of
// the call is allocated, and the size of the result is itself part of the plan.)
inline void cutChunks(OutPlan &pl, const OutRows &m, double budget)
{
   pl.maxChunk = cutRanges((int)pl.all.size(), [&](int k) { return outScratchOf(pl.all[k], pl.step[k], m, pl.mixedCall); }, budget, pl.cuts);
}

// One workgroup of the audit, torque, stretch and scale kernels: block blk of path `path` of its range (read by those kernels).
struct PathBlock
{
   int32_t path, blk;
};

inline int64_t blocksOf(int64_t n, int bp) { return (n + bp - 1) / bp; }

// The grid of such a kernel over the paths [ka, kb) with n[k] points each, bp points a block: the blocks in path order and
// first[k - ka], the place of the path's first block.  false where a path or the range has more than 2^31 - 1 blocks.
inline bool pathBlocks(const int64_t *n, int ka, int kb, int bp, std::vector<PathBlock> &blocks, std::vector<int64_t> &first)
{
   blocks.clear();
   first.assign((size_t)(kb - ka), 0);
   int64_t total = 0;
   for (int k = ka; k < kb; ++k)
   {
      first[k - ka] = total;
      const int64_t nb = blocksOf(n[k], bp);
      if (nb > 0x7fffffff || (total += nb) > 0x7fffffff) return false;
   }
   blocks.reserve((size_t)total);
   for (int k = ka; k < kb; ++k)
      for (int64_t b = 0, nb = blocksOf(n[k], bp); b < nb; ++b) blocks.push_back(PathBlock{k - ka, (int32_t)b});
   return true;
}

// The paths of a chunk run route by route through one launch sequence each: at most four, whatever the number of paths and
// however their routes alternate.  Within a sequence every offset is dense over its own paths (out_find_path searches them);
// offD is the path's place in the result of the chunk, which stays in path order.  Where a chunk holds one route only (always,
// with a positive integ_res) the two coincide and the last stage writes the result itself, as it always did; a chunk that mixes
// routes (`staged`) stages the final rows of each sequence and k_out_place moves them.
struct RouteLayout
{
   std::vector<OutPath> pc;                // the paths [ka, kb) that take the route, failed ones included (they have no points)
   int64_t t1 = 0, t2 = 0, tS = 0, tF = 0; // points of the stage-1, down-sampled, s(t) and final arrays; t1 == 0: nothing to launch
   bool staged = false;
};

inline RouteLayout routeLayout(const OutPlan &pl, int ka, int kb, int route)
{
   RouteLayout L;
   unsigned routesChunk = 0;
   for (int k = ka; k < kb; ++k) if (pl.all[k].nFwd) routesChunk |= 1u << pl.step[k].route;
   L.staged = (routesChunk & (routesChunk - 1)) != 0;
   const int64_t baseF = pl.all[ka].offF;
   for (int k = ka; k < kb; ++k) if (pl.step[k].route == route) L.pc.push_back(pl.all[k]);
   for (OutPath &q : L.pc)
   {
      q.off1 = L.t1; q.off2 = L.t2; q.offS = L.tS; q.offD = q.offF - baseF; q.offF = L.tF;
      L.t1 += q.n1; L.t2 += q.n2; L.tS += q.nFwd; L.tF += q.nF;
   }
   if (!(route & 1)) for (OutPath &q : L.pc) q.off2 = q.off1; // no smoothing: the down-sampled arrays are the stage-1 arrays
   return L;
}

} // namespace bk
