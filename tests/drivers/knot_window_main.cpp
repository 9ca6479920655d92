// knot_window_main.cpp -- the knot window of the batch sweep kernels without a GPU (tests/test_knot_window.py).
// Replays the segment-change block of k_sweep8 / k_sweep8_lock as batotp_amd/csrc/knot_window.h drives it: eight cursors ("lanes", each on
// a path of its own, ragged knot counts from the smallest the library accepts) walk over their segments, forward (dir +1) and reverse
// (dir -1), and after every query the wavefront runs ONE block if any lane's segment differs from the segment of its coefficients:
//   * a lane that changed asks the window for a hit; on a hit its two knots are the window's (edge, prefetch), otherwise it takes the
//     literal route (reads both knots from the array);
//   * the shift (the edge takes the far knot, the mark follows);
//   * EVERY lane, changed or not, loads knot_window_load(seg, ..) into its prefetch pair.
// The loads go through a fake loader: the pair is handed out at once (mode 0), or only at the head of the wavefront's next block
// (mode 1: where the kernel's wait stands) and holds a poison value until then.  Checked against a plain array lookup:
//   * a hit is reported exactly when the lane has changed before and moves one segment in the direction of the sweep -- never otherwise,
//     and then the window holds exactly knots seg and seg + 1 of the path, bit for bit (never a poison value);
//   * no load asks for a knot outside [0, n - 1];
//   * a usable mark names the index the prefetch pair was loaded from, and the edge pair is the knot beside it;
//   * a lane that did not change reloads the index it holds.
// Prints "ok queries=.. blocks=.. changes=.. hits=.. misses=.. far=.. against=.. first=.. reloads=.. clampedLoads=.."; exit status 1 at the
// first difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "knot_window.h"

namespace
{

struct Knot { double y, sol; };
typedef std::vector<Knot> Path;

uint64_t rngState = 0x2545f4914f6cdd1dull;
uint64_t rnd()
{
   rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17;
   return rngState;
}
double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

Path makePath(int n)
{
   Path p((size_t)n);
   for (int k = 0; k < n; ++k) { p[(size_t)k].y = uni() * 4.0 - 2.0; p[(size_t)k].sol = uni() * 20.0 - 10.0; }
   return p;
}

const double POISON = -7.25e300;

struct Lane
{
   const Path *p;
   int lastSeg;            // n - 2
   int seg, rowSeg;        // the cursor's segment, and the segment the lane's coefficients belong to
   double edgeY, edgeSol, preY, preSol;
   int mark;
   bool changedBefore;
   int asked;              // index of the last load into the prefetch pair, -1: none yet
   bool pending;
   // the segment's two knots as the last change formed its coefficients from them
   Knot usedL, usedR;
   void deliver()
   {
      if (pending) { preY = (*p)[(size_t)asked].y; preSol = (*p)[(size_t)asked].sol; pending = false; }
   }
   void init(const Path &path, int dir)
   {
      p = &path; lastSeg = (int)path.size() - 2;
      seg = rowSeg = dir == 1 ? 0 : lastSeg;
      edgeY = edgeSol = preY = preSol = 0;
      mark = bk::KNOT_WINDOW_NONE; changedBefore = false; asked = -1; pending = false;
      usedL = path[(size_t)seg]; usedR = path[(size_t)seg + 1];
   }
};

bool sameKnot(const Knot &a, double y, double sol) { return !std::memcmp(&a.y, &y, 8) && !std::memcmp(&a.sol, &sol, 8); }

const int W = 8;
long long nQueries = 0, nBlocks = 0, nChanges = 0, nHits = 0, nMisses = 0, nFar = 0, nAgainst = 0, nFirst = 0, nReloads = 0, nClamped = 0;

// the block; nullptr if all is well, else what went wrong
const char *block(Lane *ln, int dir, bool late)
{
   bool any = false;
   for (int k = 0; k < W; ++k) any |= ln[k].seg != ln[k].rowSeg;
   if (!any) return nullptr;
   ++nBlocks;
   // the head of the block: the kernel's wait for the loads of the previous block
   if (late)
      for (int k = 0; k < W; ++k) ln[k].deliver();
   for (int k = 0; k < W; ++k)
   {
      Lane &l = ln[k];
      const Path &path = *l.p;
      const bool chg = l.seg != l.rowSeg;
      double yL = dir == 1 ? l.edgeY : l.preY, solL = dir == 1 ? l.edgeSol : l.preSol;
      double yR = dir == 1 ? l.preY : l.edgeY, solR = dir == 1 ? l.preSol : l.edgeSol;
      if (chg)
      {
         ++nChanges;
         const bool hit = bk::knot_window_hit(l.mark, l.seg, dir);
         const bool expect = l.changedBefore && l.seg == l.rowSeg + dir;
         if (hit != expect) return hit ? "a hit where the window cannot hold the segment's knots" : "a miss one segment further in the direction of the sweep";
         if (hit)
         {
            ++nHits;
            if (!sameKnot(path[(size_t)l.seg], yL, solL) || !sameKnot(path[(size_t)l.seg + 1], yR, solR)) return "a hit with a wrong knot";
         }
         else
         {
            ++nMisses;
            if (!l.changedBefore) ++nFirst;
            else if ((l.seg - l.rowSeg) * dir < 0) ++nAgainst;
            else ++nFar;
            // the literal route
            yL = path[(size_t)l.seg].y; solL = path[(size_t)l.seg].sol;
            yR = path[(size_t)l.seg + 1].y; solR = path[(size_t)l.seg + 1].sol;
         }
         l.usedL.y = yL; l.usedL.sol = solL; l.usedR.y = yR; l.usedR.sol = solR;
      }
      bk::knot_window_shift(chg, dir, yL, solL, yR, solR, l.edgeY, l.edgeSol);
      if (chg) { l.mark = bk::knot_window_mark(l.seg, l.lastSeg, dir); l.changedBefore = true; }
      l.rowSeg = l.seg;
      // every lane loads
      const int at = bk::knot_window_load(l.seg, l.lastSeg, dir);
      if (at < 0 || at > l.lastSeg + 1) return "a load outside the path's knots";
      if (!chg) { ++nReloads; if (l.asked >= 0 && at != l.asked) return "a lane that did not change loads another knot than it holds"; }
      if (at != bk::knot_window_beyond(l.seg, dir)) ++nClamped;
      l.asked = at; l.pending = true; l.preY = l.preSol = POISON;
      if (!late) l.deliver();
      // what the window says it holds
      if (l.mark != bk::KNOT_WINDOW_NONE)
      {
         if (l.mark != l.asked) return "the mark names another knot than the one loaded";
         const int e = l.mark - dir;
         if (e < 0 || e > l.lastSeg + 1 || !sameKnot(path[(size_t)e], l.edgeY, l.edgeSol)) return "the edge pair is not the knot beside the mark";
      }
      else if (l.changedBefore && bk::knot_window_beyond(l.seg, dir) >= 0 && bk::knot_window_beyond(l.seg, dir) <= l.lastSeg + 1)
         return "no usable mark although the knot beyond exists";
      // the coefficients' knots are the segment's
      if (!sameKnot(path[(size_t)l.rowSeg], l.usedL.y, l.usedL.sol) || !sameKnot(path[(size_t)l.rowSeg + 1], l.usedR.y, l.usedR.sol))
         return "coefficients formed from other knots than the segment's";
   }
   return nullptr;
}

} // namespace

int main()
{
   // the smallest knot count the library accepts (4) and 1, 2, 3 more; then longer paths
   const int sizes[8] = {4, 5, 6, 7, 9, 40, 333, 1000};
   std::vector<Path> paths;
   for (int rep = 0; rep < 3; ++rep)
      for (int k = 0; k < 8; ++k) paths.push_back(makePath(sizes[k]));

   for (int late = 0; late < 2; ++late)
      for (int dirI = 0; dirI < 2; ++dirI)
         for (int round = 0; round < 40; ++round)
         {
            const int dir = dirI == 0 ? 1 : -1;
            Lane ln[W];
            for (int k = 0; k < W; ++k) ln[k].init(paths[(size_t)((round * 5 + k * (1 + round % 3)) % (int)paths.size())], dir);
            // how a lane moves in this round: 0 one segment per few queries (slow), 1 one segment per query, 2 two or more per query,
            // 3 a mix with moves against the sweep and random jumps
            int style[W];
            for (int k = 0; k < W; ++k) style[k] = (round + k) % 4;
            const int nQ = 3000;
            for (int q = 0; q < nQ; ++q)
            {
               for (int k = 0; k < W; ++k)
               {
                  Lane &l = ln[k];
                  int step = 0;
                  const uint64_t r = rnd();
                  if (style[k] == 0) step = (r % 23 == 0) ? 1 : 0;
                  else if (style[k] == 1) step = (r % 5 == 0) ? 0 : 1;
                  else if (style[k] == 2) step = 2 + (int)(r % 3);
                  else
                  {
                     const int w = (int)(r % 10);
                     step = w < 3 ? 0 : (w < 6 ? 1 : (w == 6 ? 2 : (w == 7 ? -1 : (w == 8 ? -2 : (int)((r >> 8) % 41) - 20))));
                  }
                  int t = l.seg + dir * step;
                  // at the far end of the path: start over from the near end now and then (one long way against the sweep)
                  const bool atEnd = dir == 1 ? l.seg == l.lastSeg : l.seg == 0;
                  if (atEnd && r % 7 == 3) t = dir == 1 ? 0 : l.lastSeg;
                  l.seg = t < 0 ? 0 : (t > l.lastSeg ? l.lastSeg : t);
               }
               nQueries += W;
               const char *err = block(ln, dir, late != 0);
               if (err)
               {
                  std::printf("mode %d dir %d round %d query %d: %s\n", late, dir, round, q, err);
                  return 1;
               }
            }
         }
   std::printf("ok queries=%lld blocks=%lld changes=%lld hits=%lld misses=%lld far=%lld against=%lld first=%lld reloads=%lld clampedLoads=%lld\n", nQueries,
               nBlocks, nChanges, nHits, nMisses, nFar, nAgainst, nFirst, nReloads, nClamped);
   return 0;
}
