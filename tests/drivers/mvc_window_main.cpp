// mvc_window_main.cpp -- the reverse-curve cursor of the forward batch kernels without a GPU (tests/test_mvc_window.py).
// Replays, side by side and query by query,
//   (a) the literal walk over the whole array: the statements sweep8_mvcwalk.inc had before the window (the cached segment is
//       read from the array at every pass), and
//   (b) the window walk of batotp_amd/csrc/mvc_window.h as sweep8_mvcwalk.inc drives it: eight cursors ("lanes", each on a curve
//       of its own) in one wavefront-uniform loop -- while any lane moves, every lane shifts and asks for both neighbours again.
// The loads of (b) go through a fake loader that hands out array elements only when asked: at once (mode 0), or when the NEXT query
// begins (mode 1), unless a move needs the pair sooner -- that is a wait, and it is counted.  A pair that has not been handed out
// holds a poison value.  After every query: seg, the segment's four values and the status bits of (a) and (b) are equal, bit for
// bit; (b) never asked for an index outside [0, n - 1] and never moved onto a pair it had not been given for that index.
// Prints "ok queries=<total> waits0=<waits in mode 0> waits1=<waits in mode 1> moves=<...>"; exit status 1 at the first difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mvc_window.h"

namespace
{

struct Pt { double s, d; };
typedef std::vector<Pt> Curve;

uint64_t rngState = 0x9e3779b97f4a7c15ull;
uint64_t rnd()
{
   rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17;
   return rngState;
}
double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

// kind 0: strictly increasing s; 1: every other value repeated; 2: runs of three equal values
Curve makeCurve(int n, int kind)
{
   Curve c((size_t)n);
   double s = 0;
   for (int k = 0; k < n; ++k)
   {
      const bool rep = (kind == 1 && (k & 1)) || (kind == 2 && (k % 4 == 1 || k % 4 == 2));
      if (k > 0 && !rep) s += 0.01 + uni();
      c[(size_t)k].s = s;
      c[(size_t)k].d = 1.0 + uni() * 5.0;
   }
   return c;
}

const double POISON = -7.25e300;

// (a) the literal walk
struct Literal
{
   const Curve *c;
   int seg;
   double s0, d0, s1, d1;
   unsigned status;
   void init(const Curve &cv)
   {
      c = &cv; seg = 0; status = 0;
      s0 = cv[0].s; d0 = cv[0].d; s1 = cv[1].s; d1 = cv[1].d;
   }
   void query(double sCur)
   {
      const int n = (int)c->size();
      for (;;)
      {
         const bool in = (sCur >= s0) & (sCur <= s1);
         const bool up = !in & (sCur > s0), dn = !in & (sCur < s0);
         status |= (!in & !up & !dn) ? (unsigned)BATOTP_ST_NONFINITE : 0u;
         const bool mvUp = up & (seg < n - 2), mvDn = dn & (seg > 0);
         if (!(mvUp | mvDn)) break;
         seg += mvUp ? 1 : -1;
         s0 = (*c)[(size_t)seg].s; d0 = (*c)[(size_t)seg].d; s1 = (*c)[(size_t)seg + 1].s; d1 = (*c)[(size_t)seg + 1].d;
      }
   }
};

// (b) one lane of the window walk and its side of the fake loader
struct Lane
{
   const Curve *c;
   int seg;
   double sLo, dLo, s0, d0, s1, d1, sHi, dHi;
   unsigned status;
   int askedLo, askedHi;     // index of the last load into the pair
   bool pendLo, pendHi;      // asked for, not handed out yet
   void deliver()
   {
      if (pendLo) { sLo = (*c)[(size_t)askedLo].s; dLo = (*c)[(size_t)askedLo].d; pendLo = false; }
      if (pendHi) { sHi = (*c)[(size_t)askedHi].s; dHi = (*c)[(size_t)askedHi].d; pendHi = false; }
   }
   bool ask(bool late)
   {
      const int n = (int)c->size();
      askedLo = bk::mvc_window_lo(seg);
      askedHi = bk::mvc_window_hi(seg, n);
      if (askedLo < 0 || askedLo > n - 1 || askedHi < 0 || askedHi > n - 1) return false;
      sLo = dLo = sHi = dHi = POISON;
      pendLo = pendHi = true;
      if (!late) deliver();
      return true;
   }
   bool init(const Curve &cv)
   {
      c = &cv; seg = 0; status = 0;
      s0 = cv[0].s; d0 = cv[0].d; s1 = cv[1].s; d1 = cv[1].d;
      const bool ok = ask(false);
      return ok;
   }
};

const int W = 8;
long long waits[2] = {0, 0}, moves = 0, passes = 0;

// one walk of the wavefront; false: a lane was about to move onto a pair it does not hold, or asked outside its curve
bool walk(Lane *ln, const double *sCur, bool late)
{
   if (late)
      for (int k = 0; k < W; ++k) ln[k].deliver();   // what the previous query asked for has arrived
   for (;;)
   {
      bk::MvcMove m[W];
      bool any = false;
      for (int k = 0; k < W; ++k)
      {
         m[k] = bk::mvc_window_test(sCur[k], ln[k].seg, (int)ln[k].c->size(), ln[k].s0, ln[k].s1);
         ln[k].status |= m[k].status;
         any |= m[k].up | m[k].dn;
      }
      if (!any) break;
      ++passes;
      // the shift reads the pair a moving lane enters: it must be the one asked for, and a pending one is waited for (all
      // lanes of the wavefront wait together: one wait per pass)
      bool waited = false;
      for (int k = 0; k < W; ++k)
      {
         Lane &l = ln[k];
         if (m[k].up && m[k].dn) return false;
         if (m[k].up) { if (l.askedHi != l.seg + 2) return false; waited |= l.pendHi; }
         if (m[k].dn) { if (l.askedLo != l.seg - 1) return false; waited |= l.pendLo; }
         moves += (m[k].up | m[k].dn) ? 1 : 0;
      }
      if (waited)
      {
         ++waits[late ? 1 : 0];
         for (int k = 0; k < W; ++k) ln[k].deliver();
      }
      for (int k = 0; k < W; ++k)
      {
         Lane &l = ln[k];
         bk::mvc_window_shift(m[k], l.seg, l.sLo, l.dLo, l.s0, l.d0, l.s1, l.d1, l.sHi, l.dHi);
         if ((m[k].up | m[k].dn) && (l.s0 == POISON || l.s1 == POISON || l.d0 == POISON || l.d1 == POISON)) return false;
         // every lane loads both neighbours again, moved or not; what was pending and unread is overwritten by the same values
         if (!l.ask(late)) return false;
      }
   }
   return true;
}

bool same(const Literal &a, const Lane &b)
{
   return a.seg == b.seg && a.status == b.status && !std::memcmp(&a.s0, &b.s0, 8) && !std::memcmp(&a.d0, &b.d0, 8) &&
          !std::memcmp(&a.s1, &b.s1, 8) && !std::memcmp(&a.d1, &b.d1, 8);
}

// the midpoint of the segment `jump` away from the cursor's (clamped to the curve)
double jumpTarget(const Literal &a, int jump)
{
   const int n = (int)a.c->size();
   int t = a.seg + jump;
   t = t < 0 ? 0 : (t > n - 2 ? n - 2 : t);
   return 0.5 * ((*a.c)[(size_t)t].s + (*a.c)[(size_t)t + 1].s);
}

} // namespace

int main()
{
   const int sizes[5] = {2, 3, 4, 5, 1000};
   std::vector<Curve> curves;
   for (int kind = 0; kind < 3; ++kind)
      for (int k = 0; k < 5; ++k) curves.push_back(makeCurve(sizes[k], kind));
   const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
   const int jumps[7] = {0, 1, -1, 2, -2, 5, -5};
   long long queries = 0;

   for (int late = 0; late < 2; ++late)
      for (int round = 0; round < 30; ++round)
      {
         // eight lanes on eight curves: every curve meets every other kind of neighbour over the rounds
         Literal lit[W];
         Lane ln[W];
         for (int k = 0; k < W; ++k)
         {
            const Curve &cv = curves[(size_t)((round * 7 + k * (1 + round % 4)) % (int)curves.size())];
            lit[k].init(cv);
            if (!ln[k].init(cv)) { std::printf("init asked outside the curve\n"); return 1; }
         }
         double sCur[W], s0v[W], hv[W];
         for (int k = 0; k < W; ++k) { s0v[k] = 0; hv[k] = 0; }
         const int nQ = 2400;
         for (int q = 0; q < nQ; ++q)
         {
            const int phase = (q / 300) % 4;   // 0: points and their ulps, 1: jumps, 2: forward steps, 3: forward steps with non-finite ones between
            for (int k = 0; k < W; ++k)
            {
               const Curve &cv = *lit[k].c;
               const int n = (int)cv.size();
               double s;
               if (phase == 0)
               {
                  const double p = cv[(size_t)(rnd() % (uint64_t)n)].s;
                  const int side = (int)(rnd() % 3);
                  s = side == 0 ? p : (side == 1 ? std::nextafter(p, inf) : std::nextafter(p, -inf));
               }
               else if (phase == 1)
                  s = jumpTarget(lit[k], jumps[rnd() % 7]);
               else
               {
                  // predictor, stages 1..6 of a step of the forward sweep: up, back down, up again; the step spans 0.1 to 3 mean segments
                  static const double frac[7] = {1.0, 0.2, 0.3, 0.8, 8.0 / 9.0, 1.0, 1.0};
                  const int st = q % 7;
                  if (st == 0)
                  {
                     s0v[k] += hv[k];
                     const double mean = cv[(size_t)n - 1].s / (double)(n - 1);
                     hv[k] = mean * (0.1 + 2.9 * uni());
                     if (s0v[k] > cv[(size_t)n - 1].s) { s0v[k] = 0; }   // a new pass over the curve: one long way down
                  }
                  s = s0v[k] + frac[st] * hv[k];
                  if (phase == 3 && rnd() % 97 == 0)
                  {
                     const int w = (int)(rnd() % 3);
                     s = w == 0 ? nan : (w == 1 ? inf : -inf);
                  }
               }
               sCur[k] = s;
               lit[k].query(s);
            }
            if (!walk(ln, sCur, late != 0))
            {
               std::printf("mode %d round %d query %d: a move onto a pair that was not given, or a load outside the curve\n", late, round, q);
               return 1;
            }
            for (int k = 0; k < W; ++k)
               if (!same(lit[k], ln[k]))
               {
                  std::printf("mode %d round %d query %d lane %d (n = %d): literal seg %d status %u [%a %a %a %a], window seg %d status %u [%a %a %a %a]\n",
                              late, round, q, k, (int)lit[k].c->size(), lit[k].seg, lit[k].status, lit[k].s0, lit[k].d0, lit[k].s1, lit[k].d1,
                              ln[k].seg, ln[k].status, ln[k].s0, ln[k].d0, ln[k].s1, ln[k].d1);
                  return 1;
               }
            queries += W;
         }
      }
   std::printf("ok queries=%lld waits0=%lld waits1=%lld moves=%lld passes=%lld\n", queries, waits[0], waits[1], moves, passes);
   return 0;
}
