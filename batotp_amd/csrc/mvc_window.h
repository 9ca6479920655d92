// mvc_window.h -- the per-lane step of BA::updateCurSeg on the reverse curve (ba.cpp:1592, 1617-1652) over a register window of
// four curve points.  Plain inline functions, branch-free, no ballots, no loads: sweep8_mvcwalk.inc keeps the wavefront-uniform
// loop, the ballot and the loads; a CPU compiler builds the same statements (tests/drivers/mvc_window_main.cpp).
//
// The window of a cursor on segment `seg` of a curve of n points holds the points
//      seg - 1: (sLo, dLo)      seg: (s0, d0)      seg + 1: (s1, d1)      seg + 2: (sHi, dHi)
// Which index a neighbour holds follows from `seg` alone, so no index is kept: the lower neighbour is usable iff seg > 0, the upper
// one iff seg < n - 2 (otherwise it holds the point of the clamped index, mvc_window_lo / mvc_window_hi, which nothing reads).
// These are exactly the conditions under which the walk may move down / up, so a move always finds the point that enters the
// segment in the window.  A move shifts the segment by one point inside the window and leaves BOTH neighbours to be loaded again,
// from mvc_window_lo(seg) and mvc_window_hi(seg, n) of the NEW seg, in every lane, moved or not (a lane that did not move loads
// what it holds).  The caller issues the two loads after the shift and does not wait for them: their next read is the next move of
// some cursor of the wavefront.  (One load per moved lane, predicated on the direction or selected into place, makes the compiler
// copy the loaded pair behind an s_waitcnt vmcnt(0) on the spot -- profiles/fwd_curve_window_code_object.txt.)
#pragma once
#include "batotp_hip.h"

#if defined(__HIPCC__)
#define MVCW_FN __host__ __device__ inline
#else
#define MVCW_FN inline
#endif

namespace bk
{

// indices of the window's neighbours, clamped to the curve
MVCW_FN int mvc_window_lo(int seg) { return seg > 0 ? seg - 1 : 0; }
MVCW_FN int mvc_window_hi(int seg, int n) { return seg + 2 < n ? seg + 2 : n - 1; }

struct MvcMove
{
   bool up, dn;     // the cursor leaves its segment upwards / downwards (never both)
   unsigned status; // BATOTP_ST_NONFINITE if sCur compares with nothing, else 0
};

// The comparison of the reference's walk from the cached segment [s0, s1] (inclusive ends) on segment `seg` of n points.
MVCW_FN MvcMove mvc_window_test(double sCur, int seg, int n, double s0, double s1)
{
   const bool in = (sCur >= s0) & (sCur <= s1);
   const bool up = !in & (sCur > s0), dn = !in & (sCur < s0);
   MvcMove m;
   m.status = (!in & !up & !dn) ? (unsigned)BATOTP_ST_NONFINITE : 0u;
   m.up = up & (seg < n - 2);
   m.dn = dn & (seg > 0);
   return m;
}

// The move: the point that enters the segment comes from the window.  Afterwards the neighbours (sLo, dLo) / (sHi, dHi) belong to
// the OLD seg until the caller has loaded them again (above); seg and the segment's two points are final.
MVCW_FN void mvc_window_shift(const MvcMove m, int &seg, double sLo, double dLo, double &s0, double &d0, double &s1, double &d1, double sHi,
                              double dHi)
{
   const double nS0 = m.up ? s1 : (m.dn ? sLo : s0), nD0 = m.up ? d1 : (m.dn ? dLo : d0);
   const double nS1 = m.up ? sHi : (m.dn ? s0 : s1), nD1 = m.up ? dHi : (m.dn ? d0 : d1);
   s0 = nS0; d0 = nD0; s1 = nS1; d1 = nD1;
   seg += m.up ? 1 : (m.dn ? -1 : 0);
}

} // namespace bk
