// knot_window.h -- the knots of the compact layout (FEAT < 0) around the knot cursor of k_sweep8 / k_sweep8_lock as a register window of
// two knots.  Plain inline functions, branch-free, no ballots, no loads: the kernels keep the wavefront-uniform guard of the segment
// change, the formulas and the loads; a CPU compiler builds the same statements (tests/drivers/knot_window_main.cpp).
//
// A cursor that sweeps in direction dir (+1 forward, -1 reverse) and last changed into segment `seg` (knots seg and seg + 1) holds
//      the edge knot: the knot of `seg` on the side the sweep moves to     (forward: seg + 1, reverse: seg)
//      the prefetch knot: the one beyond it                                (forward: seg + 2, reverse: seg - 1)
// so a change one segment further in the direction of the sweep finds both of its knots in registers (a hit): its near knot is the
// edge, its far knot the prefetch.  Any other change -- two or more segments, against the sweep, the first one of a path -- is a miss and
// takes the literal route with its own loads.  Which index the prefetch register holds is kept as one integer, the mark: the index
// itself, or KNOT_WINDOW_NONE where it would lie outside [0, lastSeg + 1] (the register then holds the knot of the clamped index, which
// nothing reads; no segment equals the marker, so such a window never hits).
// The load of the prefetch knot is issued by EVERY lane that is active in a segment-change block, changed or not, from
// knot_window_load(seg, ..) of the lane's (new) segment -- a lane that did not change loads what it holds -- straight into the window's
// registers; nothing reads them before the next segment-change block of the wavefront.  (One load per changed lane, inside `if (chg)`,
// makes the compiler load into fresh registers and copy them into place behind an s_waitcnt vmcnt(0) on the spot --
// profiles/fwd_curve_window_code_object.txt section 4, profiles/knot_window_code_object.txt.)
#pragma once

#if defined(__HIPCC__)
#define KNOTW_FN __host__ __device__ inline
#else
#define KNOTW_FN inline
#endif

namespace bk
{

constexpr int KNOT_WINDOW_NONE = -(1 << 20); // the mark of a window that holds no usable pair

// index of the knot beyond the edge of `seg`, unclamped
KNOTW_FN int knot_window_beyond(int seg, int dir) { return dir == 1 ? seg + 2 : seg - 1; }

// the knot a lane on segment `seg` loads into the prefetch register: clamped to the path's knots [0, lastSeg + 1]
KNOTW_FN int knot_window_load(int seg, int lastSeg, int dir)
{
   const int nxt = knot_window_beyond(seg, dir);
   return nxt < 0 ? 0 : (nxt > lastSeg + 1 ? lastSeg + 1 : nxt);
}

// the mark after a change into `seg`: a clamped prefetch holds no usable knot
KNOTW_FN int knot_window_mark(int seg, int lastSeg, int dir)
{
   const int nxt = knot_window_beyond(seg, dir);
   return nxt < 0 ? KNOT_WINDOW_NONE : (nxt > lastSeg + 1 ? KNOT_WINDOW_NONE : nxt);
}

// does a change into `seg` find both of its knots in the window (edge = its near knot, prefetch = its far knot)?
KNOTW_FN bool knot_window_hit(int mark, int seg, int dir) { return dir == 1 ? (mark == seg + 1) : (mark == seg); }

// The shift of a lane that changed into a segment with the knots (yL, solL) = knot seg and (yR, solR) = knot seg + 1, wherever they came
// from: the edge takes the far knot.  A lane that did not change keeps its edge.  (The prefetch register follows by the caller's load.)
KNOTW_FN void knot_window_shift(bool chg, int dir, double yL, double solL, double yR, double solR, double &edgeY, double &edgeSol)
{
   const double fy = dir == 1 ? yR : yL, fs = dir == 1 ? solR : solL;
   edgeY = chg ? fy : edgeY;
   edgeSol = chg ? fs : edgeSol;
}

} // namespace bk
