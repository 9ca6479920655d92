// sweep8_mvcwalk.inc -- BA::updateCurSeg on the reverse curve (ba.cpp:1592, 1617-1652) inside k_sweep8 and k_sweep8_lock (included
// twice in each: forward predictor and evalsdot).  In scope: sCur, segM, the window of four curve points around the cursor (mvc_window.h:
// (mSLo, mDLo), the segment's (mS0, mD0), (mS1, mD1), and (mSHi, mDHi)), mvc, nMvc, status.  The walk is the reference's comparison
// walk from the cached segment.  The point that enters the segment on a move is already in the window; a pass in which some path
// moves issues two 16-byte loads, of the window's neighbours around the new segment, and nothing reads their result before the next
// pass in which some path moves.  Only a second such pass of the same walk -- some path of the wavefront moves twice -- waits
// for the loads of the first.
{
   for (;;)
   {
      const MvcMove mvM = mvc_window_test(sCur, segM, nMvc, mS0, mS1);
      status |= mvM.status;
      // "does any cursor move": mvM.up | mvM.dn over the wavefront, from the masks of the comparisons themselves (S8_MASK, sweep8.hip.h).
      // up = !in & (sCur > s0) & (seg < n - 2) is (sCur > s0) & !(sCur <= s1) & (seg < n - 2): sCur > s0 implies sCur >= s0;
      // dn = !in & (sCur < s0) & (seg > 0) is (sCur < s0) & (seg > 0): sCur < s0 implies !in
      const s8_mask mUpM = S8_MASK(sCur > mS0) & S8_MASK(!(sCur <= mS1)) & S8_MASK(segM < nMvc - 2);
      const s8_mask mDnM = S8_MASK(sCur < mS0) & S8_MASK(segM > 0);
      if ((mUpM | mDnM) == 0) break;
      mvc_window_shift(mvM, segM, mSLo, mDLo, mS0, mD0, mS1, mD1, mSHi, mDHi);
      const double2 qLoM = mvc[mvc_window_lo(segM)], qHiM = mvc[mvc_window_hi(segM, nMvc)];
      mSLo = qLoM.x; mDLo = qLoM.y; mSHi = qHiM.x; mDHi = qHiM.y;
   }
}
