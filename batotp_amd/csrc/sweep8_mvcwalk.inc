// sweep8_mvcwalk.inc -- BA::updateCurSeg on the reverse curve (ba.cpp:1592, 1617-1652) inside k_sweep8 (included twice: forward
// predictor and evalsdot).  In scope: sCur, segM, the segment's two points (mS0, mD0), (mS1, mD1), mvc, nMvc, status.  The
// walk is the reference's comparison walk from the cached segment; a move costs one 16-byte load (the point that enters).
{
   for (;;)
   {
      const bool inM = (sCur >= mS0) & (sCur <= mS1);
      const bool upM = !inM & (sCur > mS0), dnM = !inM & (sCur < mS0);
      status |= (!inM & !upM & !dnM) ? (unsigned)BATOTP_ST_NONFINITE : 0u;
      const bool mvUpM = upM & (segM < nMvc - 2), mvDnM = dnM & (segM > 0);
      if (!S8_ANY(mvUpM | mvDnM)) break;
      const double2 qM = mvc[mvUpM ? segM + 2 : (mvDnM ? segM - 1 : segM)];
      const double nS0 = mvUpM ? mS1 : (mvDnM ? qM.x : mS0), nD0 = mvUpM ? mD1 : (mvDnM ? qM.y : mD0);
      const double nS1 = mvUpM ? qM.x : (mvDnM ? mS0 : mS1), nD1 = mvUpM ? qM.y : (mvDnM ? mD0 : mD1);
      mS0 = nS0; mD0 = nD0; mS1 = nS1; mD1 = nD1;
      segM += mvUpM ? 1 : (mvDnM ? -1 : 0);
   }
}
