// ba_stretch.cpp -- the seam between BA::optimizeBatch and the time stretch of finished trajectories
// (include/batotp_hip_stretch.h).  This is the only file of the host library that refers to those entry points: the other
// files reach them through the pointer BA::setStretchToLimits leaves in the object, so a program that never asks for a
// stretch links against any implementation of include/batotp_hip.h.
#include <vector>

#include "ba.h"
#include "batotp_hip_stretch.h"

namespace BATOTP
{

static int stretchRange(void *output, const void *problem, double target, int maxRounds, double maxFactor, size_t n, void **out, BatchStretch *report)
{
   batotp_output *r = nullptr;
   std::vector<batotp_path_stretch> rows(n);
   const int rc = batotp_hip_output_stretch_audit(static_cast<batotp_output *>(output), static_cast<const batotp_problem *>(problem), target,
                                                  (int32_t)maxRounds, maxFactor, &r, rows.data());
   *out = r;
   if (rc != BATOTP_OK) return rc;
   for (size_t k = 0; k < n; ++k)
   {
      BatchStretch &s = report[k];
      s.nIn = rows[k].n_in; s.nOut = rows[k].n_out;
      s.factor = rows[k].factor;
      s.rounds = rows[k].rounds; s.status = rows[k].status;
      s.done = true;
   }
   return BATOTP_OK;
}

void BA::setStretchToLimits(double target, int maxRounds, double maxFactor)
{
   _stretchTarget = target; _stretchRounds = maxRounds; _stretchMaxFactor = maxFactor;
   _stretchFn = target > 0 ? &stretchRange : nullptr;
}

} // namespace BATOTP
