// ba_tscale.cpp -- the seam between BA::optimizeBatch and the stretch of finished trajectories until their torque limits pass
// (include/batotp_hip_tscale.h).  This is the only file of the host library that refers to those entry points: the other
// files reach them through the pointer BA::setStretchToTorqueLimits leaves in the object, so a program that never asks for
// it links against any implementation of include/batotp_hip.h.
#include <vector>

#include "ba.h"
#include "batotp_hip_tscale.h"

namespace BATOTP
{

static int stretchTorquesOfRange(void *output, const void *problem, const void *model, unsigned int flags, double target, int maxRounds, double maxFactor,
                                 size_t n, void **out, BatchStretch *report)
{
   batotp_output *r = nullptr;
   std::vector<batotp_path_stretch> rows(n);
   const int rc = batotp_hip_output_stretch_torques(static_cast<batotp_output *>(output), static_cast<const batotp_problem *>(problem),
                                                    static_cast<const batotp_serial_model *>(model), (uint32_t)flags, target, (int32_t)maxRounds, maxFactor, &r,
                                                    rows.data(), nullptr);
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

void BA::setStretchToTorqueLimits(double target, int maxRounds, double maxFactor)
{
   _tscaleTarget = target; _tscaleRounds = maxRounds; _tscaleMaxFactor = maxFactor;
   _tscaleFn = target > 0 ? &stretchTorquesOfRange : nullptr;
}

} // namespace BATOTP
