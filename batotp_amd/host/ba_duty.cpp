// ba_duty.cpp -- the seam between BA::optimizeBatch and the stretch of finished trajectories until their RMS torques are inside the
// drives' continuous torques (include/batotp_hip_duty.h).  This is the only file of the host library that refers to those entry
// points: the other files reach them through the pointer BA::setStretchToRatedTorques leaves in the object, so a program that
// never asks for it links against any implementation of include/batotp_hip.h.
#include <vector>

#include "ba.h"
#include "batotp_hip_duty.h"

namespace BATOTP
{

static int stretchDutyOfRange(void *output, const void *problem, const void *model, unsigned int flags, const double *rated, double target, int maxRounds,
                              double maxFactor, size_t n, void **out, BatchStretch *report, BatchDuty *duty)
{
   batotp_output *r = nullptr;
   std::vector<batotp_path_stretch> rows(n);
   std::vector<batotp_path_duty> recs(n);
   const int rc = batotp_hip_output_stretch_duty(static_cast<batotp_output *>(output), static_cast<const batotp_problem *>(problem),
                                                 static_cast<const batotp_serial_model *>(model), (uint32_t)flags, rated, target, (int32_t)maxRounds, maxFactor, &r,
                                                 rows.data(), nullptr, recs.data());
   *out = r;
   if (rc != BATOTP_OK) return rc;
   for (size_t k = 0; k < n; ++k)
   {
      BatchStretch &s = report[k];
      s.nIn = rows[k].n_in; s.nOut = rows[k].n_out;
      s.factor = rows[k].factor;
      s.rounds = rows[k].rounds; s.status = rows[k].status;
      s.done = true;
      BatchDuty &d = duty[k];
      for (int j = 0; j < 8 && j < BATOTP_MAX_LINKS; ++j) d.rms[j] = recs[k].rms[j];
      d.util = recs[k].util; d.row = recs[k].row; d.nHold = recs[k].n_hold;
      d.s = recs[k].s; d.sRow = recs[k].s_row;
      d.energy = recs[k].energy; d.peakPower = recs[k].peak_power; d.powerAt = recs[k].power_at; d.nPts = recs[k].n_pts;
      d.done = true;
   }
   return BATOTP_OK;
}

void BA::setStretchToRatedTorques(const std::vector<double> &rated, double target, int maxRounds, double maxFactor)
{
   _dutyRated = rated;
   _dutyTarget = target; _dutyRounds = maxRounds; _dutyMaxFactor = maxFactor;
   _dutyFn = (target > 0 && !rated.empty()) ? &stretchDutyOfRange : nullptr;
}

} // namespace BATOTP
