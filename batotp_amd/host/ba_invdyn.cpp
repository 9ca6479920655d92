// ba_invdyn.cpp -- the seam between BA::optimizeBatch and the torque rows for finished trajectories
// (include/batotp_hip_invdyn.h).  This is the only file of the host library that refers to those entry points: the other
// files reach them through the pointer BA::setOutputTorques leaves in the object, so a program that never asks for torque
// rows links against any implementation of include/batotp_hip.h.
#include "ba.h"
#include "batotp_hip_invdyn.h"

namespace BATOTP
{

static int torquesOfRange(void *output, const void *model, unsigned int flags, void **out)
{
   batotp_output *r = nullptr;
   const int rc = batotp_hip_output_torques(static_cast<batotp_output *>(output), static_cast<const batotp_serial_model *>(model), (uint32_t)flags, &r);
   *out = r;
   return rc;
}

void BA::setOutputTorques(bool on)
{
   _torquesFn = on ? &torquesOfRange : nullptr;
}

} // namespace BATOTP
