// ba_kin.cpp -- the seam between BA and the kinematic chain of the device layer (include/batotp_hip_kin.h).
// This is the only file of the host library that refers to the chain's entry points: the other files reach them through
// the pointers BA::setToolPoint leaves in the object, so a program that never sets a tool point links against any
// implementation of include/batotp_hip.h.
#include "ba.h"
#include "batotp_hip_kin.h"

namespace BATOTP
{

static int resampleWithChain(void *ctx, const void *params, const void *chain, int nPaths, const int64_t *nIn, const double *x, const double *sresIn,
                             void **out)
{
   batotp_resampled *r = nullptr;
   const int rc = batotp_hip_resample_chain(static_cast<batotp_ctx *>(ctx), static_cast<const batotp_resample_params *>(params),
                                            static_cast<const batotp_kin_chain *>(chain), (int32_t)nPaths, nIn, x, sresIn, &r);
   *out = r;
   return rc;
}

static int batchChain(void *batch, const void *chain)
{
   return batotp_hip_set_kin_chain(static_cast<batotp_batch *>(batch), static_cast<const batotp_kin_chain *>(chain));
}

void BA::setToolPoint(const double tool[3])
{
   myRobot.setToolPoint(tool);
   _kinResampleFn = &resampleWithChain;
   _kinBatchFn = &batchChain;
}

} // namespace BATOTP
