/*
 * batotp_hip_clamp_kat.h -- known-answer test of the clamp chain of a sweep stage's prologue (batotp_amd/csrc/device_math.h:
 * clamp_chain_literal, clamp_chain_fast, clamp_consts_ok, clamp_raw_ok), on the device.  include/batotp_hip.h is unchanged.
 *
 * For each of the n operand tuples (raw[i], interp[i], cap[i], smin[i], lim1[i]), with the floor +0.0 of every sweep:
 *    literal[i]  the forward chain as the reference writes it, with compare-and-select (std::max / std::min of ba.cpp:1085, 1204-1236):
 *                   v = max(raw, +0); m = max(interp, smin); v = v > m ? m : v; v = min(v, cap); v = max(v, smin); v = min(v, lim1)
 *    fast[i]     the same chain through v_max_f64 / v_min_f64, one instruction per clamp
 *    valid[i]    1 where the kernels take the fast chain: clamp_consts_ok(+0, smin, cap) && clamp_raw_ok(raw, interp), else 0
 * (In the kernels lim1 is a fabs of a finite quotient, or +inf; with vN >= smin > 0 by then the last clamp agrees for any lim1.)
 * The entry point returns BATOTP_ERR_ARG for n <= 0 or a null pointer.  tests/test_gpu_stage_clamps.py holds the assertions.
 */
#ifndef BATOTP_HIP_CLAMP_KAT_H
#define BATOTP_HIP_CLAMP_KAT_H

#include "batotp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int batotp_hip_clamp_kat(batotp_ctx *ctx, int64_t n, const double *raw, const double *interp, const double *cap, const double *smin,
                         const double *lim1, double *literal, double *fast, int32_t *valid);

#ifdef __cplusplus
}
#endif

#endif
