/*
 * batotp_hip_duty.h -- the CONTINUOUS (rated) torque of finished trajectories: RMS torques, energy, peak power, and a stretch until
 * the RMS torque of every joint is inside its rating.
 *
 * The torque scale (batotp_hip_tscale.h) checks and enforces the PEAK torque.  A drive's second figure is its continuous torque,
 * against which the RMS torque of a repeated motion is sized.  Under a dilation of time by k the torque at a point is
 * A / k^2 + B / k + G, so the mean square of a joint's torque over the path is a QUARTIC in x = 1/k whose five coefficients are
 * sums over the path: one streaming pass gives the RMS torque of every joint and the speed factor at which it meets its rating.
 * The mechanical energy and the peak power come out of the same registers.
 *
 * ---- definition (the tests pin it bit for bit; DESIGN.md 4 and tests/duty_reference.py restate it) ---------------------------
 * This definition is the library's own: the reference has no counterpart.
 * All arithmetic is binary64, in exactly the order written, without contraction; `/` and sqrt are the correctly rounded ones;
 * every reciprocal is formed once on the host.
 *
 * Per point i of a path: A_j, B_j, G_j and tau_j = (A_j + B_j) + G_j are EXACTLY those of batotp_hip_tscale.h, and qd_j is the
 * unit * v_j of batotp_hip_invdyn.h.  Then, each a single rounded product,
 *       m0 = A*A   m1 = A*B   m2 = B*B   m3 = A*G   m4 = B*G   m5 = G*G   m6 = tau*tau          (seven per joint)
 *       p = tau_0*qd_0;  p = p + tau_j*qd_j  for j = 1 .. n_links-1                              (power)
 *       w = (p > 0) ? p : 0.0                                                                    (its positive part)
 *
 * The sum is part of the definition.  A path is cut into blocks of BATOTP_DUTY_BLOCK_POINTS = 128 points, two wavefronts of 64.
 * Lanes past the end of the path contribute +0.0.  Inside a wavefront of 64 values: v[l] = v[l] + v[l+32] for l < 32, then the
 * same with 16, 8, 4, 2, 1.  Block sum = wave 0 + wave 1.  Path sum = the block sums added one after another in ascending block
 * order, ((b0 + b1) + b2) + ...; a path without points has the sum +0.0.  The same rule for all 7 n_links + 1 quantities
 * (S0..S6 of every joint from m0..m6, and W from w).
 *
 * Peak power: the largest p that is not NaN; ties go to the lowest point; none: -Inf and at = -1.
 *
 * Host rule, from the sums of one path of n points, with rr_j = 1.0 / rated_j and lim_j = target * rated_j:
 *       rms_j = sqrt(S6_j / (double)n)          u_j = rms_j * rr_j
 *       util = the largest u_j that is finite, row = its joint, ties to the lowest joint; n = 0 or no finite u: util = -1, row = -1
 *       L_j = (lim_j*lim_j) * (double)n
 *       c4 = S0   c3 = 2.0*S1   c2 = S2 + 2.0*S3   c1 = 2.0*S4   c0 = S5
 *       P_j(x) = (((c4*x + c3)*x + c2)*x + c1)*x + c0
 *       joint j HOLDS iff !(c0 < L_j): gravity alone reaches the rating and no dilation helps; n_hold counts such joints
 *       a joint that does not hold and has !(P_j(1.0) <= L_j) gets a candidate from exactly 64 passes of
 *             lo = 0.0, hi = 1.0;   mid = 0.5*(lo+hi);  if P_j(mid) <= L_j then lo = mid else hi = mid;     the candidate is lo
 *       s = the smallest candidate, s_row = its joint, ties to the lowest joint; none: s = +Inf, s_row = -1
 *       energy = h * W          (h: the time step of the path)
 * A path without points is not evaluated: rms 0, util -1, row -1, n_hold 0, s +Inf, s_row -1, energy +0.0.
 */
#ifndef BATOTP_HIP_DUTY_H
#define BATOTP_HIP_DUTY_H

#include "batotp_hip_tscale.h"

#ifdef __cplusplus
extern "C" {
#endif

/* points per block of the sum; public because the sum depends on it */
#define BATOTP_DUTY_BLOCK_POINTS 128
#if defined(__cplusplus)
static_assert(BATOTP_DUTY_BLOCK_POINTS == BATOTP_TSCALE_BLOCK_POINTS, "the duty kernel has the grid and the lanes of the scale kernel");
#else
_Static_assert(BATOTP_DUTY_BLOCK_POINTS == BATOTP_TSCALE_BLOCK_POINTS, "the duty kernel has the grid and the lanes of the scale kernel");
#endif

typedef struct batotp_path_duty {        /* 128 bytes */
    double  rms[BATOTP_MAX_LINKS];       /* RMS torque of every joint, 0 beyond n_links                                     */
    double  util;                        /* largest finite rms_j / rated_j, -1 if none                                      */
    int32_t row;                         /* its joint, -1 if none                                                           */
    int32_t n_hold;                      /* joints whose gravity torque alone reaches target * rated                        */
    double  s;                           /* largest speed factor x = 1/k at which every joint that can meets its rating; +Inf if none binds */
    int32_t s_row;                       /* joint of s, -1 if none                                                          */
    int32_t reserved;                    /* 0                                                                               */
    double  energy;                      /* h * sum of the positive part of the mechanical power                            */
    double  peak_power;                  /* largest power that is not NaN, -Inf if none                                     */
    int64_t power_at;                    /* its point, -1 if none                                                           */
    int64_t n_pts;
} batotp_path_duty;

typedef struct batotp_path_duty_sums {   /* 480 bytes: what the kernels write */
    double  S[BATOTP_MAX_LINKS][7];      /* path sums of m0..m6 of every joint, +0.0 beyond n_links                         */
    double  W;                           /* path sum of w                                                                   */
    double  peak_power;
    int64_t power_at;
    int64_t n_pts;
} batotp_path_duty_sums;

/* The known-answer entry.  A NEW output: the rows of o followed by model->n_links torque rows, bit for bit those of
 * batotp_hip_output_torques(o, model, flags), AND one record per path in duty[n_paths] (host; may be NULL only for an output
 * without paths) and, if sums is not NULL, the raw sums in sums[n_paths].  rated[n_links]: the continuous torque of every joint.
 * BATOTP_ERR_ARG with a message (batotp_hip_last_error), *out = NULL, nothing launched: everything batotp_hip_output_torques
 * refuses, an o that has torque rows, a rated_j of a joint in use that is not finite and positive, a target outside (0, 1].
 * Ranges of paths under batotp_hip_set_workspace_budget as batotp_hip_output_torques cuts them; nothing depends on the cut. */
int batotp_hip_output_duty(batotp_output *o, const batotp_serial_model *model, uint32_t flags, const double *rated, double target,
                           batotp_output **out, batotp_path_duty *duty, batotp_path_duty_sums *sums);
/* The rounds of batotp_hip_output_stretch_torques with the RMS family on top.  A round makes the torque rows, the scale records
 * AND the duty records of the current rows in one pass over them, then audits as batotp_hip_output_stretch_torques does.
 *       rms_ok = util <= target or util == -1
 *       if !rms_ok:  ok = false, and if n_hold == 0 && s < 1.0:  need = max(need, 1.0 / s)
 *    decided in this order:
 *       1. ok:                                                                BATOTP_STRETCH_PASSES
 *       2. kin_ok && ((!trq_ok && n_static > 0) || (!rms_ok && n_hold > 0)):  BATOTP_STRETCH_STATIC
 *       3. capped   4. rounds exhausted   5. the interval rule of batotp_hip_stretch.h
 *    *out: bit for bit batotp_hip_output_torques(batotp_hip_output_stretch_to(o, report.n_out)).  scale and duty may be NULL.
 *    With ratings that never bind, report and scale are those of batotp_hip_output_stretch_torques byte for byte.
 * BATOTP_ERR_ARG as above, and for everything batotp_hip_output_stretch_torques refuses. */
int batotp_hip_output_stretch_duty(batotp_output *o, const batotp_problem *prob, const batotp_serial_model *model, uint32_t flags,
                                   const double *rated, double target, int32_t max_rounds, double max_factor, batotp_output **out,
                                   batotp_path_stretch *report, batotp_path_tscale *scale, batotp_path_duty *duty);
/* HIP-event milliseconds of the kernels of this header in the call that made out (all rounds and ranges); BATOTP_ERR_STATE if
 * out was not made by one of the two calls above */
int batotp_hip_output_duty_ms(batotp_output *out, float *ms);
/* launches of the duty kernel (ranges of paths, summed over the rounds) of that call; BATOTP_ERR_STATE as above */
int batotp_hip_output_duty_ranges(batotp_output *out, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* BATOTP_HIP_DUTY_H */
