/*
 * batotp_hip_tscale.h -- stretch finished trajectories until their TORQUE limits pass: dynamic time scaling on the device.
 *
 * The stretch (batotp_hip_stretch.h) brings the velocity and acceleration families of the audit inside their limits; the torque
 * rows (batotp_hip_invdyn.h) say what the motors have to deliver.  This header closes the chain: under a uniform dilation of
 * time by k the torque of a rigid chain at a path point is
 *       A / k^2 + B / k + G          (Hollerbach's dynamic time scaling)
 * with A the inertial plus velocity-product part, B the viscous friction and G gravity -- the three addends the torque kernel
 * forms anyway.  Keeping them apart gives, in the one pass that makes the torque rows, the speed factor x = 1/k every path
 * admits, and the rounds below stretch every path by its own factor until the TRQ family of the audit passes too.
 *
 * ---- definition (the tests pin it bit for bit; DESIGN.md 4 and tests/tscale_reference.py restate it) -------------------------
 * This definition is the library's own: the reference has no counterpart.
 * All arithmetic is binary64, in exactly the order written, without contraction; `/` and sqrt are the correctly rounded ones.
 *
 * Per point i of a path: q, qd, qdd, c, s, t2, t4 are EXACTLY those of batotp_hip_invdyn.h (the same differences, index rule,
 * trig policy, two passes of the recursion).  The three addends are kept apart:
 *       A_j = t2_j          B_j = model->link[j].fv * qd_j          G_j = t4_j
 * and the torque row is still (A_j + B_j) + G_j.
 *
 * Bounds, formed once on the host: mid_j = (trq_max_j + trq_min_j) * 0.5 and half_j = (trq_max_j - trq_min_j) * 0.5 as in the
 * audit;  hi_j = mid_j + target*half_j;  lo_j = mid_j - target*half_j.
 *
 * Static points: point i is STATIC if for some joint  !(G_j - hi_j < 0 && lo_j - G_j < 0)  -- gravity alone is not strictly
 * inside the range there, and no dilation helps.  A NaN in G makes the point static.
 *
 * Candidates, at a point that is not static, per joint and side:
 *       upper bound (side +1):  (a, b, c) = ( A_j,  B_j, G_j - hi_j)
 *       lower bound (side -1):  (a, b, c) = (-A_j, -B_j, lo_j - G_j)          (c < 0 in both)
 *       disc = b*b - (4.0*a)*c          q = b + sqrt(disc)          x = (2.0*(-c)) / q
 * The candidate exists iff disc >= 0 && q > 0; a candidate whose disc, q or x is not finite takes no part.  x is the smallest
 * positive root of a x^2 + b x + c, whatever the sign of a (a = 0: the root of the line, if it rises).
 *
 * Reduction over the path: s = the minimum candidate over points, joints and sides; ties go to the lowest point, then the
 * lowest joint, then the upper side before the lower.  No candidate: s = +Inf, at = row = -1, side = 0.  Every x in (0, s]
 * satisfies every bound at every point that is not static: the SMALLEST root is taken so that "slower is also admissible" holds.
 * n_static counts the static points.  A path of fewer than 3 points has A = B = 0 and no candidate: it passes iff gravity is
 * inside the range.
 */
#ifndef BATOTP_HIP_TSCALE_H
#define BATOTP_HIP_TSCALE_H

#include "batotp_hip_stretch.h"
#include "batotp_hip_invdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A path is cut into blocks of this many points (one workgroup each, one lane per point); public so that tests can aim at the
 * block boundaries.  The result does not depend on it. */
#define BATOTP_TSCALE_BLOCK_POINTS 128
/* a fourth status of batotp_path_stretch: gravity alone leaves the torque range somewhere on the path -- no stretch helps */
#define BATOTP_STRETCH_STATIC 3

typedef struct batotp_path_tscale {   /* 40 bytes */
    double  s;         /* largest admissible speed factor x = 1/k predicted from the rows: the smallest root, +Inf if there is none */
    int64_t at;        /* point of that root, -1 if none                                                                  */
    int32_t row;       /* joint of that root, -1 if none                                                                  */
    int32_t side;      /* +1 upper bound, -1 lower bound, 0 if none                                                       */
    int64_t n_static;  /* points at which some joint's gravity torque is not strictly inside its range                    */
    int64_t reserved;  /* 0                                                                                               */
} batotp_path_tscale;

/* The known-answer entry.  A NEW output: the rows of o followed by model->n_links torque rows, bit for bit those of
 * batotp_hip_output_torques(o, model, flags), AND one record per path in scale[n_paths] (host; may be NULL only for an output
 * without paths).  The torque range is prob's jnt_trq_max / jnt_trq_min, whether or not BATOTP_F_TRQ_ON is set.
 * BATOTP_ERR_ARG with a message (batotp_hip_last_error), *out = NULL, nothing launched: everything batotp_hip_output_torques
 * and batotp_hip_output_audit refuse for these arguments, a problem of a parallel mechanism, a torque range of a joint in use
 * that is not finite and positive, a target outside (0, 1], an o that has torque rows.
 * Ranges of paths under batotp_hip_set_workspace_budget as batotp_hip_output_torques cuts them; nothing depends on the cut. */
int batotp_hip_output_torque_scale(batotp_output *o, const batotp_problem *prob, const batotp_serial_model *model,
                                   uint32_t flags, double target, batotp_output **out, batotp_path_tscale *scale);
/* The rounds: batotp_hip_output_stretch_audit with the torque family on top.
 *    Every round works on the current rows (the rows of o, then always rows stretched FROM the rows of o): it makes their
 *    torque rows and scale records (above), and audits the result on the device at tol 0 against a copy of prob that has
 *    BATOTP_F_TRQ_ON set.  (ok, need) follow from JNT_VEL, JNT_ACC, CART_VEL, CART_ACC by the rule of
 *    batotp_hip_output_stretch_audit; call that ok kin_ok.  Then
 *       trq_ok = the TRQ peak is <= target or is -1
 *       if !trq_ok:  ok = false, and if n_static == 0 && s < 1.0:  need = max(need, 1.0 / s)
 *    and the path's outcome is decided in this order:
 *       1. ok:                                   BATOTP_STRETCH_PASSES
 *       2. !trq_ok && n_static > 0 && kin_ok:    BATOTP_STRETCH_STATIC -- the path is not stretched again
 *       3. the path is capped:                   BATOTP_STRETCH_CAPPED
 *       4. rounds >= max_rounds:                 BATOTP_STRETCH_ROUNDS
 *       5. otherwise the interval rule of batotp_hip_stretch.h (want, max(.., m+1), bound, cap) gives its new point count.
 *    report[n_paths] (host): the stretch's struct.  scale[n_paths] (host, may be NULL): the records of the final rows.
 *    *out: the stretched rows followed by n_links torque rows -- bit for bit what batotp_hip_output_torques gives for
 *    batotp_hip_output_stretch_to(o, report.n_out).
 * BATOTP_ERR_ARG as above, and for everything batotp_hip_output_stretch_audit refuses.  No row leaves HBM except the packed
 * joint rows of BATOTP_F_HOST_TRIG; the records come back in one small copy per round. */
int batotp_hip_output_stretch_torques(batotp_output *o, const batotp_problem *prob, const batotp_serial_model *model,
                                      uint32_t flags, double target, int32_t max_rounds, double max_factor,
                                      batotp_output **out, batotp_path_stretch *report, batotp_path_tscale *scale);
/* HIP-event milliseconds of the kernels of this header in the call that made out (all rounds and ranges; the stretch kernels
 * and the audits are not counted); BATOTP_ERR_STATE if out was not made by one of the two calls above */
int batotp_hip_output_tscale_ms(batotp_output *out, float *ms);
/* launches of the scale kernel (ranges of paths, summed over the rounds) of that call; BATOTP_ERR_STATE as above */
int batotp_hip_output_tscale_ranges(batotp_output *out, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* BATOTP_HIP_TSCALE_H */
