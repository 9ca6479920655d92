/*
 * batotp_hip_stretch.h -- uniform dilation of time for finished trajectories, on the device.
 *
 * The audit (batotp_hip_audit.h) says how far the published samples of a batotp_output exceed their limits; this header is the
 * remedy.  The same geometric path is sampled with the same time step h over a longer duration: velocities fall as 1/k and
 * accelerations as 1/k^2.  Three uses are one primitive: a given point count (several trajectories brought to a common
 * duration), a given factor (a speed override), and "until the audit passes".  The work is one streaming pass over rows that
 * already lie in HBM; the result is a batotp_output like any other.
 *
 * ---- definition (the tests pin it bit for bit; DESIGN.md 4 and tests/stretch_reference.py restate it) ----------------------
 * This definition is the library's own: the reference has no counterpart.
 *
 * One path of the output: rows x_r[i], i = 0..n-1, time step h.  The result has n2 >= n points at the same h.  Every row,
 * joint and Cartesian, is treated alike and component-wise: ORIENTATION ROWS (the quaternion of a pose path) ARE INTERPOLATED
 * AS PLAIN NUMBERS and are not renormalised.
 *
 * All arithmetic is binary64, in exactly the order written, without contraction.
 *    A path with n2 == n, or with n < 2, is copied bit for bit (n < 2: n2 = n always).
 *    Otherwise  rk = (double)(n-1) / (double)(n2-1), formed ONCE ON THE HOST with a plain `/`, and for p = 0..n2-2:
 *       u = (double)p * rk          j = min((int64)u, n-2)          f = u - (double)j
 *       d  = x[j+1] - x[j]
 *       m0 = (x[j+1] - x[j-1]) * 0.5   if j >= 1,      else d
 *       m1 = (x[j+2] - x[j]) * 0.5     if j+2 <= n-1,  else d
 *       c2 = (3.0*d - 2.0*m0) - m1
 *       c3 = (m0 + m1) - 2.0*d
 *       y[p] = x[j] + f*(m0 + f*(c2 + f*c3))
 *    and y[n2-1] = x[n-1], taken by rule and not by arithmetic.
 *
 * This is the Catmull-Rom Hermite cubic through the source points: it is C1, and y[0] = x[0] exactly (f = 0).  On a cell its
 * second derivative runs linearly from 2 D_j - D_{j+1} to 2 D_{j+1} - D_j, where D_i are the second differences of the source
 * (on the two end cells, whose outer tangent is one-sided, from -D to 2 D of the neighbouring point).
 * After a stretch by k the finite-difference acceleration of the result is therefore AT MOST 3 (old peak) / k^2, and about
 * (old peak) / k^2 on smooth data.  That is why the audit mode below needs rounds -- one stretch by sqrt(peak) need not be
 * enough -- and why the rounds end: every round multiplies the bound by less than one.
 *
 * Values that are not finite propagate through whatever stencil reads them (0 * Inf is NaN, as IEEE has it); the payload and
 * the sign of a NaN are not part of the definition.
 */
#ifndef BATOTP_HIP_STRETCH_H
#define BATOTP_HIP_STRETCH_H

#include "batotp_hip_audit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The NEW points of a path are cut into blocks of this many (one workgroup each, one lane per new point); public so that
 * tests can aim at the block boundaries.  The result does not depend on it. */
#define BATOTP_STRETCH_BLOCK_POINTS 256
/* no path is stretched beyond this many points (the bound of batotp_hip_output_from_rows) */
#define BATOTP_STRETCH_MAX_POINTS ((int64_t)1 << 40)

#define BATOTP_STRETCH_PASSES    0   /* every audited family of the path is within the target                         */
#define BATOTP_STRETCH_ROUNDS    1   /* stretched max_rounds times and still over the target                          */
#define BATOTP_STRETCH_CAPPED    2   /* stretched to the bound of max_factor and still over the target                */

typedef struct batotp_path_stretch {
    int64_t n_in;      /* points of the path in o                                                                      */
    int64_t n_out;     /* points of the path in the result                                                             */
    double  factor;    /* (double)(n_out-1) / (double)(n_in-1); 1.0 for n_in < 2                                       */
    int32_t rounds;    /* how many times the path was stretched (each time from the rows of o)                         */
    int32_t status;    /* BATOTP_STRETCH_*                                                                             */
} batotp_path_stretch;

/* A NEW output with n_out[k] points for path k of o; row counts and sres are those of o, and o is left untouched.  Every
 * accessor of batotp_hip.h, batotp_hip_output_destroy, batotp_hip_output_audit and batotp_hip_output_torques work on the
 * result.  An output without paths or without points gives a valid empty result.
 * BATOTP_ERR_ARG with a message (batotp_hip_last_error), *out = NULL, nothing launched or allocated: a NULL argument; an o
 * that has TORQUE ROWS (torques are no function of the path alone: stretch first, then call batotp_hip_output_torques on the
 * result); n_out[k] < the points of path k, or > BATOTP_STRETCH_MAX_POINTS; n_out[k] != the points of a path with fewer than
 * two.
 * Work space comes from the context's output workspace; when the descriptor tables of the whole result exceed the budget of
 * batotp_hip_set_workspace_budget (output_bytes), ranges of paths are processed one after another.  The result does not
 * depend on the cut. */
int batotp_hip_output_stretch_to(batotp_output *o, const int64_t *n_out, batotp_output **out);
/* the same with n_out[k] = (int64)ceil((double)(n-1) * factor[k]) + 1 (n_out[k] = n for n < 2); a factor that is not finite
 * or < 1 is BATOTP_ERR_ARG as above */
int batotp_hip_output_stretch_by(batotp_output *o, const double *factor, batotp_output **out);
/* Stretch every path of o, each by its own factor, until its audit against prob passes.
 *    target in (0, 1]: the utilisation every audited family has to come down to; max_rounds in 1..16; max_factor >= 1, finite.
 *    Round 0 audits o on the device (tol 0).  A path PASSES when each of JNT_VEL, JNT_ACC, CART_VEL, CART_ACC has its peak
 *    <= target or is -1 (not audited, or nothing to evaluate); TRQ takes no part.  For a path that does not pass:
 *       need = 1.0;  velocity families: need = max(need, peak / target);  acceleration families: need = max(need, sqrt(peak / target))
 *       m = the intervals of the path's current result (n_in - 1 before the first stretch)
 *       want = ceil((double)m * need);  intervals = max(want, (double)(m+1))
 *       bound = min(floor((double)(n_in-1) * max_factor), (double)(BATOTP_STRETCH_MAX_POINTS - 1))
 *       if intervals > bound: intervals = bound, and the path is capped -- it is stretched to the bound (if that is more
 *       points than it has) and not again
 *       n2 = (int64)intervals + 1
 *    Every round stretches FROM THE ROWS OF o to the current n2 -- a stretched result is never stretched again -- and the
 *    result is audited again; paths that pass keep their n2.  It ends when every path passes, is capped, or has been
 *    stretched max_rounds times.
 *    report[n_paths] (host, may not be NULL): see batotp_path_stretch; the status is that of the final audit -- PASSES
 *    whenever the rows of the result pass, else CAPPED for a capped path, else ROUNDS.
 * The audit records come back through batotp_hip_output_audit_device and one small copy per round: no row leaves HBM.
 * BATOTP_ERR_ARG as batotp_hip_output_stretch_to, and for everything batotp_hip_output_audit refuses, and for target,
 * max_rounds or max_factor outside the ranges above. */
int batotp_hip_output_stretch_audit(batotp_output *o, const batotp_problem *prob, double target, int32_t max_rounds,
                                    double max_factor, batotp_output **out, batotp_path_stretch *report);
/* HIP-event milliseconds of the stretch kernels of the call that made out (all rounds and ranges);
 * BATOTP_ERR_STATE if out was not made by one of the three calls above */
int batotp_hip_output_stretch_ms(batotp_output *out, float *ms);
/* the number of kernel launches (ranges of paths, summed over the rounds) of that call; BATOTP_ERR_STATE as above */
int batotp_hip_output_stretch_ranges(batotp_output *out, int32_t *n_ranges);

#ifdef __cplusplus
}
#endif
#endif /* BATOTP_HIP_STRETCH_H */
