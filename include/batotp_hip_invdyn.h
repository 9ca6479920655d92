/*
 * batotp_hip_invdyn.h -- torque rows for finished trajectories: inverse dynamics of a serial chain on the device.
 *
 * The fast kernels of this library plan under joint velocity and acceleration limits only.  This header answers, for such a
 * batotp_output (or one brought in with batotp_hip_output_from_rows, include/batotp_hip_audit.h), what the motors have to
 * deliver along the published samples: the torques of a batotp_serial_model at every output point, appended to the rows as
 * n_links torque rows, without the rows leaving HBM.  The result is a batotp_output like any other; the TRQ family of
 * batotp_hip_output_audit reads its torque rows, and a controller takes them as feed-forward next to the positions.
 *
 * ---- definition (the tests pin it bit for bit; DESIGN.md 4 and 4d restate it) -------------------------------------------------
 * This definition is the library's own: the reference has no counterpart.
 *
 * One path of the output: joint rows x_j[i], j = 0..n_links-1, i = 0..n-1; h = the path's sres (batotp_hip_output_info).
 * All arithmetic is binary64, in exactly the order written, without contraction.
 *
 * Finite differences -- exactly the audit's (batotp_hip_audit.h), so the two cannot disagree about a velocity:
 *    c1 = 1.0 / (2.0*h)            c2 = 1.0 / (h*h)            (formed once on the host)
 *    v_j[k] = (x_j[k+1] - x_j[k-1]) * c1
 *    a_j[k] = ((x_j[k+1] - x_j[k]) - (x_j[k] - x_j[k-1])) * c2
 *
 * Index rule: point i takes the differences at ic = min(max(i, 1), n-2) -- the two end points those of their interior
 * neighbour.  A path of n < 3 points has v = a = +0.0 at every point.
 *
 * Scaled values: unit = _DEG2RAD (3.14159265358979323846 / 180.0) if model->degrees, else 1.0;
 *    q_j = unit * x_j[i]        qd_j = unit * v_j[ic]        qdd_j = unit * a_j[ic]
 *
 * Trig: c_j = cos(q_j), s_j = sin(q_j) at the point i itself.  With BATOTP_F_HOST_TRIG they are the host libm's cos() and
 * sin(), called separately (tables made on the host); without the flag the device libm is used, which agrees with the host's
 * to rounding only (the tolerance mode of DESIGN.md 2).
 *
 * Torque: two passes of the recursive Newton-Euler recursion of the chain model (rnea_pass, the function behind
 * batotp_hip_set_serial_model; its CPU twin is bo_rnea of the oracle):
 *    t2 = rnea(model, c, s, qd, qdd, base acceleration (0, 0, 0))
 *    t4 = rnea(model, c, s, 0,  0,   base acceleration -gravity)
 *    tau_j = (t2_j + model->link[j].fv * qd_j) + t4_j
 * i.e. a2 + a3 + a4 of the chain's dynamics coefficients for (q, q' = dq/dt, q'' = d2q/dt2): the torque at sdot = 1,
 * sddot = 0 with time as the path parameter.  A single pass with gravity folded in gives other bits and is not the definition.
 *
 * Values that are not finite propagate: a NaN joint value makes the torques of the points whose differences or angles read it
 * NaN, and the audit's n_nonfinite then counts them.
 */
#ifndef BATOTP_HIP_INVDYN_H
#define BATOTP_HIP_INVDYN_H

#include "batotp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A path is cut into blocks of this many points (one workgroup each, one lane per point); public so that tests can aim at the
 * block boundaries.  The result does not depend on it. */
#define BATOTP_INVDYN_BLOCK_POINTS 128

/* A NEW output: the joint and Cartesian rows of o copied bit for bit, followed by model->n_links torque rows (every path
 * [n_theta + n_cart + n_links][n_pts]).  n_pts and sres are those of o, and o is left untouched.  Every accessor of
 * batotp_hip.h, batotp_hip_output_destroy and batotp_hip_output_audit work on the result; batotp_hip_output_channels reports
 * (n_theta, n_cart, n_links).  An output without paths or without points gives a valid empty result.
 * flags: only BATOTP_F_HOST_TRIG is read (see above).
 * BATOTP_ERR_ARG with a message (batotp_hip_last_error), *out = NULL, nothing launched or allocated: a NULL argument,
 * model->n_links outside 1..BATOTP_MAX_LINKS or different from the joint rows of o, an o that already has torque rows, a
 * model entry (gravity, axis, off, com, mass, inertia, fv of a link in use) that is not finite, a joint axis a with
 * | |a|^2 - 1 | > 1e-12, a flag other than BATOTP_F_HOST_TRIG.
 * Work space comes from the context's output workspace; when the tables of the whole output exceed the budget of
 * batotp_hip_set_workspace_budget (output_bytes), ranges of paths are processed one after another.  The result does not
 * depend on the cut. */
int batotp_hip_output_torques(batotp_output *o, const batotp_serial_model *model, uint32_t flags, batotp_output **out);
/* HIP-event milliseconds of the torque kernel(s) of that call, summed over its ranges; BATOTP_ERR_STATE if out was not made
 * by batotp_hip_output_torques */
int batotp_hip_output_torques_ms(batotp_output *out, float *ms);
/* the number of ranges of paths that call was cut into (0 for a result without points); BATOTP_ERR_STATE as above */
int batotp_hip_output_torques_ranges(batotp_output *out, int32_t *n_ranges);

#ifdef __cplusplus
}
#endif
#endif /* BATOTP_HIP_INVDYN_H */
