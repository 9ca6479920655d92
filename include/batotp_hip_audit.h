/*
 * batotp_hip_audit.h -- audit of finished trajectories against their limits, on the device.
 *
 * A batotp_output (include/batotp_hip.h: batotp_hip_output) holds the constant-time trajectories a controller receives: the
 * integrated curve resampled in time, smoothed, down-sampled and possibly re-interpolated (reference batotp/ba.cpp:1668-1931).
 * The audit answers, without the rows leaving HBM, whether those published samples respect the limits of the problem and how
 * close they come to them: one streaming pass over the rows, one batotp_path_audit per path back.  It is deliberately an audit
 * of the SAMPLES (finite differences), not of the splines behind them.
 *
 * ---- definition (the tests pin it bit for bit; DESIGN.md 4 restates it) ----------------------------------------------------
 * One path of the output: rows x_r[i], i = 0..n-1, in the stage's own order -- n_theta joint rows, then n_cart Cartesian rows,
 * then n_trq torque rows; h = the path's sres (batotp_hip_output_info).
 *
 * All arithmetic is binary64, in exactly the order written, without contraction.  Every reciprocal is formed ONCE ON THE HOST
 * with a plain `/`; the kernel only subtracts, multiplies, takes fabs, takes sqrt and compares:
 *    c1 = 1.0 / (2.0*h)            c2 = 1.0 / (h*h)
 *    rv_j = 1.0 / jnt_vel_max[j]   ra_j = 1.0 / jnt_acc_max[j]
 *    rcv = 1.0 / cart_vel_max      rca = 1.0 / cart_acc_max
 *    mid_r = (jnt_trq_max[r] + jnt_trq_min[r]) * 0.5    half_r = (jnt_trq_max[r] - jnt_trq_min[r]) * 0.5    rt_r = 1.0 / half_r
 *
 * At the interior points i = 1..n-2:
 *    v_r[i] = (x_r[i+1] - x_r[i-1]) * c1
 *    a_r[i] = ((x_r[i+1] - x_r[i]) - (x_r[i] - x_r[i-1])) * c2
 *
 * Families and their utilisations u (u <= 1: within the limit):
 *    JNT_VEL    interior points, joint rows      fabs(v_j[i]) * rv_j
 *    JNT_ACC    interior points, joint rows      fabs(a_j[i]) * ra_j
 *    CART_VEL   interior points                  sqrt((vx*vx + vy*vy) + vz*vz) * rcv
 *    CART_ACC   interior points                  the same with a and rca
 *    TRQ        EVERY point 0..n-1, torque rows  fabs(x_r[i] - mid_r) * rt_r
 * The Cartesian families use the position rows: the first min(3, n_cart) Cartesian rows (what evalCartQuadCoeffs, reference
 * batotp/ba.cpp:1423-1439, reads); terms of rows that do not exist are left out.
 *
 * JNT_VEL is always audited (the reference keeps joint-velocity limits always on); JNT_ACC, CART_VEL, CART_ACC and TRQ are
 * audited when the corresponding BATOTP_F_* flag of the batotp_problem is set AND the output has the rows.  An audited family
 * whose limit is not finite and positive (torque: half_r) is BATOTP_ERR_ARG.
 *
 * Per family: `peak` = the maximum utilisation, `at` = the output point of the peak, `row` = the row inside the family (joint
 * j, torque row r, 0 for the Cartesian families).  Ties go to the LOWEST point index, then the LOWEST row -- the rule that makes
 * the result independent of how the reduction is split.  A family that was not audited, or that has no point to evaluate
 * (n < 3 for the difference families, n = 0 for torque, no finite utilisation at all), has peak = -1.0, at = row = -1.
 *
 * n_over = the number of points at which ANY audited utilisation is > 1.0 + tol (strict; 1.0 + tol is formed once on the host).
 * n_nonfinite = the number of row values (of all rows) that are NaN or +-Inf.  A utilisation that is not finite takes no part
 * in the peaks or in n_over: the count is how a NaN trajectory is reported instead of passing as "peak 0.3".
 * A path with n_pts = 0 (failed sweep) gets every family at -1 and every count 0.
 */
#ifndef BATOTP_HIP_AUDIT_H
#define BATOTP_HIP_AUDIT_H

#include "batotp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A path is cut into blocks of this many points (one workgroup each, a halo of one point on each side); public so that tests
 * can aim at the block boundaries.  The result does not depend on it. */
#define BATOTP_AUDIT_BLOCK_POINTS 1024

#define BATOTP_AUDIT_JNT_VEL  0
#define BATOTP_AUDIT_JNT_ACC  1
#define BATOTP_AUDIT_CART_VEL 2
#define BATOTP_AUDIT_CART_ACC 3
#define BATOTP_AUDIT_TRQ      4
#define BATOTP_AUDIT_FAMILIES 5

typedef struct batotp_audit_peak {
    double  peak;      /* maximum utilisation of the family, -1.0 if there is none     */
    int64_t at;        /* output point of the peak, -1 if there is none                */
    int32_t row;       /* row inside the family, -1 if there is none                   */
    int32_t reserved;  /* 0                                                            */
} batotp_audit_peak;

typedef struct batotp_path_audit {
    batotp_audit_peak fam[BATOTP_AUDIT_FAMILIES];  /* indexed by BATOTP_AUDIT_*        */
    int64_t n_pts;         /* points of the path                                       */
    int64_t n_over;        /* points with an audited utilisation > 1.0 + tol           */
    int64_t n_nonfinite;   /* row values that are NaN or +-Inf                         */
} batotp_path_audit;

/* Audit every path of o against the limits of prob (the batotp_problem the batch was created with, or any other with the same
 * n_joints); out[n_paths of o] on the host.  BATOTP_ERR_ARG -- nothing touched -- for NULLs, a tol that is negative or not
 * finite, prob->n_joints != the output's joint rows, more torque rows than the problem has (n_cart rows of a parallel
 * mechanism, n_joints otherwise) and an audited family with a limit that is not finite and positive.  Work space comes from
 * the context's workspace (the output stage's scratch). */
int batotp_hip_output_audit(batotp_output *o, const batotp_problem *prob, double tol, batotp_path_audit *out);
/* the same with the rows left on the device: out_dev = DEVICE memory for n_paths batotp_path_audit (for gathers) */
int batotp_hip_output_audit_device(batotp_output *o, const batotp_problem *prob, double tol, void *out_dev);
/* milliseconds of the two kernels of the last audit of o (HIP events on the context's stream); BATOTP_ERR_STATE before one */
int batotp_hip_output_audit_ms(batotp_output *o, float *ms);
/* A genuine batotp_output from trajectories the caller supplies: rows on the host, path after path, each
 * [n_theta + n_cart + n_trq][n_pts[k]]; sres[k] = the time step of path k.  Every accessor of batotp_hip.h and
 * batotp_hip_output_destroy work on it.  This is how trajectories computed elsewhere are audited.  BATOTP_ERR_ARG for NULLs,
 * negative counts, row counts outside 0..BATOTP_MAX_JOINTS / 0..BATOTP_MAX_CART / 0..BATOTP_MAX_JOINTS or no row at all, and
 * a step of a path with points that is not finite and positive. */
int batotp_hip_output_from_rows(batotp_ctx *ctx, int32_t n_paths, const int64_t *n_pts, const double *sres,
                                int32_t n_theta, int32_t n_cart, int32_t n_trq, const double *rows, batotp_output **out);

#ifdef __cplusplus
}
#endif
#endif /* BATOTP_HIP_AUDIT_H */
