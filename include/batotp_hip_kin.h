/*
 * batotp_hip_kin.h -- the tool point of a serial arm from its kinematic chain, on the device.
 *
 * The reference computes a tool point for two robots only (Robot::fwdKinKuka, Robot::fwdKinRR, batotp/robot.cpp:105-202), so a
 * path taught in joint space can carry a Cartesian speed or acceleration limit on those two alone.  A batotp_kin_chain describes
 * any chain of revolute joints the way batotp_serial_model (include/batotp_hip.h) does -- joint axes and joint-origin offsets in
 * zero-aligned frames -- plus the tool point, and the entry points below use it wherever the two closed forms are used: in the
 * resampler (batotp_hip_resample_chain) and in the output stage (batotp_hip_set_kin_chain).  include/batotp_hip.h is unchanged;
 * without a chain every configuration behaves as before.
 *
 * ---- definition (this project's own; the tests pin it bit for bit; DESIGN.md 4 restates it) -----------------------------------
 * The chain has `n` links.
 *    axis_i  is a unit vector.
 *    off_i   is the joint origin relative to the parent's joint origin.
 *    tool    is the tool point relative to the last joint origin.
 * All three are in the coordinates of the zero configuration, in which every frame coincides with the base.  This is the
 * convention of batotp_serial_model.
 *
 * Trigonometry: q_i = unit * theta_i, unit = _DEG2RAD (3.14159265358979323846 / 180.0) if `degrees` is set, else 1.
 * c_i = cos(q_i) and s_i = sin(q_i) are separate libm calls.
 *
 * Arithmetic is binary64 in the order written, no contraction:
 *
 *    p = tool
 *    for i = n-1 ... 0:
 *       a = axis_i
 *       d  = (a0*p0 + a1*p1) + a2*p2
 *       x0 = a1*p2 - a2*p1;  x1 = a2*p0 - a0*p2;  x2 = a0*p1 - a1*p0
 *       k  = d*(1.0 - c_i)
 *       p_j = off_i[j] + ((p_j*c_i + x_j*s_i) + a_j*k)        j = 0,1,2, from the old p
 *    Cartesian rows 0..2 of the point = p
 *
 * With BATOTP_F_HOST_TRIG, c_i and s_i come from host tables, laid out as the chain model's tables of the dynamics are
 * (batotp_hip_upload_joint_trig): rows cos q_0 ... cos q_{n-1}, then the sines.  Results then equal the host twin
 * (Robot::chainToolPoint) and the Python restatement (tests/kin_reference.py) bit for bit.  Without the flag the device libm is
 * used: the documented tolerance mode of DESIGN.md 2.
 */
#ifndef BATOTP_HIP_KIN_H
#define BATOTP_HIP_KIN_H

#include "batotp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct batotp_kin_chain {
    int32_t n_links;                     /* 1 .. BATOTP_MAX_LINKS                                     */
    int32_t degrees;                     /* joint values are degrees: scaled by _DEG2RAD first        */
    double  axis[BATOTP_MAX_LINKS][3];   /* joint axes, unit vectors                                  */
    double  off[BATOTP_MAX_LINKS][3];    /* joint origin relative to the parent's joint origin        */
    double  tool[3];                     /* tool point relative to the last joint origin              */
} batotp_kin_chain;

/* Every entry point that takes a chain checks it first and returns BATOTP_ERR_ARG with a message, without launching anything, for
 * n_links outside 1..BATOTP_MAX_LINKS, an entry of the used links or of the tool point that is not finite, and an axis with
 * | |a|^2 - 1 | > 1e-12. */

/* axes and offsets of a dynamics model plus a tool point */
int batotp_hip_kin_chain_from_model(const batotp_serial_model *model, const double tool[3], batotp_kin_chain *out);
/* the built-in chain of a robot type (include/batotp_models.h), all three in degrees: BATOTP_ROBOT_KUKA = LWR IV+ with the tool
 * point of Robot::fwdKinKuka, BATOTP_ROBOT_RR = the two-link arm of Robot::fwdKinRR, BATOTP_ROBOT_UR = a nominal UR5;
 * BATOTP_ERR_ARG if none */
int batotp_hip_builtin_kin_chain(int32_t robot_type, batotp_kin_chain *out);

/* Known-answer entry: the tool points of a ragged set of point lists.  theta is [n_links][n_pts[p]] per path, path after path;
 * cart_out is [3][n_pts[p]] laid out likewise (both on the host).  BATOTP_F_HOST_TRIG in `flags` selects the host tables.  It runs
 * the device function and the kernel shape of the resampler's call: one lane per point, the path found by binary search. */
int batotp_hip_fwdkin_chain(batotp_ctx *ctx, const batotp_kin_chain *chain, uint32_t flags, int32_t n_paths, const int64_t *n_pts,
                            const double *theta, double *cart_out);

/* batotp_hip_resample with the chain as the kinematics: the tool point of the taught points when a Cartesian limit is on, and of
 * the points each of the two passes leaves (reference batotp/ba.cpp:247-256, 626-628).  Requires path_type == BATOTP_PATH_JOINT,
 * n_cart == 3 and chain->n_links == n_joints (BATOTP_ERR_ARG with a message otherwise); robot_type is not consulted for the
 * kinematics.  The Cartesian rows of x are ignored.  Everything else is batotp_hip_resample's own code, and the result is an
 * ordinary batotp_resampled. */
int batotp_hip_resample_chain(batotp_ctx *ctx, const batotp_resample_params *prm, const batotp_kin_chain *chain, int32_t n_paths,
                              const int64_t *n_in, const double *x, const double *sres_in, batotp_resampled **out);

/* The chain of a batch, used by batotp_hip_output: with it a JOINT path of ANY robot type gets three Cartesian rows, the tool
 * point at the output points (reference ba.cpp:1722-1725), from the chain instead of a closed form.  Needs n_links == n_joints
 * and a batch with at least 3 Cartesian channels.  The sweeps need nothing: their Cartesian limits read the splines of the
 * Cartesian channels, whatever produced them. */
int batotp_hip_set_kin_chain(batotp_batch *batch, const batotp_kin_chain *chain);

#ifdef __cplusplus
}
#endif
#endif /* BATOTP_HIP_KIN_H */
