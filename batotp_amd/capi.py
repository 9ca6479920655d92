"""ctypes binding of the C-ABI in include/batotp_hip.h.

The product library is ``batotp_amd/csrc/libbatotp_hip.so`` (HIP kernels for gfx950); ``load_hip`` raises
if it is missing and ``Context`` raises if no GPU is usable -- there is no fallback.  ``Library`` binds any
shared object that exports the same entry points; the test-suite uses that to put its CPU checker behind
the same classes (``tests/helpers.load_oracle``) -- nothing in this package knows where that checker lives.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
HIP_LIB_PATH = os.path.join(_HERE, "csrc", "libbatotp_hip.so")

MAX_JOINTS = 8
MAX_CART = 8

# robot ids (reference batotp/robot.h:33-37)
ROBOT_KUKA, ROBOT_UR, ROBOT_RR, ROBOT_CSPR3DOF, ROBOT_GENJNT = 1, 2, 3, 4, 5
# problem flags
F_JNT_ACC_ON, F_TRQ_ON, F_CART_VEL_ON, F_CART_ACC_ON = 1 << 0, 1 << 1, 1 << 2, 1 << 3
F_PARALLEL, F_PAR2SER, F_HOST_TRIG, F_NO_SAMPLES, F_COMPACT_SPLINES = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8
F_CURVES_IN_PLACE = 1 << 9  # the forward curve overwrites the reverse curve (one curve buffer per path)
F_MVC_IN_CURVES = 1 << 10   # the pointwise evaluation writes into the curve buffers (valid until a sweep starts)
F_SVD = 1 << 11             # solveLinSys by Jacobi SVD instead of LU (_isSVD)
# per-path status bits
ST_MAX_INTEG_TIME, ST_CAPACITY, ST_BISECT_FAIL = 1 << 0, 1 << 1, 1 << 2
ST_NONFINITE, ST_SHORT, ST_SEG_ERROR = 1 << 3, 1 << 4, 1 << 5

# path kinds / status bits of the resampler
PATH_JOINT, PATH_CART, PATH_BOTH = 1, 2, 3
RS_TOO_SHORT, RS_IDENTICAL, RS_CAPACITY, RS_SMALL_STEP, RS_SEG_ERROR = 1, 2, 4, 8, 16
# OutputParams.integ_res: every path of the range is sampled with its own step (BATOTP_OUT_STEP_PER_PATH)
OUT_STEP_PER_PATH = 0.0

_d8 = C.c_double * 8


class Problem(C.Structure):
    """struct batotp_problem"""

    _fields_ = [
        ("n_joints", C.c_int32),
        ("n_cart", C.c_int32),
        ("robot_type", C.c_int32),
        ("flags", C.c_uint32),
        ("jnt_vel_max", _d8),
        ("jnt_acc_max", _d8),
        ("jnt_trq_max", _d8),
        ("jnt_trq_min", _d8),
        ("cart_vel_max", C.c_double),
        ("cart_acc_max", C.c_double),
        ("jnt_thresh", C.c_double),
        ("quad_rad_thresh", C.c_double),
        ("integ_res", C.c_double),
        ("max_integ_time", C.c_double),
        ("pmat", C.c_double * 9),
    ]

    @property
    def dyn_dim(self) -> int:
        if not (self.flags & F_TRQ_ON):
            return 0
        return self.n_cart if (self.flags & F_PARALLEL) else self.n_joints

    @property
    def n_channels(self) -> int:
        return self.n_joints + self.n_cart + 4 * self.dyn_dim


class SerialLink(C.Structure):
    """struct batotp_serial_link"""
    _fields_ = [("axis", C.c_double * 3), ("off", C.c_double * 3), ("com", C.c_double * 3), ("mass", C.c_double),
                ("inertia", C.c_double * 6), ("fv", C.c_double)]


class SerialModel(C.Structure):
    """struct batotp_serial_model"""
    _fields_ = [("n_links", C.c_int32), ("degrees", C.c_int32), ("gravity", C.c_double * 3), ("link", SerialLink * 8)]


class KinChain(C.Structure):
    """struct batotp_kin_chain (include/batotp_hip_kin.h): joint axes, joint-origin offsets and the tool point of a serial arm"""
    _fields_ = [("n_links", C.c_int32), ("degrees", C.c_int32), ("axis", (C.c_double * 3) * 8), ("off", (C.c_double * 3) * 8),
                ("tool", C.c_double * 3)]


def make_kin_chain(axis, off, tool, degrees: bool) -> KinChain:
    """axis / off: n_links rows of 3 values, tool: 3 values"""
    ch = KinChain()
    ch.n_links, ch.degrees = len(axis), 1 if degrees else 0
    assert len(off) == len(axis) <= 8
    for i, (a, o) in enumerate(zip(axis, off)):
        for j in range(3):
            ch.axis[i][j], ch.off[i][j] = float(a[j]), float(o[j])
    for j in range(3):
        ch.tool[j] = float(tool[j])
    return ch


class PathResult(C.Structure):
    """struct batotp_path_result"""

    _fields_ = [
        ("t_rev", C.c_double),
        ("t_total", C.c_double),
        ("n_rev", C.c_int64),
        ("n_fwd", C.c_int64),
        ("steps_rev", C.c_int64),
        ("steps_fwd", C.c_int64),
        ("status_rev", C.c_uint32),
        ("status_fwd", C.c_uint32),
        ("n_bisect_fail_rev", C.c_int32),
        ("n_bisect_fail_fwd", C.c_int32),
    ]


RESULT_DTYPE = np.dtype(
    [
        ("t_rev", "<f8"), ("t_total", "<f8"), ("n_rev", "<i8"), ("n_fwd", "<i8"),
        ("steps_rev", "<i8"), ("steps_fwd", "<i8"), ("status_rev", "<u4"), ("status_fwd", "<u4"),
        ("n_bisect_fail_rev", "<i4"), ("n_bisect_fail_fwd", "<i4"),
    ]
)
assert RESULT_DTYPE.itemsize == C.sizeof(PathResult)


def make_problem(n_joints: int, n_cart: int = 0, robot_type: int = ROBOT_GENJNT, flags: int = 0,
                 jnt_vel_max: Sequence[float] = (), jnt_acc_max: Sequence[float] = (),
                 jnt_trq_max: Sequence[float] = (), jnt_trq_min: Sequence[float] = (),
                 cart_vel_max: float = 0.0, cart_acc_max: float = 0.0, jnt_thresh: float = 1e-6,
                 cart_thresh: float = 1e-6, integ_res: float = 0.01, max_integ_time: float = 6000.0,
                 pmat: Optional[Sequence[float]] = None) -> Problem:
    p = Problem()
    p.n_joints, p.n_cart, p.robot_type, p.flags = n_joints, n_cart, robot_type, flags
    for name, vals in (("jnt_vel_max", jnt_vel_max), ("jnt_acc_max", jnt_acc_max),
                       ("jnt_trq_max", jnt_trq_max), ("jnt_trq_min", jnt_trq_min)):
        arr = getattr(p, name)
        for k, v in enumerate(vals):
            arr[k] = float(v)
    p.cart_vel_max, p.cart_acc_max = cart_vel_max, cart_acc_max
    p.jnt_thresh = jnt_thresh
    p.quad_rad_thresh = cart_thresh * cart_thresh  # reference ba.cpp:2048
    p.integ_res, p.max_integ_time = integ_res, max_integ_time
    if pmat is not None:
        for k, v in enumerate(pmat):
            p.pmat[k] = float(v)
    return p


class ResampleParams(C.Structure):
    """struct batotp_resample_params"""
    _fields_ = [
        ("n_joints", C.c_int32), ("n_cart", C.c_int32), ("robot_type", C.c_int32), ("path_type", C.c_int32),
        ("scale_type", C.c_int32), ("flags", C.c_uint32),
        ("s_weights", C.c_double * 3),
        ("theta_norm_res", C.c_double), ("theta_norm_res2", C.c_double),
        ("cart_norm_res", C.c_double), ("cart_norm_res2", C.c_double),
        ("jnt_thresh", C.c_double), ("cart_thresh", C.c_double),
        ("pmat", C.c_double * 9),
        ("input_decim_fact", C.c_int32), ("smooth_window", C.c_int32),
        # automatic integration resolution (flags & RS_AUTO_INTEG_RES): inputs of the rule
        ("jnt_vel_max", C.c_double * MAX_JOINTS), ("jnt_acc_max", C.c_double * MAX_JOINTS),
        ("cart_vel_max", C.c_double), ("cart_acc_max", C.c_double), ("quad_rad_thresh", C.c_double),
        ("degrees", C.c_int32), ("reserved", C.c_int32),
    ]

    @classmethod
    def from_bytes(cls, raw: bytes):
        """a struct stored by an earlier round (shorter: without the inputs of the automatic integration resolution)"""
        raw = bytes(raw)
        return cls.from_buffer_copy(raw + b"\0" * max(0, C.sizeof(cls) - len(raw)))


RS_AUTO_INTEG_RES = 1 << 16


class OutputParams(C.Structure):
    """struct batotp_output_params"""
    _fields_ = [("n_joints", C.c_int32), ("path_type", C.c_int32), ("integ_res", C.c_double), ("out_res", C.c_double),
                ("out_smooth_fact", C.c_double)]


class BatotpError(RuntimeError):
    pass


# ---- audit of finished trajectories (include/batotp_hip_audit.h) -------------------------------------------------------
AUDIT_BLOCK_POINTS = 1024   # BATOTP_AUDIT_BLOCK_POINTS: points per workgroup of the audit kernel
INVDYN_BLOCK_POINTS = 128   # BATOTP_INVDYN_BLOCK_POINTS (include/batotp_hip_invdyn.h): points per workgroup of the torque kernel
AUDIT_JNT_VEL, AUDIT_JNT_ACC, AUDIT_CART_VEL, AUDIT_CART_ACC, AUDIT_TRQ = range(5)
AUDIT_FAMILIES = ("JNT_VEL", "JNT_ACC", "CART_VEL", "CART_ACC", "TRQ")


class AuditPeak(C.Structure):
    """struct batotp_audit_peak"""
    _fields_ = [("peak", C.c_double), ("at", C.c_int64), ("row", C.c_int32), ("reserved", C.c_int32)]


class PathAudit(C.Structure):
    """struct batotp_path_audit"""
    _fields_ = [("fam", AuditPeak * 5), ("n_pts", C.c_int64), ("n_over", C.c_int64), ("n_nonfinite", C.c_int64)]


AUDIT_DTYPE = np.dtype([("fam", [("peak", "<f8"), ("at", "<i8"), ("row", "<i4"), ("reserved", "<i4")], (5,)),
                        ("n_pts", "<i8"), ("n_over", "<i8"), ("n_nonfinite", "<i8")])
assert AUDIT_DTYPE.itemsize == C.sizeof(PathAudit)


# ---- stretching finished trajectories in time (include/batotp_hip_stretch.h) ----------------------------------------------
STRETCH_BLOCK_POINTS = 256          # BATOTP_STRETCH_BLOCK_POINTS: new points per workgroup of the stretch kernel
STRETCH_MAX_POINTS = 1 << 40        # BATOTP_STRETCH_MAX_POINTS
STRETCH_PASSES, STRETCH_ROUNDS, STRETCH_CAPPED = 0, 1, 2


class PathStretch(C.Structure):
    """struct batotp_path_stretch"""
    _fields_ = [("n_in", C.c_int64), ("n_out", C.c_int64), ("factor", C.c_double), ("rounds", C.c_int32), ("status", C.c_int32)]


STRETCH_DTYPE = np.dtype([("n_in", "<i8"), ("n_out", "<i8"), ("factor", "<f8"), ("rounds", "<i4"), ("status", "<i4")])
assert STRETCH_DTYPE.itemsize == C.sizeof(PathStretch) == 32


# ---- stretching until the torque limits pass (include/batotp_hip_tscale.h) ------------------------------------------------
TSCALE_BLOCK_POINTS = 128           # BATOTP_TSCALE_BLOCK_POINTS: points per workgroup of the scale kernel
STRETCH_STATIC = 3                  # BATOTP_STRETCH_STATIC


class PathTscale(C.Structure):
    """struct batotp_path_tscale"""
    _fields_ = [("s", C.c_double), ("at", C.c_int64), ("row", C.c_int32), ("side", C.c_int32), ("n_static", C.c_int64), ("reserved", C.c_int64)]


TSCALE_DTYPE = np.dtype([("s", "<f8"), ("at", "<i8"), ("row", "<i4"), ("side", "<i4"), ("n_static", "<i8"), ("reserved", "<i8")])
assert TSCALE_DTYPE.itemsize == C.sizeof(PathTscale) == 40


# ---- the continuous torque rating: RMS torques, energy, peak power (include/batotp_hip_duty.h) -----------------------------
DUTY_BLOCK_POINTS = 128             # BATOTP_DUTY_BLOCK_POINTS: points per block of the sum, which is part of the definition
MAX_LINKS = 8                       # BATOTP_MAX_LINKS


class PathDuty(C.Structure):
    """struct batotp_path_duty"""
    _fields_ = [("rms", C.c_double * MAX_LINKS), ("util", C.c_double), ("row", C.c_int32), ("n_hold", C.c_int32), ("s", C.c_double),
                ("s_row", C.c_int32), ("reserved", C.c_int32), ("energy", C.c_double), ("peak_power", C.c_double), ("power_at", C.c_int64),
                ("n_pts", C.c_int64)]


class PathDutySums(C.Structure):
    """struct batotp_path_duty_sums"""
    _fields_ = [("S", (C.c_double * 7) * MAX_LINKS), ("W", C.c_double), ("peak_power", C.c_double), ("power_at", C.c_int64), ("n_pts", C.c_int64)]


DUTY_DTYPE = np.dtype([("rms", "<f8", (MAX_LINKS,)), ("util", "<f8"), ("row", "<i4"), ("n_hold", "<i4"), ("s", "<f8"), ("s_row", "<i4"),
                       ("reserved", "<i4"), ("energy", "<f8"), ("peak_power", "<f8"), ("power_at", "<i8"), ("n_pts", "<i8")])
DUTY_SUMS_DTYPE = np.dtype([("S", "<f8", (MAX_LINKS, 7)), ("W", "<f8"), ("peak_power", "<f8"), ("power_at", "<i8"), ("n_pts", "<i8")])
assert DUTY_DTYPE.itemsize == C.sizeof(PathDuty) == 128 and DUTY_SUMS_DTYPE.itemsize == C.sizeof(PathDutySums) == 480


def _dptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Library:
    """One loaded implementation of the C-ABI."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise BatotpError(f"{path} is missing -- build it first (python -c 'import __graft_entry__ as g; g.build()')")
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        P, I32, I64, D = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
        sig = {
            "batotp_hip_device_count": [C.POINTER(C.c_int)],
            "batotp_hip_ctx_create": [C.c_int, C.POINTER(P)],
            "batotp_hip_ctx_destroy": [P],
            "batotp_hip_ctx_trim": [P],
            "batotp_hip_fp64_kat": [P, I64, D, D, D, D, D],
            "batotp_hip_div6_kat": [P, I64, D, D],
            "batotp_hip_spline_lanes_kat": [P, I64, D, D, D, C.POINTER(I32)],
            "batotp_hip_sdiv_kat": [P, I64, D, D, D, C.POINTER(I32)],
            "batotp_hip_batch_create": [P, C.POINTER(Problem), I32, C.POINTER(C.c_int64), I64, C.POINTER(P)],
            "batotp_hip_batch_destroy": [P],
            "batotp_hip_upload_knots": [P, I32, I32, D, D],
            "batotp_hip_upload_knots_device": [P, I32, I32, P, D],
            "batotp_hip_upload_knots_device_rows": [P, I32, I32, P, I32, D],
            "batotp_hip_upload_rr_trig": [P, I32, D],
            "batotp_hip_set_serial_model": [P, C.POINTER(SerialModel)],
            "batotp_hip_upload_joint_trig": [P, I32, D],
            "batotp_hip_builtin_serial_model": [I32, C.POINTER(SerialModel)],
            "batotp_hip_upload_path_sites": [P, I32, D, C.c_double, C.c_double, I32],
            "batotp_hip_upload_coeffs": [P, I32, I32, D],
            "batotp_hip_upload_curve": [P, I32, D, D, I64],
            "batotp_hip_precompute": [P, I32],
            "batotp_hip_pointwise_mvc": [P],
            "batotp_hip_sweep": [P, I32],
            "batotp_hip_optimize": [P],
            "batotp_hip_synchronize": [P],
            "batotp_hip_get_results": [P, C.c_void_p],
            "batotp_hip_download_curve": [P, I32, I32, D, D, I64, C.POINTER(C.c_int64)],
            "batotp_hip_download_coeffs": [P, I32, I32, D],
            "batotp_hip_download_samples": [P, I32, I32, D],
            "batotp_hip_download_dyn": [P, I32, I32, I32, D],
            "batotp_hip_download_mvc": [P, I32, D, D, D],
            "batotp_hip_results_device_ptr": [P, C.POINTER(P), C.POINTER(C.c_int64)],
            "batotp_hip_pack_curves": [P, I32, I32, I32, P, I64, C.POINTER(C.c_int64)],
            "batotp_hip_last_kernel_ms": [P, I32, C.POINTER(C.c_float)],
            "batotp_hip_batch_bytes": [P, C.POINTER(C.c_int64)],
            "batotp_hip_set_sweep_group": [P, I32],
            "batotp_hip_set_paths_per_wave": [P, I32],
            "batotp_hip_set_overlap": [P, I32],
            "batotp_hip_set_sweep_hold": [P, I32, I32],
            "batotp_hip_set_flat_form": [P, I32],
            "batotp_hip_set_sweep_prefetch": [P, I32, I32],
            "batotp_hip_set_spline_tiles": [P, I32],
            "batotp_hip_set_fast_forward": [P, I32],
            "batotp_hip_set_cert_hold": [P, I32],
            "batotp_hip_set_poison": [P, I32],
            "batotp_hip_set_resample_trace": [P, I32],
            "batotp_hip_resampled_trace": [P, C.POINTER(C.c_uint64)],
            "batotp_hip_resampled_trace_data": [P, I32, D, I64, C.POINTER(I64)],
            "batotp_hip_set_k3_form": [P, I32],
            "batotp_hip_set_path_order": [P, I32],
            "batotp_hip_set_workspace_budget": [P, C.c_int64, C.c_int64],
            "batotp_hip_spline_tile_fallbacks": [P, C.POINTER(I32)],
            "batotp_hip_flat_loop_status": [P, C.POINTER(I32)],
            "batotp_hip_toolchain": [C.c_char_p, C.c_char_p, I32],
            "batotp_hip_last_sweep_launch": [P, I32, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32)],
            "batotp_hip_resample": [P, C.POINTER(ResampleParams), I32, C.POINTER(C.c_int64), D, D, C.POINTER(P)],
            "batotp_hip_resampled_destroy": [P],
            "batotp_hip_resampled_auto": [P, D, D, C.POINTER(I32)],
            "batotp_hip_upload_forward_curve": [P, I32, D, D, I64, C.c_double],
            "batotp_hip_set_path_integ_res": [P, I32, I32, D],
            "batotp_hip_resampled_info": [P, C.POINTER(C.c_int64), D, C.POINTER(C.c_uint32)],
            "batotp_hip_resampled_knots_device": [P, C.POINTER(P), C.POINTER(C.c_int64)],
            "batotp_hip_resampled_download": [P, I32, D],
            "batotp_hip_resampled_ms": [P, C.POINTER(C.c_float)],
            "batotp_hip_resampled_checksums": [P, C.POINTER(C.c_uint64)],
            "batotp_hip_output": [P, C.POINTER(OutputParams), I32, I32, C.POINTER(P)],
            "batotp_hip_output_destroy": [P],
            "batotp_hip_out_segmax_kat": [P, I32, C.POINTER(I32), C.POINTER(I32)],
            "batotp_hip_output_info": [P, C.POINTER(C.c_int64), D],
            "batotp_hip_output_channels": [P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32)],
            "batotp_hip_output_download": [P, I32, D],
            "batotp_hip_output_download_all": [P, D],
            "batotp_hip_output_device": [P, C.POINTER(P), C.POINTER(C.c_int64)],
            "batotp_hip_output_ms": [P, C.POINTER(C.c_float)],
        }
        for name, argtypes in sig.items():
            fn = getattr(L, name)  # raises AttributeError if the symbol is not exported
            fn.argtypes = argtypes
            fn.restype = C.c_int
        L.batotp_hip_last_error.restype = C.c_char_p
        L.batotp_hip_last_error.argtypes = []
        self.symbols = sorted(list(sig) + ["batotp_hip_last_error"])
        # entry points of include/batotp_hip_audit.h: bound only where the library exports them (a checker behind this class
        # has none); `symbols` stays the table of include/batotp_hip.h
        audit_sig = {
            "batotp_hip_output_audit": [P, C.POINTER(Problem), C.c_double, C.c_void_p],
            "batotp_hip_output_audit_device": [P, C.POINTER(Problem), C.c_double, C.c_void_p],
            "batotp_hip_output_audit_ms": [P, C.POINTER(C.c_float)],
            "batotp_hip_output_from_rows": [P, I32, C.POINTER(C.c_int64), D, I32, I32, I32, D, C.POINTER(P)],
        }
        self.audit_symbols = sorted(audit_sig)
        self.has_audit = all(hasattr(L, name) for name in audit_sig)
        if self.has_audit:
            for name, argtypes in audit_sig.items():
                fn = getattr(L, name)
                fn.argtypes = argtypes
                fn.restype = C.c_int

        # ... and of include/batotp_hip_kin.h (the tool point of a kinematic chain), likewise
        kin_sig = {
            "batotp_hip_kin_chain_from_model": [C.POINTER(SerialModel), D, C.POINTER(KinChain)],
            "batotp_hip_builtin_kin_chain": [I32, C.POINTER(KinChain)],
            "batotp_hip_fwdkin_chain": [P, C.POINTER(KinChain), C.c_uint32, I32, C.POINTER(C.c_int64), D, D],
            "batotp_hip_resample_chain": [P, C.POINTER(ResampleParams), C.POINTER(KinChain), I32, C.POINTER(C.c_int64), D, D, C.POINTER(P)],
            "batotp_hip_set_kin_chain": [P, C.POINTER(KinChain)],
        }
        self.kin_symbols = sorted(kin_sig)
        self.has_kin = all(hasattr(L, name) for name in kin_sig)
        if self.has_kin:
            for name, argtypes in kin_sig.items():
                fn = getattr(L, name)
                fn.argtypes = argtypes
                fn.restype = C.c_int

        # ... and of include/batotp_hip_invdyn.h (torque rows for finished trajectories), likewise
        invdyn_sig = {
            "batotp_hip_output_torques": [P, C.POINTER(SerialModel), C.c_uint32, C.POINTER(P)],
            "batotp_hip_output_torques_ms": [P, C.POINTER(C.c_float)],
            "batotp_hip_output_torques_ranges": [P, C.POINTER(I32)],
        }
        self.invdyn_symbols = sorted(invdyn_sig)
        self.has_invdyn = all(hasattr(L, name) for name in invdyn_sig)
        if self.has_invdyn:
            for name, argtypes in invdyn_sig.items():
                fn = getattr(L, name)
                fn.argtypes = argtypes
                fn.restype = C.c_int

        # ... and of include/batotp_hip_stretch.h (finished trajectories stretched in time), likewise
        stretch_sig = {
            "batotp_hip_output_stretch_to": [P, C.POINTER(C.c_int64), C.POINTER(P)],
            "batotp_hip_output_stretch_by": [P, D, C.POINTER(P)],
            "batotp_hip_output_stretch_audit": [P, C.POINTER(Problem), C.c_double, I32, C.c_double, C.POINTER(P), C.c_void_p],
            "batotp_hip_output_stretch_ms": [P, C.POINTER(C.c_float)],
            "batotp_hip_output_stretch_ranges": [P, C.POINTER(I32)],
        }
        self.stretch_symbols = sorted(stretch_sig)
        self.has_stretch = all(hasattr(L, name) for name in stretch_sig)
        if self.has_stretch:
            for name, argtypes in stretch_sig.items():
                fn = getattr(L, name)
                fn.argtypes = argtypes
                fn.restype = C.c_int

        # ... and of include/batotp_hip_tscale.h (stretched until the torque limits pass), likewise
        tscale_sig = {
            "batotp_hip_output_torque_scale": [P, C.POINTER(Problem), C.POINTER(SerialModel), C.c_uint32, C.c_double, C.POINTER(P), C.c_void_p],
            "batotp_hip_output_stretch_torques": [P, C.POINTER(Problem), C.POINTER(SerialModel), C.c_uint32, C.c_double, I32, C.c_double,
                                                  C.POINTER(P), C.c_void_p, C.c_void_p],
            "batotp_hip_output_tscale_ms": [P, C.POINTER(C.c_float)],
            "batotp_hip_output_tscale_ranges": [P, C.POINTER(I32)],
        }
        self.tscale_symbols = sorted(tscale_sig)
        self.has_tscale = all(hasattr(L, name) for name in tscale_sig)
        if self.has_tscale:
            for name, argtypes in tscale_sig.items():
                fn = getattr(L, name)
                fn.argtypes = argtypes
                fn.restype = C.c_int

        # ... and of include/batotp_hip_duty.h (the continuous torque rating), likewise
        duty_sig = {
            "batotp_hip_output_duty": [P, C.POINTER(SerialModel), C.c_uint32, D, C.c_double, C.POINTER(P), C.c_void_p, C.c_void_p],
            "batotp_hip_output_stretch_duty": [P, C.POINTER(Problem), C.POINTER(SerialModel), C.c_uint32, D, C.c_double, I32, C.c_double,
                                               C.POINTER(P), C.c_void_p, C.c_void_p, C.c_void_p],
            "batotp_hip_output_duty_ms": [P, C.POINTER(C.c_float)],
            "batotp_hip_output_duty_ranges": [P, C.POINTER(I32)],
        }
        self.duty_symbols = sorted(duty_sig)
        self.has_duty = all(hasattr(L, name) for name in duty_sig)
        if self.has_duty:
            for name, argtypes in duty_sig.items():
                fn = getattr(L, name)
                fn.argtypes = argtypes
                fn.restype = C.c_int

    def need_duty(self):
        if not self.has_duty:
            raise BatotpError(f"{self.path} does not export the duty entry points (include/batotp_hip_duty.h)")

    def need_tscale(self):
        if not self.has_tscale:
            raise BatotpError(f"{self.path} does not export the torque-scale entry points (include/batotp_hip_tscale.h)")

    def need_stretch(self):
        if not self.has_stretch:
            raise BatotpError(f"{self.path} does not export the stretch entry points (include/batotp_hip_stretch.h)")

    def need_invdyn(self):
        if not self.has_invdyn:
            raise BatotpError(f"{self.path} does not export the inverse-dynamics entry points (include/batotp_hip_invdyn.h)")

    def need_kin(self):
        if not self.has_kin:
            raise BatotpError(f"{self.path} does not export the kinematic-chain entry points (include/batotp_hip_kin.h)")

    def builtin_kin_chain(self, robot_type: int) -> KinChain:
        self.need_kin()
        ch = KinChain()
        self.check(self.lib.batotp_hip_builtin_kin_chain(robot_type, C.byref(ch)), "builtin_kin_chain")
        return ch

    def kin_chain_from_model(self, model: SerialModel, tool) -> KinChain:
        self.need_kin()
        ch = KinChain()
        t = np.ascontiguousarray(tool, dtype=np.float64)
        assert t.size == 3
        self.check(self.lib.batotp_hip_kin_chain_from_model(C.byref(model), _dptr(t), C.byref(ch)), "kin_chain_from_model")
        return ch

    def need_audit(self):
        if not self.has_audit:
            raise BatotpError(f"{self.path} does not export the audit entry points (include/batotp_hip_audit.h)")

    def check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.batotp_hip_last_error()
            raise BatotpError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")

    def builtin_serial_model(self, robot_type: int) -> SerialModel:
        m = SerialModel()
        self.check(self.lib.batotp_hip_builtin_serial_model(robot_type, C.byref(m)), "builtin_serial_model")
        return m

    def toolchain(self):
        """(built with, flat loop validated with)"""
        a, b = C.create_string_buffer(256), C.create_string_buffer(256)
        self.check(self.lib.batotp_hip_toolchain(a, b, 256), "toolchain")
        return a.value.decode(), b.value.decode()

    def device_count(self) -> int:
        n = C.c_int(0)
        self.lib.batotp_hip_device_count(C.byref(n))
        return n.value


# debug aid for test runs (tests/conftest.py, BATOTP_TEST_POISON=1): every context fills its workspaces with 0xFF bytes before use
DEFAULT_POISON = False


class Context:
    def __init__(self, library: Library, device: int = 0):
        self.library = library
        self.handle = C.c_void_p()
        library.check(library.lib.batotp_hip_ctx_create(device, C.byref(self.handle)), "batotp_hip_ctx_create")
        if DEFAULT_POISON:
            self.set_poison(True)

    def set_resample_trace(self, on: bool):
        """one-path resample calls keep a checksum of every intermediate stage (Resampled.trace)"""
        self.library.check(self.library.lib.batotp_hip_set_resample_trace(self.handle, 1 if on else 0), "set_resample_trace")

    def set_poison(self, on: bool):
        """debug aid: workspaces and batch arrays are filled with 0xFF bytes before use (include/batotp_hip.h)"""
        self.library.check(self.library.lib.batotp_hip_set_poison(self.handle, 1 if on else 0), "set_poison")

    def close(self):
        if self.handle:
            self.library.lib.batotp_hip_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sweep_group(self, lanes: int):
        self.library.check(self.library.lib.batotp_hip_set_sweep_group(self.handle, lanes), "set_sweep_group")

    def set_overlap(self, on: bool):
        self.library.check(self.library.lib.batotp_hip_set_overlap(self.handle, 1 if on else 0), "set_overlap")

    def set_sweep_hold(self, reverse: int, forward: int):
        self.library.check(self.library.lib.batotp_hip_set_sweep_hold(self.handle, reverse, forward), "set_sweep_hold")

    def set_flat_form(self, form: int):
        """1 = k_sweep8, in the forward sweep at hold 8 its lockstep form k_sweep8_lock (default); 2 = k_sweep8's flat loop in the
        forward sweep too (the previous form: A/B, parity); 0 = the flat instantiation of the general kernel (include/batotp_hip.h)"""
        self.library.check(self.library.lib.batotp_hip_set_flat_form(self.handle, form), "set_flat_form")

    def set_sweep_prefetch(self, reverse: int, forward: int):
        self.library.check(self.library.lib.batotp_hip_set_sweep_prefetch(self.handle, reverse, forward), "set_sweep_prefetch")

    def set_cert_hold(self, hold: int):
        """k_sweep8, reverse sweep: hold of the certificate phase (-1 automatic, 0 off, 1..8); include/batotp_hip.h"""
        self.library.check(self.library.lib.batotp_hip_set_cert_hold(self.handle, int(hold)), "set_cert_hold")

    def set_fast_forward(self, on):
        """certified fast-forward of the bisection (include/batotp_hip.h); never changes a result"""
        self.library.check(self.library.lib.batotp_hip_set_fast_forward(self.handle, int(on)), "set_fast_forward")

    def set_workspace_budget(self, resample_bytes: int = 0, output_bytes: int = 0):
        """scratch bytes per chunk of paths of the resampler / the output stage (0 = from the free device memory)"""
        self.library.check(self.library.lib.batotp_hip_set_workspace_budget(self.handle, int(resample_bytes), int(output_bytes)), "set_workspace_budget")

    def set_path_order(self, mode: int):
        """ragged batches: 1 = the sweeps take the paths longest first (default), 0 = in the order given"""
        self.library.check(self.library.lib.batotp_hip_set_path_order(self.handle, int(mode)), "set_path_order")

    def set_k3_form(self, form: int):
        """per-knot evaluation of velocity / acceleration-only problems: 1 = k_pointwise_va (default), 0 = the general kernel"""
        self.library.check(self.library.lib.batotp_hip_set_k3_form(self.handle, int(form)), "set_k3_form")

    def set_spline_tiles(self, on):
        """True / False, or -1 for the automatic choice (tiles for small batches)"""
        self.library.check(self.library.lib.batotp_hip_set_spline_tiles(self.handle, -1 if on == -1 else int(on)), "set_spline_tiles")   # (2: the single-pass kernel for pairs)

    def flat_loop_status(self) -> int:
        """1 = the automatic loop choice uses the flat loop; negative: why not (include/batotp_hip.h)"""
        st = C.c_int32(0)
        self.library.check(self.library.lib.batotp_hip_flat_loop_status(self.handle, C.byref(st)), "flat_loop_status")
        return st.value

    def set_paths_per_wave(self, n: int):
        self.library.check(self.library.lib.batotp_hip_set_paths_per_wave(self.handle, n), "set_paths_per_wave")

    def synchronize(self):
        self.library.check(self.library.lib.batotp_hip_synchronize(self.handle), "synchronize")

    def trim(self):
        """release the workspaces cached between resample calls (invalidates live Resampled objects)"""
        self.library.check(self.library.lib.batotp_hip_ctx_trim(self.handle), "ctx_trim")

    def fp64_kat(self, a: np.ndarray, b: np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        q, r, p = np.empty_like(a), np.empty_like(a), np.empty_like(a)
        self.library.check(self.library.lib.batotp_hip_fp64_kat(self.handle, a.size, _dptr(a), _dptr(b), _dptr(q), _dptr(r), _dptr(p)), "fp64_kat")
        return q, r, p


class Resampled:
    """Uniform-s knots of a set of taught paths, produced by batotp_hip_resample and resident on the
    device (feed them to Batch.upload_knots_device)."""

    def __init__(self, ctx: Context, prm: ResampleParams, x_list: Sequence[np.ndarray], sres_in: Sequence[float],
                 chain: Optional[KinChain] = None):
        """chain: the kinematic chain whose tool point fills the Cartesian rows of a JOINT path (batotp_hip_resample_chain)"""
        self.ctx, self.lib, self.L = ctx, ctx.library.lib, ctx.library
        if chain is not None:
            self.L.need_kin()
        self.n_paths = len(x_list)
        n_ch_in = prm.n_joints + prm.n_cart
        # poses (path type BOTH, 6 rows) leave the resampler as position + quaternion: one row more
        self.n_ch = n_ch_in + (1 if (prm.path_type == PATH_BOTH and prm.n_cart == 6) else 0)
        n_in = np.ascontiguousarray([x.shape[1] for x in x_list], dtype=np.int64)
        for x in x_list:
            assert x.shape[0] == n_ch_in
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(x, dtype=np.float64).ravel() for x in x_list]))
        sr = np.ascontiguousarray(sres_in, dtype=np.float64)
        self.handle = C.c_void_p()
        if chain is None:
            self.L.check(self.lib.batotp_hip_resample(ctx.handle, C.byref(prm), self.n_paths, n_in.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      _dptr(flat), _dptr(sr), C.byref(self.handle)), "batotp_hip_resample")
        else:
            self.L.check(self.lib.batotp_hip_resample_chain(ctx.handle, C.byref(prm), C.byref(chain), self.n_paths,
                                                            n_in.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(flat), _dptr(sr),
                                                            C.byref(self.handle)), "batotp_hip_resample_chain")
        self.n_knots = np.zeros(self.n_paths, dtype=np.int64)
        self.sres = np.zeros(self.n_paths, dtype=np.float64)
        self.status = np.zeros(self.n_paths, dtype=np.uint32)
        self.L.check(self.lib.batotp_hip_resampled_info(self.handle, self.n_knots.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(self.sres),
                                                        self.status.ctypes.data_as(C.POINTER(C.c_uint32))), "resampled_info")

    def auto(self):
        """(integ_res[n_paths], s_weights[n_paths][3], scale_type[n_paths]) the automatic integration resolution left"""
        ir = np.zeros(self.n_paths); sw = np.zeros((self.n_paths, 3)); st = np.zeros(self.n_paths, dtype=np.int32)
        self.L.check(self.lib.batotp_hip_resampled_auto(self.handle, _dptr(ir), _dptr(sw), st.ctypes.data_as(C.POINTER(C.c_int32))), "resampled_auto")
        return ir, sw, st

    def close(self):
        if self.handle:
            self.lib.batotp_hip_resampled_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_ptr(self) -> int:
        ptr, cnt = C.c_void_p(), C.c_int64(0)
        self.L.check(self.lib.batotp_hip_resampled_knots_device(self.handle, C.byref(ptr), C.byref(cnt)), "resampled_knots_device")
        return ptr.value

    def knots(self, path: int) -> np.ndarray:
        y = np.empty((self.n_ch, int(self.n_knots[path])), dtype=np.float64)
        self.L.check(self.lib.batotp_hip_resampled_download(self.handle, path, _dptr(y)), "resampled_download")
        return y

    def ms(self) -> float:
        v = C.c_float(0)
        self.L.check(self.lib.batotp_hip_resampled_ms(self.handle, C.byref(v)), "resampled_ms")
        return float(v.value)

    def trace(self) -> np.ndarray:
        """checksums of the eight intermediate stages of a traced one-path call (include/batotp_hip.h)"""
        out = np.zeros(8, dtype=np.uint64)
        self.L.check(self.lib.batotp_hip_resampled_trace(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64))), "resampled_trace")
        return out

    def trace_data(self, stage: int) -> np.ndarray:
        """the array of a traced stage that is kept on the host (2, 3); empty for the others"""
        n = C.c_int64(0)
        self.L.check(self.lib.batotp_hip_resampled_trace_data(self.handle, stage, None, 0, C.byref(n)), "resampled_trace_data")
        out = np.empty(int(n.value), dtype=np.float64)
        if n.value:
            self.L.check(self.lib.batotp_hip_resampled_trace_data(self.handle, stage, _dptr(out), n.value, C.byref(n)), "resampled_trace_data")
        return out

    def checksums(self) -> np.ndarray:
        """order-independent 64-bit checksum of every path's knots, computed where the knots are (include/batotp_hip.h)"""
        out = np.zeros(self.n_paths, dtype=np.uint64)
        self.L.check(self.lib.batotp_hip_resampled_checksums(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64))), "resampled_checksums")
        return out


class Output:
    """Constant-time output trajectories of a range of paths of a batch (batotp_hip_output), resident on the device."""

    def __init__(self, batch: "Batch", prm: OutputParams, path0: int, n_paths: int, per_path_steps: bool = False):
        """per_path_steps: every path is sampled with its own integration step (Batch.set_path_integ_res) instead of prm.integ_res"""
        self.lib, self.L = batch.lib, batch.L
        if per_path_steps:
            prm = OutputParams.from_buffer_copy(bytes(prm))
            prm.integ_res = OUT_STEP_PER_PATH
        self.n_paths, self.n_joints = n_paths, prm.n_joints
        self.handle = C.c_void_p()
        self.L.check(self.lib.batotp_hip_output(batch.handle, C.byref(prm), path0, n_paths, C.byref(self.handle)), "batotp_hip_output")
        self._read_info()

    def _read_info(self):
        n_paths = self.n_paths
        self.n_pts = np.zeros(n_paths, dtype=np.int64)
        self.sres = np.zeros(n_paths, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_output_info(self.handle, self.n_pts.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(self.sres)), "output_info")
        a, b_, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.L.check(self.lib.batotp_hip_output_channels(self.handle, C.byref(a), C.byref(b_), C.byref(c)), "output_channels")
        self.n_theta, self.n_cart, self.n_trq = a.value, b_.value, c.value
        self.n_rows = a.value + b_.value + c.value

    @classmethod
    def from_rows(cls, ctx: "Context", rows_list: Sequence[np.ndarray], sres, n_theta: int, n_cart: int, n_trq: int) -> "Output":
        """a genuine Output from trajectories computed elsewhere (batotp_hip_output_from_rows): rows_list[k] is
        [n_theta + n_cart + n_trq][n_pts of path k], sres[k] (or one value for all) the time step of path k"""
        ctx.library.need_audit()
        self = cls.__new__(cls)
        self.lib, self.L = ctx.library.lib, ctx.library
        self.n_paths, self.n_joints = len(rows_list), n_theta
        R = n_theta + n_cart + n_trq
        arrs = [np.ascontiguousarray(r, dtype=np.float64) for r in rows_list]
        for a in arrs:
            assert a.ndim == 2 and a.shape[0] == R, (a.shape, R)
        n_pts = np.ascontiguousarray([a.shape[1] for a in arrs], dtype=np.int64)
        sr = np.ascontiguousarray(np.broadcast_to(np.asarray(sres, dtype=np.float64), (len(arrs),)))
        flat = np.ascontiguousarray(np.concatenate([a.ravel() for a in arrs])) if arrs else np.zeros(0)
        self.handle = C.c_void_p()
        self.L.check(self.lib.batotp_hip_output_from_rows(ctx.handle, len(arrs), n_pts.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(sr),
                                                          n_theta, n_cart, n_trq, _dptr(flat), C.byref(self.handle)), "batotp_hip_output_from_rows")
        self._read_info()
        return self

    def audit(self, prob: Problem, tol: float = 0.0) -> np.ndarray:
        """the trajectories against the limits of prob, on the device (include/batotp_hip_audit.h): one AUDIT_DTYPE row per path"""
        self.L.need_audit()
        out = np.zeros(self.n_paths, dtype=AUDIT_DTYPE)
        self.L.check(self.lib.batotp_hip_output_audit(self.handle, C.byref(prob), float(tol), out.ctypes.data_as(C.c_void_p)), "output_audit")
        return out

    def audit_ms(self) -> float:
        """milliseconds of the kernels of the last audit"""
        self.L.need_audit()
        v = C.c_float(0)
        self.L.check(self.lib.batotp_hip_output_audit_ms(self.handle, C.byref(v)), "output_audit_ms")
        return float(v.value)

    def torques(self, model: SerialModel, host_trig: bool = True, flags: Optional[int] = None) -> "Output":
        """a NEW Output: these joint and Cartesian rows followed by model.n_links torque rows, the inverse dynamics of the chain
        model at every output point (batotp_hip_output_torques, include/batotp_hip_invdyn.h).  host_trig: cos / sin from the host
        libm (bit parity with tests/invdyn_reference.py), else the device libm; flags overrides it with a raw flag word"""
        self.L.need_invdyn()
        new = Output.__new__(Output)
        new.lib, new.L = self.lib, self.L
        new.n_paths, new.n_joints = self.n_paths, self.n_joints
        new.handle = C.c_void_p()
        f = (F_HOST_TRIG if host_trig else 0) if flags is None else int(flags)
        self.L.check(self.lib.batotp_hip_output_torques(self.handle, C.byref(model), f, C.byref(new.handle)), "batotp_hip_output_torques")
        new._read_info()
        return new

    def torques_ms(self) -> float:
        """milliseconds of the torque kernels of the call that made this Output (Output.torques)"""
        self.L.need_invdyn()
        v = C.c_float(0)
        self.L.check(self.lib.batotp_hip_output_torques_ms(self.handle, C.byref(v)), "output_torques_ms")
        return float(v.value)

    def torques_ranges(self) -> int:
        """ranges of paths the call that made this Output was cut into (workspace budget)"""
        self.L.need_invdyn()
        v = C.c_int32(0)
        self.L.check(self.lib.batotp_hip_output_torques_ranges(self.handle, C.byref(v)), "output_torques_ranges")
        return int(v.value)

    def _like(self) -> "Output":
        new = Output.__new__(Output)
        new.lib, new.L = self.lib, self.L
        new.n_paths, new.n_joints = self.n_paths, self.n_joints
        new.handle = C.c_void_p()
        return new

    def stretch_to(self, n_out) -> "Output":
        """a NEW Output: the same paths with n_out[k] >= n_pts[k] points at the same time step, the Catmull-Rom cubic through
        these rows (batotp_hip_output_stretch_to, include/batotp_hip_stretch.h)"""
        self.L.need_stretch()
        n2 = np.ascontiguousarray(n_out, dtype=np.int64)
        assert n2.shape == (self.n_paths,), (n2.shape, self.n_paths)
        new = self._like()
        self.L.check(self.lib.batotp_hip_output_stretch_to(self.handle, n2.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(new.handle)),
                     "batotp_hip_output_stretch_to")
        new._read_info()
        return new

    def stretch_by(self, factor) -> "Output":
        """stretch_to with n_out[k] = ceil((n_pts[k] - 1) * factor[k]) + 1; factor: one value for all paths or one per path"""
        self.L.need_stretch()
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(factor, dtype=np.float64), (self.n_paths,)))
        new = self._like()
        self.L.check(self.lib.batotp_hip_output_stretch_by(self.handle, _dptr(f), C.byref(new.handle)), "batotp_hip_output_stretch_by")
        new._read_info()
        return new

    def stretch_audit(self, prob: Problem, target: float = 1.0, max_rounds: int = 8, max_factor: float = 16.0):
        """(a NEW Output, report): every path stretched, each by its own factor, until its audit against prob has every velocity
        and acceleration peak <= target (batotp_hip_output_stretch_audit); report is one STRETCH_DTYPE row per path"""
        self.L.need_stretch()
        new = self._like()
        report = np.zeros(self.n_paths, dtype=STRETCH_DTYPE)
        self.L.check(self.lib.batotp_hip_output_stretch_audit(self.handle, C.byref(prob), float(target), int(max_rounds), float(max_factor),
                                                              C.byref(new.handle), report.ctypes.data_as(C.c_void_p)),
                     "batotp_hip_output_stretch_audit")
        new._read_info()
        return new, report

    def stretch_ms(self) -> float:
        """milliseconds of the stretch kernels of the call that made this Output"""
        self.L.need_stretch()
        v = C.c_float(0)
        self.L.check(self.lib.batotp_hip_output_stretch_ms(self.handle, C.byref(v)), "output_stretch_ms")
        return float(v.value)

    def stretch_ranges(self) -> int:
        """kernel launches (ranges of paths, over all rounds) of the call that made this Output"""
        self.L.need_stretch()
        v = C.c_int32(0)
        self.L.check(self.lib.batotp_hip_output_stretch_ranges(self.handle, C.byref(v)), "output_stretch_ranges")
        return int(v.value)

    def torque_scale(self, prob: Problem, model: SerialModel, target: float = 1.0, host_trig: bool = True, flags: Optional[int] = None):
        """(a NEW Output, records): the rows of Output.torques(model) and one TSCALE_DTYPE row per path -- the largest speed factor
        the torque range of prob admits at target, where it binds, and the points at which gravity alone leaves the range
        (batotp_hip_output_torque_scale, include/batotp_hip_tscale.h); flags overrides host_trig with a raw flag word"""
        self.L.need_tscale()
        new = self._like()
        rec = np.zeros(self.n_paths, dtype=TSCALE_DTYPE)
        f = (F_HOST_TRIG if host_trig else 0) if flags is None else int(flags)
        self.L.check(self.lib.batotp_hip_output_torque_scale(self.handle, C.byref(prob), C.byref(model), f, float(target), C.byref(new.handle),
                                                             rec.ctypes.data_as(C.c_void_p)), "batotp_hip_output_torque_scale")
        new._read_info()
        return new, rec

    def stretch_torques(self, prob: Problem, model: SerialModel, target: float = 1.0, max_rounds: int = 8, max_factor: float = 16.0,
                        host_trig: bool = True, flags: Optional[int] = None):
        """(a NEW Output, report, records): every path stretched, each by its own factor, until its velocity, acceleration AND torque
        peaks are <= target (batotp_hip_output_stretch_torques); the Output carries the torque rows of the stretched paths, report is
        one STRETCH_DTYPE row per path (status STRETCH_STATIC: gravity alone exceeds the range), records the TSCALE_DTYPE rows of
        the result"""
        self.L.need_tscale()
        new = self._like()
        report = np.zeros(self.n_paths, dtype=STRETCH_DTYPE)
        rec = np.zeros(self.n_paths, dtype=TSCALE_DTYPE)
        f = (F_HOST_TRIG if host_trig else 0) if flags is None else int(flags)
        self.L.check(self.lib.batotp_hip_output_stretch_torques(self.handle, C.byref(prob), C.byref(model), f, float(target), int(max_rounds),
                                                                float(max_factor), C.byref(new.handle), report.ctypes.data_as(C.c_void_p),
                                                                rec.ctypes.data_as(C.c_void_p)), "batotp_hip_output_stretch_torques")
        new._read_info()
        return new, report, rec

    def tscale_ms(self) -> float:
        """milliseconds of the scale kernels of the call that made this Output (torque_scale / stretch_torques), all rounds"""
        self.L.need_tscale()
        v = C.c_float(0)
        self.L.check(self.lib.batotp_hip_output_tscale_ms(self.handle, C.byref(v)), "output_tscale_ms")
        return float(v.value)

    def tscale_ranges(self) -> int:
        """launches of the scale kernel (ranges of paths, over all rounds) of the call that made this Output"""
        self.L.need_tscale()
        v = C.c_int32(0)
        self.L.check(self.lib.batotp_hip_output_tscale_ranges(self.handle, C.byref(v)), "output_tscale_ranges")
        return int(v.value)

    def _rated(self, model: SerialModel, rated) -> np.ndarray:
        r = np.ascontiguousarray(rated, dtype=np.float64)
        assert r.shape == (int(model.n_links),), (r.shape, int(model.n_links))
        return r

    def duty(self, model: SerialModel, rated, target: float = 1.0, host_trig: bool = True, sums: bool = False, flags: Optional[int] = None):
        """(a NEW Output, records[, sums]): the rows of Output.torques(model) and one DUTY_DTYPE row per path -- the RMS torque of every
        joint, its utilisation of the continuous torques rated[n_links], the speed factor at which the RMS torque meets target * rated,
        the mechanical energy and the peak power (batotp_hip_output_duty, include/batotp_hip_duty.h); sums=True: the raw
        DUTY_SUMS_DTYPE rows the kernels wrote as well"""
        self.L.need_duty()
        new = self._like()
        rec = np.zeros(self.n_paths, dtype=DUTY_DTYPE)
        raw = np.zeros(self.n_paths, dtype=DUTY_SUMS_DTYPE) if sums else None
        f = (F_HOST_TRIG if host_trig else 0) if flags is None else int(flags)
        self.L.check(self.lib.batotp_hip_output_duty(self.handle, C.byref(model), f, _dptr(self._rated(model, rated)), float(target), C.byref(new.handle),
                                                     rec.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p) if sums else None),
                     "batotp_hip_output_duty")
        new._read_info()
        return (new, rec, raw) if sums else (new, rec)

    def stretch_duty(self, prob: Problem, model: SerialModel, rated, target: float = 1.0, max_rounds: int = 8, max_factor: float = 16.0,
                     host_trig: bool = True, flags: Optional[int] = None):
        """(a NEW Output, report, scale records, duty records): Output.stretch_torques with the RMS family on top -- every path is
        stretched until its RMS torques are inside target * rated as well (batotp_hip_output_stretch_duty)"""
        self.L.need_duty()
        new = self._like()
        report = np.zeros(self.n_paths, dtype=STRETCH_DTYPE)
        rec = np.zeros(self.n_paths, dtype=TSCALE_DTYPE)
        duty = np.zeros(self.n_paths, dtype=DUTY_DTYPE)
        f = (F_HOST_TRIG if host_trig else 0) if flags is None else int(flags)
        self.L.check(self.lib.batotp_hip_output_stretch_duty(self.handle, C.byref(prob), C.byref(model), f, _dptr(self._rated(model, rated)), float(target),
                                                             int(max_rounds), float(max_factor), C.byref(new.handle), report.ctypes.data_as(C.c_void_p),
                                                             rec.ctypes.data_as(C.c_void_p), duty.ctypes.data_as(C.c_void_p)),
                     "batotp_hip_output_stretch_duty")
        new._read_info()
        return new, report, rec, duty

    def duty_ms(self) -> float:
        """milliseconds of the duty kernels of the call that made this Output (duty / stretch_duty), all rounds"""
        self.L.need_duty()
        v = C.c_float(0)
        self.L.check(self.lib.batotp_hip_output_duty_ms(self.handle, C.byref(v)), "output_duty_ms")
        return float(v.value)

    def duty_ranges(self) -> int:
        """launches of the duty kernel (ranges of paths, over all rounds) of the call that made this Output"""
        self.L.need_duty()
        v = C.c_int32(0)
        self.L.check(self.lib.batotp_hip_output_duty_ranges(self.handle, C.byref(v)), "output_duty_ranges")
        return int(v.value)

    def close(self):
        if self.handle:
            self.lib.batotp_hip_output_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self, k: int) -> np.ndarray:
        """[n_theta + n_cart + n_trq][n_pts] of path k of the range"""
        out = np.empty((self.n_rows, int(self.n_pts[k])), dtype=np.float64)
        if out.size:
            self.L.check(self.lib.batotp_hip_output_download(self.handle, k, _dptr(out)), "output_download")
        return out

    def all_rows(self):
        """every path of the range from one device-to-host copy: list of [n_rows][n_pts] arrays"""
        flat = np.empty(int(self.n_pts.sum()) * self.n_rows, dtype=np.float64)
        if flat.size:
            self.L.check(self.lib.batotp_hip_output_download_all(self.handle, _dptr(flat)), "output_download_all")
        out, at = [], 0
        for n in self.n_pts:
            out.append(flat[at: at + int(n) * self.n_rows].reshape(self.n_rows, int(n)))
            at += int(n) * self.n_rows
        return out

    def theta(self, k: int) -> np.ndarray:
        return self.rows(k)[: self.n_theta]

    def ms(self) -> float:
        v = C.c_float(0)
        self.L.check(self.lib.batotp_hip_output_ms(self.handle, C.byref(v)), "output_ms")
        return float(v.value)


def output_from_rows(ctx: "Context", rows_list, sres, n_theta: int, n_cart: int, n_trq: int) -> Output:
    """Output.from_rows"""
    return Output.from_rows(ctx, rows_list, sres, n_theta, n_cart, n_trq)


def fwdkin_chain(ctx: "Context", chain: KinChain, theta_list: Sequence[np.ndarray], host_trig: bool = True):
    """tool points of a ragged set of point lists (batotp_hip_fwdkin_chain): theta_list[p] is [n_links][n_p]; returns a list of
    [3][n_p] arrays.  host_trig: cos / sin from the host libm (bit parity with tests/kin_reference.py), else the device libm"""
    ctx.library.need_kin()
    arrs = [np.ascontiguousarray(t, dtype=np.float64) for t in theta_list]
    for a in arrs:
        assert a.ndim == 2 and a.shape[0] == chain.n_links, (a.shape, chain.n_links)
    n_pts = np.ascontiguousarray([a.shape[1] for a in arrs], dtype=np.int64)
    flat = np.ascontiguousarray(np.concatenate([a.ravel() for a in arrs])) if arrs else np.zeros(0)
    out = np.empty(3 * int(n_pts.sum()), dtype=np.float64)
    ctx.library.check(ctx.library.lib.batotp_hip_fwdkin_chain(ctx.handle, C.byref(chain), F_HOST_TRIG if host_trig else 0, len(arrs),
                                                              n_pts.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(flat), _dptr(out)), "fwdkin_chain")
    res, at = [], 0
    for n in n_pts:
        res.append(out[at: at + 3 * int(n)].reshape(3, int(n)))
        at += 3 * int(n)
    return res


def sdiv_kat(ctx: "Context", a: np.ndarray, b: np.ndarray):
    """(a / b as k_sweep8 divides by a shared reciprocal, which operand pairs went through the reciprocal)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    q = np.empty_like(a); w = np.empty(a.size, dtype=np.int32)
    ctx.library.check(ctx.library.lib.batotp_hip_sdiv_kat(ctx.handle, a.size, _dptr(a), _dptr(b), _dptr(q),
                                                          w.ctypes.data_as(C.POINTER(C.c_int32))), "sdiv_kat")
    return q, w.astype(bool)


def clamp_kat(ctx: "Context", raw, interp, cap, smin, lim1):
    """(literal chain, one-instruction chain, validity flag) of the sweep prologue's clamp chain per operand tuple
    (include/batotp_hip_clamp_kat.h; an entry point of the product library only)"""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (raw, interp, cap, smin, lim1)]
    n = arrs[0].size
    assert all(a.size == n for a in arrs)
    fn = ctx.library.lib.batotp_hip_clamp_kat
    D = C.POINTER(C.c_double)
    fn.argtypes = [C.c_void_p, C.c_int64, D, D, D, D, D, D, D, C.POINTER(C.c_int32)]
    fn.restype = C.c_int
    literal = np.empty(n); fast = np.empty(n); valid = np.empty(n, dtype=np.int32)
    ctx.library.check(fn(ctx.handle, n, *[_dptr(a) for a in arrs], _dptr(literal), _dptr(fast),
                         valid.ctypes.data_as(C.POINTER(C.c_int32))), "clamp_kat")
    return literal, fast, valid.astype(bool)


def out_segmax_kat(ctx: "Context", segs):
    """running maxima of the raw segment indices of several paths (findInterpSegs' cursor), through the output stage's launch function"""
    n1 = np.ascontiguousarray([len(x) for x in segs], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32) for x in segs]), dtype=np.int32)
    ctx.library.check(ctx.library.lib.batotp_hip_out_segmax_kat(ctx.handle, len(segs), n1.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                flat.ctypes.data_as(C.POINTER(C.c_int32))), "out_segmax_kat")
    return np.split(flat, np.cumsum(n1)[:-1])


def spline_lanes_kat(ctx: "Context", y: np.ndarray):
    """second derivatives of one series by the wavefront-per-series solve (+ its fallback) and by the lane-per-series kernel;
    returns (sol, sol_seq, redone)"""
    y = np.ascontiguousarray(y, dtype=np.float64)
    sol, seq = np.empty_like(y), np.empty_like(y)
    redone = C.c_int32(0)
    ctx.library.check(ctx.library.lib.batotp_hip_spline_lanes_kat(ctx.handle, y.size, _dptr(y), _dptr(sol), _dptr(seq), C.byref(redone)),
                      "spline_lanes_kat")
    return sol, seq, int(redone.value)


def div6_kat(ctx: "Context", a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    q = np.empty_like(a)
    ctx.library.check(ctx.library.lib.batotp_hip_div6_kat(ctx.handle, a.size, _dptr(a), _dptr(q)), "div6_kat")
    return q


class Batch:
    """B independent paths resident on one device."""

    def __init__(self, ctx: Context, prob: Problem, n_knots: Sequence[int], max_steps: int):
        self.ctx, self.lib, self.L = ctx, ctx.library.lib, ctx.library
        self.prob = prob
        self.n_knots = np.ascontiguousarray(n_knots, dtype=np.int64)
        self.n_paths = int(self.n_knots.size)
        self.max_steps = int(max_steps)
        self.handle = C.c_void_p()
        self.L.check(self.lib.batotp_hip_batch_create(ctx.handle, C.byref(prob), self.n_paths,
                                                      self.n_knots.ctypes.data_as(C.POINTER(C.c_int64)), self.max_steps,
                                                      C.byref(self.handle)), "batotp_hip_batch_create")

    def close(self):
        if self.handle:
            self.lib.batotp_hip_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- uploads -----------------------------------------------------------------------------
    def upload_knots(self, path0: int, y_list: Sequence[np.ndarray], sres: Sequence[float]):
        """y_list[k]: [n_joints+n_cart][N_k] knot values of path path0+k."""
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(y, dtype=np.float64).ravel() for y in y_list]))
        sr = np.ascontiguousarray(sres, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_knots(self.handle, path0, len(y_list), _dptr(flat), _dptr(sr)), "upload_knots")

    def upload_knots_device(self, path0: int, n: int, dev_ptr: int, sres: Sequence[float]):
        sr = np.ascontiguousarray(sres, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_knots_device(self.handle, path0, n, C.c_void_p(dev_ptr), _dptr(sr)), "upload_knots_device")

    def upload_knots_device_rows(self, path0: int, n: int, dev_ptr: int, src_rows: int, sres: Sequence[float]):
        """paths [path0, path0 + n) from a device block whose paths carry src_rows rows each: the first n_joints + n_cart are taken"""
        sr = np.ascontiguousarray(sres, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_knots_device_rows(self.handle, path0, n, C.c_void_p(dev_ptr), int(src_rows), _dptr(sr)),
                     "upload_knots_device_rows")

    def upload_rr_trig(self, path: int, trig: np.ndarray):
        t = np.ascontiguousarray(trig, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_rr_trig(self.handle, path, _dptr(t)), "upload_rr_trig")

    def set_serial_model(self, model: SerialModel):
        self.L.check(self.lib.batotp_hip_set_serial_model(self.handle, C.byref(model)), "set_serial_model")

    def set_kin_chain(self, chain: KinChain):
        """the kinematic chain whose tool point the output stage puts into the three Cartesian rows of a JOINT path"""
        self.L.need_kin()
        self.L.check(self.lib.batotp_hip_set_kin_chain(self.handle, C.byref(chain)), "set_kin_chain")

    def upload_joint_trig(self, path: int, trig: np.ndarray):
        """trig: [2*n_joints][N] cosines, then sines, of the joint angles (radians) at the knot samples"""
        t = np.ascontiguousarray(trig, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_joint_trig(self.handle, path, _dptr(t)), "upload_joint_trig")

    def upload_path_sites(self, path: int, sites: np.ndarray, vfact: float, afact: float, parallel_now: int):
        s = np.ascontiguousarray(sites, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_path_sites(self.handle, path, _dptr(s), vfact, afact, parallel_now), "upload_path_sites")

    def upload_coeffs(self, path: int, channel: int, c: np.ndarray):
        a = np.ascontiguousarray(c, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_coeffs(self.handle, path, channel, _dptr(a)), "upload_coeffs")

    def upload_curve(self, path: int, s: np.ndarray, sdot: np.ndarray):
        a = np.ascontiguousarray(s, dtype=np.float64)
        b = np.ascontiguousarray(sdot, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_curve(self.handle, path, _dptr(a), _dptr(b), a.size), "upload_curve")

    def upload_forward_curve(self, path: int, s: np.ndarray, sdot: np.ndarray, t_total: float):
        a = np.ascontiguousarray(s, dtype=np.float64)
        b = np.ascontiguousarray(sdot, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_upload_forward_curve(self.handle, path, _dptr(a), _dptr(b), a.size, float(t_total)), "upload_forward_curve")

    def set_path_integ_res(self, path0: int, integ_res):
        v = np.ascontiguousarray(integ_res, dtype=np.float64)
        self.L.check(self.lib.batotp_hip_set_path_integ_res(self.handle, path0, v.size, _dptr(v)), "set_path_integ_res")

    # ---- hot path ----------------------------------------------------------------------------
    def precompute(self, stage: int = 0):
        self.L.check(self.lib.batotp_hip_precompute(self.handle, stage), "precompute")

    def pointwise_mvc(self):
        self.L.check(self.lib.batotp_hip_pointwise_mvc(self.handle), "pointwise_mvc")

    def sweep(self, direction: int):
        self.L.check(self.lib.batotp_hip_sweep(self.handle, direction), "sweep")

    def optimize(self):
        self.L.check(self.lib.batotp_hip_optimize(self.handle), "optimize")

    def spline_tile_fallbacks(self) -> int:
        n = C.c_int32(0)
        self.L.check(self.lib.batotp_hip_spline_tile_fallbacks(self.handle, C.byref(n)), "spline_tile_fallbacks")
        return n.value

    def last_sweep_launch(self, direction: int):
        """(lanes per path, paths per wavefront, hold of the flat loop or -1 for the nested loops) of the last launch"""
        lanes, ppw, hold = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.L.check(self.lib.batotp_hip_last_sweep_launch(self.handle, direction, C.byref(lanes), C.byref(ppw), C.byref(hold)), "last_sweep_launch")
        return lanes.value, ppw.value, hold.value

    # ---- results -----------------------------------------------------------------------------
    def results(self) -> np.ndarray:
        out = np.zeros(self.n_paths, dtype=RESULT_DTYPE)
        self.L.check(self.lib.batotp_hip_get_results(self.handle, out.ctypes.data_as(C.c_void_p)), "get_results")
        return out

    def curve(self, path: int, which: int):
        n = C.c_int64(0)
        self.L.check(self.lib.batotp_hip_download_curve(self.handle, path, which, None, None, 0, C.byref(n)), "download_curve")
        s = np.empty(max(n.value, 0)); sd = np.empty(max(n.value, 0))
        if n.value > 0:
            self.L.check(self.lib.batotp_hip_download_curve(self.handle, path, which, _dptr(s), _dptr(sd), n.value, C.byref(n)), "download_curve")
        return s, sd

    def coeffs(self, path: int, channel: int) -> np.ndarray:
        out = np.empty((4, int(self.n_knots[path])))
        self.L.check(self.lib.batotp_hip_download_coeffs(self.handle, path, channel, _dptr(out)), "download_coeffs")
        return out

    def samples(self, path: int, channel: int) -> np.ndarray:
        out = np.empty((3, int(self.n_knots[path])))
        self.L.check(self.lib.batotp_hip_download_samples(self.handle, path, channel, _dptr(out)), "download_samples")
        return out

    def dyn(self, path: int, k: int, row: int) -> np.ndarray:
        out = np.empty(int(self.n_knots[path]))
        self.L.check(self.lib.batotp_hip_download_dyn(self.handle, path, k, row, _dptr(out)), "download_dyn")
        return out

    def mvc(self, path: int):
        n = int(self.n_knots[path])
        a, b, c = np.empty(n), np.empty(n), np.empty(n)
        self.L.check(self.lib.batotp_hip_download_mvc(self.handle, path, _dptr(a), _dptr(b), _dptr(c)), "download_mvc")
        return a, b, c

    def pack_curves(self, which: int, path0: int, n_paths: int, dst_ptr: int, dst_points: int) -> int:
        """curves of paths [path0, path0 + n_paths) packed as (s, sdot) pairs into memory of the library's device at dst_ptr;
        returns the number of pairs (call with dst_ptr = 0, dst_points = 0 to size the buffer when no curve is empty ...
        sizes also follow from results()['n_fwd' / 'n_rev'])"""
        total = C.c_int64(0)
        self.L.check(self.lib.batotp_hip_pack_curves(self.handle, which, path0, n_paths, C.c_void_p(dst_ptr), dst_points, C.byref(total)), "pack_curves")
        return int(total.value)

    def results_device_ptr(self):
        ptr, nbytes = C.c_void_p(), C.c_int64(0)
        self.L.check(self.lib.batotp_hip_results_device_ptr(self.handle, C.byref(ptr), C.byref(nbytes)), "results_device_ptr")
        return ptr.value, nbytes.value

    def kernel_ms(self, which: int) -> float:
        ms = C.c_float(0)
        self.L.check(self.lib.batotp_hip_last_kernel_ms(self.handle, which, C.byref(ms)), "last_kernel_ms")
        return float(ms.value)

    def nbytes(self) -> int:
        n = C.c_int64(0)
        self.L.check(self.lib.batotp_hip_batch_bytes(self.handle, C.byref(n)), "batch_bytes")
        return n.value


_hip_library: Optional[Library] = None


def load_hip() -> Library:
    """The product library.  Raises BatotpError when it has not been built."""
    global _hip_library
    if _hip_library is None:
        _hip_library = Library(HIP_LIB_PATH)
    return _hip_library
