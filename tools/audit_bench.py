#!/usr/bin/env python3
"""Measure the trajectory audit (batotp_hip_output_audit) on synthetic outputs.

For every size the script builds an output through capi.output_from_rows, audits it a few times to warm up and reports the MEDIAN of
the HIP-event times (Output.audit_ms: the two kernels of an audit) of --repeats audits.  The yardstick is measured in the same run on
the same rows: a device-to-device hipMemcpy of them, which reads and writes the bytes the audit only reads.  Every line carries
milliseconds, points/s and GB/s of the 8 * rows * points bytes.  A last line puts the audit of a real batch (copies of a golden path
through sweeps and output stage) beside the time of that batch's output stage (Output.ms).

    python tools/audit_bench.py [--scale 1.0] [--repeats 15] [--out profiles/audit_bench.txt]

--scale multiplies the number of paths of every size (the rows of a full-size output are tens of GB of host memory on their way in).
Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from batotp_amd import capi  # noqa: E402

SIZES = [  # (paths, points per path, joint rows, Cartesian rows, torque rows)
    (1024, 200_000, 7, 0, 0),
    (1024, 200_000, 7, 3, 3),
    (16384, 10_000, 7, 0, 0),
]


def problem(n_theta, n_cart):
    flags = capi.F_JNT_ACC_ON | capi.F_PARALLEL
    if n_cart:
        flags |= capi.F_TRQ_ON | capi.F_CART_VEL_ON | capi.F_CART_ACC_ON
    return capi.make_problem(n_theta, n_cart, capi.ROBOT_CSPR3DOF if n_cart else capi.ROBOT_GENJNT, flags,
                             jnt_vel_max=[2.0] * n_theta, jnt_acc_max=[40.0] * n_theta, jnt_trq_max=[12.0] * 3, jnt_trq_min=[1.0] * 3,
                             cart_vel_max=1.5, cart_acc_max=30.0)


class Hip:
    """the HIP runtime the library is bound to, for the copy that serves as yardstick"""

    def __init__(self):
        h = self.h = C.CDLL("libamdhip64.so.7", mode=os.RTLD_NOLOAD | os.RTLD_NOW)
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        h.hipEventSynchronize.argtypes = [C.c_void_p]
        h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        h.hipEventDestroy.argtypes = [C.c_void_p]
        h.hipDeviceSynchronize.argtypes = []

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with HIP error {rc}")

    def copy_ms(self, src, nbytes, repeats):
        dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.check(self.h.hipMalloc(C.byref(dst), nbytes), "hipMalloc")
        self.check(self.h.hipEventCreate(C.byref(e0)), "hipEventCreate")
        self.check(self.h.hipEventCreate(C.byref(e1)), "hipEventCreate")
        times = []
        for it in range(3 + repeats):
            self.check(self.h.hipDeviceSynchronize(), "hipDeviceSynchronize")
            self.check(self.h.hipEventRecord(e0, None), "hipEventRecord")
            self.check(self.h.hipMemcpy(dst, C.c_void_p(src), nbytes, 3), "hipMemcpy (device to device)")
            self.check(self.h.hipEventRecord(e1, None), "hipEventRecord")
            self.check(self.h.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float(0)
            self.check(self.h.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            if it >= 3:
                times.append(float(ms.value))
        self.h.hipEventDestroy(e0); self.h.hipEventDestroy(e1); self.h.hipFree(dst)
        return statistics.median(times)


def device_rows(out):
    ptr, cnt = C.c_void_p(), C.c_int64(0)
    out.L.check(out.lib.batotp_hip_output_device(out.handle, C.byref(ptr), C.byref(cnt)), "output_device")
    return ptr.value, int(cnt.value)


def audit_median(out, prob, repeats):
    for _ in range(3):
        a = out.audit(prob, 0.05)
    times = []
    for _ in range(repeats):
        out.audit(prob, 0.05)
        times.append(out.audit_ms())
    return statistics.median(times), min(times), max(times), a


def line(tag, ms, points, rows):
    return f"{tag}: {ms:.3f} ms, {points / ms * 1e3:.4g} points/s, {8.0 * rows * points / ms / 1e6:.1f} GB/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--real-copies", type=int, default=32)
    args = ap.parse_args()
    assert args.repeats >= 10
    ctx = capi.Context(capi.load_hip(), 0)
    hip = Hip()
    lines = [f"audit_bench: scale {args.scale}, median of {args.repeats} audits after 3 warm-up audits, HIP events; block {capi.AUDIT_BLOCK_POINTS} points"]
    rng = np.random.default_rng(1)
    for paths, n, nt, nc, nq in SIZES:
        paths = max(1, int(round(paths * args.scale)))
        R = nt + nc + nq
        # a smooth random trajectory per row (utilisations below and around 1), the same rows for every path: the kernel's work does not
        # depend on the values
        t = np.arange(n) * 0.008
        one = np.ascontiguousarray(np.stack([np.sin(t * rng.uniform(0.2, 2.0) + rng.uniform(0, 6)) * rng.uniform(0.2, 1.0) for _ in range(R)]))
        if nq:
            one[nt + nc:] = 6.5 + 5.0 * one[nt + nc:]
        out = capi.output_from_rows(ctx, [one] * paths, 0.008, nt, nc, nq)
        prob = problem(nt, nc)
        med, lo, hi, a = audit_median(out, prob, args.repeats)
        src, doubles = device_rows(out)
        assert doubles == paths * n * R
        copy = hip.copy_ms(src, doubles * 8, args.repeats)
        tag = f"{paths} paths x {n} points x {R} rows ({nt}+{nc}+{nq})"
        lines.append(line(f"audit   {tag}", med, paths * n, R) + f" (min {lo:.3f}, max {hi:.3f})")
        lines.append(line(f"copy    {tag}", copy, paths * n, R) + " (device-to-device hipMemcpy of the same rows: reads AND writes them)")
        lines.append(f"ratio   {tag}: audit / copy = {med / copy:.3f}; worst peaks " +
                     " ".join(f"{name} {float(a['fam'][:, f]['peak'].max()):.3f}" for f, name in enumerate(capi.AUDIT_FAMILIES)))
        out.close()
        for ln in lines[-3:]:
            print(ln, flush=True)
    # a real batch: output stage and audit of the same trajectories
    import helpers
    case = helpers.Case("synth_ur_s7_100k")
    k = args.real_copies
    b = capi.Batch(ctx, case.problem, [case.n] * k, case.max_steps())
    b.upload_knots(0, [case.y] * k, [case.sres] * k)
    b.optimize()
    prm = capi.OutputParams(case.problem.n_joints, capi.PATH_JOINT, case.problem.integ_res, 0.008, 5.0)
    out = capi.Output(b, prm, 0, k)
    out_ms = out.ms()
    med, lo, hi, a = audit_median(out, case.problem, args.repeats)
    pts = int(out.n_pts.sum())
    lines.append(line(f"real    {k} copies of synth_ur_s7_100k, {pts} output points x {out.n_rows} rows: audit", med, pts, out.n_rows) +
                 f"; output stage (batotp_hip_output_ms) {out_ms:.3f} ms; audit / output stage = {med / out_ms:.4f}")
    print(lines[-1], flush=True)
    out.close(); b.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
