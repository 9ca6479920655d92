#!/usr/bin/env python3
"""Measure the torque rows for finished trajectories (batotp_hip_output_torques) on real and synthetic outputs.

Every figure is the MEDIAN of the HIP-event times (Output.torques_ms: the kernels of one call) of --repeats calls after three
warm-up calls.  Measured in the same run on the same rows: a device-to-device hipMemcpy of the rows, and for the real batch the
output stage that produced them (Output.ms).

  real       --real-copies copies of the output of synth_ur_s7_100k (6 joint rows) with a 6-link model: the nominal UR chain
             (axes and offsets of the built-in kinematic chain) with made-up inertial parameters
  synthetic  a quarter of the audit benchmark's batch: 256 paths x 200000 points x 7 joint rows, built-in KUKA model

Both with the device libm (the kernel alone) and with host trig tables (kernel + the packing kernel; the host's share of that
route -- copies and libm -- is reported as wall clock beside it).

    python tools/invdyn_bench.py [--scale 1.0] [--repeats 15] [--out profiles/invdyn_bench.txt]

--scale multiplies the number of paths of the synthetic batch.  Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from batotp_amd import capi  # noqa: E402
from audit_bench import Hip, device_rows  # noqa: E402


def ur_model(lib):
    """nominal UR chain, inertial parameters made up (masses of a few kg, centres of mass a few cm out, small inertia tensors)"""
    ch = lib.builtin_kin_chain(capi.ROBOT_UR)
    m = capi.SerialModel()
    m.n_links, m.degrees = ch.n_links, ch.degrees
    m.gravity[2] = -9.81
    rng = np.random.default_rng(3)
    for i in range(ch.n_links):
        L = m.link[i]
        for j in range(3):
            L.axis[j], L.off[j], L.com[j] = ch.axis[i][j], ch.off[i][j], float(rng.uniform(-0.05, 0.05))
        L.mass, L.fv = float(rng.uniform(1.0, 8.0)), float(rng.uniform(0.1, 1.0))
        for j, v in enumerate((0.02, 0.02, 0.01, 0.001, -0.001, 0.002)):
            L.inertia[j] = v
    return m


def torques_median(out, model, host_trig, repeats, warm=3):
    ms, wall = [], []
    for it in range(warm + repeats):
        t0 = time.perf_counter()
        new = out.torques(model, host_trig=host_trig)
        t1 = time.perf_counter()
        if it >= warm:
            ms.append(new.torques_ms()); wall.append((t1 - t0) * 1e3)
        ranges = new.torques_ranges()
        new.close()
    return statistics.median(ms), min(ms), max(ms), statistics.median(wall), ranges


def report(lines, tag, out, model, hip, repeats, out_ms=None):
    pts, rows_in = int(out.n_pts.sum()), out.n_rows
    src, doubles = device_rows(out)
    copy = hip.copy_ms(src, doubles * 8, repeats)
    lines.append(f"copy    {tag}: {copy:.3f} ms, {pts / copy * 1e3:.4g} points/s (device-to-device hipMemcpy of the {rows_in} input rows)")
    for host_trig in (False, True):
        # (a call with host tables spends seconds on the host for a batch of this size: fewer of them)
        few = host_trig and pts > 10_000_000
        med, lo, hi, wall, ranges = torques_median(out, model, host_trig, 5 if few else repeats, 1 if few else 3)
        what = ("host trig tables" + (" (median of 5 after 1)" if few else "")) if host_trig else "device libm"
        ln = (f"torques {tag}, {what}: kernels {med:.3f} ms (min {lo:.3f}, max {hi:.3f}), {pts / med * 1e3:.4g} points/s, "
              f"{ranges} range(s), call wall clock {wall:.1f} ms; kernels / copy = {med / copy:.2f}")
        if out_ms is not None:
            ln += f"; output stage (batotp_hip_output_ms) {out_ms:.3f} ms; kernels / output stage = {med / out_ms:.4f}"
        lines.append(ln)
    for ln in lines[-3:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--real-copies", type=int, default=32)
    args = ap.parse_args()
    assert args.repeats >= 10
    lib = capi.load_hip()
    ctx = capi.Context(lib, 0)
    hip = Hip()
    lines = [f"invdyn_bench: scale {args.scale}, median of {args.repeats} calls after 3 warm-up calls, HIP events; block {capi.INVDYN_BLOCK_POINTS} points"]

    # the real batch: output stage and torque rows of the same trajectories
    import helpers
    case = helpers.Case("synth_ur_s7_100k")
    k = args.real_copies
    b = capi.Batch(ctx, case.problem, [case.n] * k, case.max_steps())
    b.upload_knots(0, [case.y] * k, [case.sres] * k)
    b.optimize()
    prm = capi.OutputParams(case.problem.n_joints, capi.PATH_JOINT, case.problem.integ_res, 0.008, 5.0)
    out = capi.Output(b, prm, 0, k)
    tag = f"{k} copies of synth_ur_s7_100k, {int(out.n_pts.sum())} output points x {out.n_theta}+{out.n_cart} rows, 6-link model"
    report(lines, tag, out, ur_model(lib), hip, args.repeats, out.ms())
    out.close(); b.close()

    # the synthetic batch: a smooth random trajectory per row, the same rows for every path (the kernel's work does not depend on the values)
    paths, n, nt = max(1, int(round(256 * args.scale))), 200_000, 7
    rng = np.random.default_rng(1)
    t = np.arange(n) * 0.008
    one = np.ascontiguousarray(np.stack([np.sin(t * rng.uniform(0.2, 2.0) + rng.uniform(0, 6)) * rng.uniform(20.0, 90.0) for _ in range(nt)]))
    out = capi.output_from_rows(ctx, [one] * paths, 0.008, nt, 0, 0)
    report(lines, f"{paths} paths x {n} points x {nt} rows, built-in KUKA model", out, lib.builtin_serial_model(capi.ROBOT_KUKA), hip, args.repeats)
    out.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
