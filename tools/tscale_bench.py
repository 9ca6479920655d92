#!/usr/bin/env python3
"""k_tscale beside k_invdyn of the same build on the same rows (HIP-event times, alternating in one process).

    python tools/tscale_bench.py [--paths 64] [--reps 15]

The rows are the output of synth_gen7dof_s0 through the device pipeline (7402 points, 7 joint rows), tiled to --paths paths; the
model is the built-in KUKA table; the torque range is +-(1.05 max|G| + 0.5 max|A + B| + 1e-3) of the rows' own torques (it binds, and gravity stays inside).
torques_ms: k_invdyn (+ k_invdyn_pack with host tables).  tscale_ms: k_tscale + k_tscale_finish (+ k_invdyn_pack)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
from batotp_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    lib = capi.load_hip()
    ctx = capi.Context(lib, 0)
    case = helpers.Case("synth_gen7dof_s0")
    out, b = helpers.run_to_output(ctx, [case])
    model = lib.builtin_serial_model(capi.ROBOT_KUKA)
    nl = model.n_links
    rows = out.rows(0)
    sres = float(out.sres[0])
    n_cart = out.n_cart
    tau = out.torques(model, host_trig=False).rows(0)[nl + n_cart:]
    # the same samples at a time step of 1e6 s stand still: their torques are gravity's
    still = capi.output_from_rows(ctx, [rows], [1e6], nl, n_cart, 0)
    grav = still.torques(model, host_trig=False).rows(0)[nl + n_cart:]
    still.close()
    limit = 1.05 * np.abs(grav).max(axis=1) + 0.5 * np.abs(tau - grav).max(axis=1) + 1e-3
    prob = capi.Problem.from_buffer_copy(bytes(case.problem))
    for j in range(nl):
        prob.jnt_trq_max[j], prob.jnt_trq_min[j] = float(limit[j]), -float(limit[j])
    big = capi.output_from_rows(ctx, [rows] * a.paths, [sres] * a.paths, nl, n_cart, 0)
    pts = rows.shape[1] * a.paths
    for host_trig in (False, True):
        t_inv, t_ts = [], []
        for rep in range(a.reps + 1):
            o1 = big.torques(model, host_trig=host_trig)
            o2, rec = big.torque_scale(prob, model, 1.0, host_trig=host_trig)
            if rep:                                        # the first pair warms up
                t_inv.append(o1.torques_ms()); t_ts.append(o2.tscale_ms())
            o1.close(); o2.close()
        mi, mt = statistics.median(t_inv), statistics.median(t_ts)
        print(f"TSCALE bench: {a.paths} paths x {rows.shape[1]} points x {nl} joint rows (+{n_cart} Cartesian), {'host trig tables' if host_trig else 'device libm'}: "
              f"k_invdyn {mi:.4f} ms [{min(t_inv):.4f} .. {max(t_inv):.4f}], k_tscale + finish {mt:.4f} ms [{min(t_ts):.4f} .. {max(t_ts):.4f}], "
              f"ratio {mt / mi:.3f}; {pts / mt * 1e-6:.2f}e9 points/s; s of path 0 {float(rec[0]['s']):.6f}, static points {int(rec[0]['n_static'])}")
    big.close(); out.close(); b.close()


if __name__ == "__main__":
    main()
