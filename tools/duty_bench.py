#!/usr/bin/env python3
"""k_duty beside k_tscale of the same build on the same rows (HIP-event times, alternating in one process).

    python tools/duty_bench.py [--paths 64] [--reps 15]

The shapes of tools/tscale_bench.py: the rows are the output of synth_gen7dof_s0 through the device pipeline (7402 points, 7 joint
rows), tiled to --paths paths; the model is the built-in KUKA table; the torque range is +-(1.05 max|G| + 0.5 max|A + B| + 1e-3) of
the rows' own torques; the ratings are the rows' own RMS torques over 1.3, and no less than 1.25 times gravity's.
tscale_ms: k_tscale + k_tscale_finish (+ k_invdyn_pack with host tables).  duty_ms: k_duty + k_tscale_finish + k_duty_finish
(+ k_invdyn_pack): what a round of batotp_hip_output_stretch_duty launches in place of the former."""
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
    rated = np.maximum(np.sqrt((tau * tau).mean(axis=1)) / 1.3, 1.25 * np.sqrt((grav * grav).mean(axis=1))) + 1e-3
    big = capi.output_from_rows(ctx, [rows] * a.paths, [sres] * a.paths, nl, n_cart, 0)
    pts = rows.shape[1] * a.paths
    for host_trig in (False, True):
        t_ts, t_du = [], []
        for rep in range(a.reps + 1):
            o1, rec = big.torque_scale(prob, model, 1.0, host_trig=host_trig)
            o2, duty = big.duty(model, rated, 1.0, host_trig=host_trig)
            if rep:                                        # the first pair warms up
                t_ts.append(o1.tscale_ms()); t_du.append(o2.duty_ms())
            o1.close(); o2.close()
        mt, md = statistics.median(t_ts), statistics.median(t_du)
        print(f"DUTY bench: {a.paths} paths x {rows.shape[1]} points x {nl} joint rows (+{n_cart} Cartesian), {'host trig tables' if host_trig else 'device libm'}: "
              f"k_tscale + finish {mt:.4f} ms [{min(t_ts):.4f} .. {max(t_ts):.4f}], k_duty + finishes {md:.4f} ms [{min(t_du):.4f} .. {max(t_du):.4f}], "
              f"ratio {md / mt:.3f}; {pts / md * 1e-6:.2f}e9 points/s; util of path 0 {float(duty[0]['util']):.6f} (joint {int(duty[0]['row'])}), "
              f"s {float(duty[0]['s']):.6f}, energy {float(duty[0]['energy']):.4f} J, peak power {float(duty[0]['peak_power']):.4f} W")
    big.close(); out.close(); b.close()


if __name__ == "__main__":
    main()
