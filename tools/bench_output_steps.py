#!/usr/bin/env python3
"""Times the output stage (batotp_hip_output) on ranges whose paths integrate with different steps, and the uniform-step call
that must not pay for it (profiles/output_per_path_steps.txt).

    python tools/bench_output_steps.py --mode one-call   [--lib PATH]   one per-path-mode call (+ output_info) for the range
    python tools/bench_output_steps.py --mode per-path   [--lib PATH]   one positive-integ_res call (+ output_info) per path
    python tools/bench_output_steps.py --mode uniform    [--lib PATH]   batotp_hip_output_ms of a uniform-step call

--lib names another build of the product library (e.g. the parent commit's, which knows the last two modes only).  one-call /
per-path: --paths copies of synth_gen7dof_s0[:400] with as many distinct steps h (0.6 + 1.4 k / paths); wall time around the
calls, --runs runs after one warm-up run that fills the context's workspace.  uniform: --paths copies of synth_ur_s7_100k,
out_res 0.008, smoothing 5.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import helpers  # noqa: E402
from batotp_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["one-call", "per-path", "uniform"], required=True)
ap.add_argument("--lib", default=None)
ap.add_argument("--paths", type=int, default=None)
ap.add_argument("--runs", type=int, default=5)
a = ap.parse_args()

lib = capi.Library(a.lib) if a.lib else capi.load_hip()
ctx = capi.Context(lib, 0)

if a.mode == "uniform":
    K = a.paths or 256
    case = helpers.Case("synth_ur_s7_100k")
    h = case.problem.integ_res
    b = capi.Batch(ctx, case.problem, [case.n] * K, case.max_steps())
    for k in range(K):
        b.upload_knots(k, [case.y], [case.sres])
    b.optimize()
    prm = capi.OutputParams(case.problem.n_joints, capi.PATH_JOINT, h, 0.008, 5.0)
    ms = []
    for _ in range(a.runs + 1):
        o = capi.Output(b, prm, 0, K)
        ms.append(o.ms())
        pts = int(o.n_pts.sum())
        o.close()
    print(json.dumps({"mode": a.mode, "lib": a.lib or "this tree", "paths": K, "points": pts, "warmup_ms": ms[0], "runs_ms": ms[1:],
                      "median_ms": statistics.median(ms[1:]), "slowest_ms": max(ms[1:])}))
    sys.exit(0)

K = a.paths or 512
case = helpers.Case("synth_gen7dof_s0")
h = case.problem.integ_res
y = np.ascontiguousarray(case.y[:, :400])
steps = [h * (0.6 + 1.4 * k / K) for k in range(K)]
assert len(set(steps)) == K
b = capi.Batch(ctx, case.problem, [400] * K, case.max_steps())
for k in range(K):
    b.upload_knots(k, [y], [case.sres])
b.set_path_integ_res(0, steps)
b.optimize()
base = helpers.output_params(case.name)
wall, pts = [], 0
for _ in range(a.runs + 1):
    t0 = time.perf_counter()
    if a.mode == "one-call":
        o = capi.Output(b, base, 0, K, per_path_steps=True)     # the constructor also calls batotp_hip_output_info
        pts = int(o.n_pts.sum())
        o.close()
    else:
        pts = 0
        for k in range(K):
            o = capi.Output(b, capi.OutputParams(base.n_joints, base.path_type, steps[k], base.out_res, base.out_smooth_fact), k, 1)
            pts += int(o.n_pts[0])
            o.close()
    wall.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({"mode": a.mode, "lib": a.lib or "this tree", "paths": K, "points": pts, "out_res": base.out_res, "smooth": base.out_smooth_fact,
                  "warmup_ms": wall[0], "runs_ms": wall[1:], "median_ms": statistics.median(wall[1:])}))
