#!/usr/bin/env python3
"""Measure the time stretch of finished trajectories (batotp_hip_output_stretch_by) on synthetic outputs.

For every size and factor the script builds an output through capi.output_from_rows, stretches it a few times to warm up and reports
the MEDIAN of the HIP-event times (Output.stretch_ms: the stretch kernel of the call) of --repeats stretches.  The yardstick is measured
in the same run: a device-to-device hipMemcpy of the RESULT's bytes, which reads and writes as many bytes as the kernel writes (the
kernel reads 1 / factor of that).  Every line carries milliseconds, new points/s and GB/s of the 8 * rows * new points bytes written.

    python tools/stretch_bench.py [--scale 1.0] [--repeats 15] [--out profiles/stretch_bench.txt]

--scale multiplies the number of paths of every size.  Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from batotp_amd import capi  # noqa: E402
from audit_bench import Hip, device_rows  # noqa: E402

SIZES = [  # (paths, points per path, joint rows): the batches of profiles/audit_bench.txt
    (256, 200_000, 7),
    (4096, 10_000, 7),
]
FACTORS = [1.05, 2.0]


def stretch_median(out, factor, repeats):
    times = []
    for it in range(3 + repeats):
        new = out.stretch_by(factor)
        if it >= 3:
            times.append(new.stretch_ms())
        if it + 1 < 3 + repeats:
            new.close()
    return statistics.median(times), min(times), max(times), new


def line(tag, ms, points, rows):
    return f"{tag}: {ms:.3f} ms, {points / ms * 1e3:.4g} new points/s, {8.0 * rows * points / ms / 1e6:.1f} GB/s written"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 10
    ctx = capi.Context(capi.load_hip(), 0)
    hip = Hip()
    lines = [f"stretch_bench: scale {args.scale}, median of {args.repeats} stretches after 3 warm-up stretches, HIP events; "
             f"block {capi.STRETCH_BLOCK_POINTS} new points"]
    rng = np.random.default_rng(1)
    for paths, n, R in SIZES:
        paths = max(1, int(round(paths * args.scale)))
        # a smooth random trajectory per row, the same rows for every path: the kernel's work does not depend on the values
        t = np.arange(n) * 0.008
        one = np.ascontiguousarray(np.stack([np.sin(t * rng.uniform(0.2, 2.0) + rng.uniform(0, 6)) * rng.uniform(0.2, 1.0) for _ in range(R)]))
        out = capi.output_from_rows(ctx, [one] * paths, 0.008, R, 0, 0)
        for factor in FACTORS:
            med, lo, hi, new = stretch_median(out, factor, args.repeats)
            n2 = int(new.n_pts[0])
            dst, doubles = device_rows(new)
            assert doubles == paths * n2 * R and new.stretch_ranges() == 1
            copy = hip.copy_ms(dst, doubles * 8, args.repeats)
            tag = f"{paths} paths x {n} -> {n2} points x {R} rows (factor {factor})"
            lines.append(line(f"stretch {tag}", med, paths * n2, R) + f" (min {lo:.3f}, max {hi:.3f})")
            lines.append(line(f"copy    {tag}", copy, paths * n2, R) + " (device-to-device hipMemcpy of the result's bytes: reads AND writes them)")
            lines.append(f"ratio   {tag}: stretch / copy = {med / copy:.3f}")
            new.close()
            for ln in lines[-3:]:
                print(ln, flush=True)
        out.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
