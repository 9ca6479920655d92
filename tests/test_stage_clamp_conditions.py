"""CPU, with the oracle: the headline workload runs the one-instruction clamp chain of the sweep prologue throughout
(batotp_amd/csrc/device_math.h, clamp_chain_fast: valid while sdotMin > 0, sdotCap and the floor are no NaNs and neither raw value of a
stage is a NaN).

For the first four seeds of the headline configuration (bench_seeds("fill7", 0, 1)) at a reduced knot count, through the oracle's
resampler and the oracle's sweeps:
  * the bootstrap's sdotMin is positive in both directions.  Point 0 of a curve is (s, sdotMin): the bootstrap's second pass starts from
    sdotMin and clamps it into [sdotMin, limits], so the published value is sdotMin itself;
  * sdotCap = s_end / h and the floor 0 / h are finite numbers;
  * no published stage value is a NaN or an infinity in either direction, and no sweep reports BATOTP_ST_NONFINITE.  The published
    points are the sixth stage values of every step; the clamp chain hands a NaN raw value through to its result and the tableau
    combination hands a NaN stage value on to every later stage of its step (0 * NaN is a NaN), so a NaN in any stage would show in
    the point the step publishes;
  * the reverse curve the forward sweep interpolates on has strictly increasing positions and finite speeds, so the interpolation
    mD0 + tauM (mD1 - mD0) divides by a positive number and is no NaN.
The per-stage values themselves are not part of the library's interface; what is asserted is what makes them ordinary numbers."""
import numpy as np

import bench
from batotp_amd import capi
from test_gpu_sweep8_lockstep import _run

KNOTS = 3000     # instead of the headline's 100 000


def test_headline_seeds_run_the_fast_clamp_chain(oracle_ctx):
    seeds = bench.bench_seeds("fill7", 0, 1)[:4]
    assert len(seeds) == 4
    for seed in seeds:
        y, sres, prob, _ = bench.make_knots("gen7", seed, KNOTS, tool=bench.ORACLE_KNOTS)
        n = y.shape[1]
        h = float(prob.integ_res)
        s_end = sres * (n - 1)
        assert h > 0 and np.isfinite(s_end / h) and (0.0 / h) == 0.0
        res, rev, fwd, _ = _run(oracle_ctx, prob, [y], [sres], int(bench.WORKLOADS["gen7"]["cap"] * n) + 64)
        assert int(res["status_rev"][0]) == 0 and int(res["status_fwd"][0]) == 0, (seed, res[0])
        (s_r, v_r), (s_f, v_f) = rev[0], fwd[0]
        assert len(v_r) > 100 and len(v_f) > 100, (seed, len(v_r), len(v_f))
        # the bootstrap's sdotMin of both directions: the reverse sweep starts at the end of the path, its point 0 is the curve's last one
        assert v_f[0] > 0.0 and v_r[-1] > 0.0, (seed, v_f[0], v_r[-1])
        for a in (s_r, v_r, s_f, v_f):
            assert np.isfinite(a).all(), seed
        assert np.all(np.diff(s_r) > 0.0), seed
