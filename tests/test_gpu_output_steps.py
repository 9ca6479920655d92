"""GPU (-m gpu): the output stage on a range whose paths integrate with different steps, in ONE call
(OutputParams.integ_res == capi.OUT_STEP_PER_PATH; capi.Output(..., per_path_steps=True)).

Expected values come from the CPU checker, which serves one step per call: the same batch with the same steps
(set_path_integ_res) is swept there and capi.Output is called once per path with integ_res = that path's step.  As a
second check the device's own one-path calls through the unchanged positive-integ_res route must give the same bytes
as its single per-path-mode call.  Tolerance 0 everywhere: counts and sres by ==, rows bit for bit."""
import numpy as np
import pytest

import helpers
from helpers import Case, assert_bit_equal, output_params
from batotp_amd import capi

pytestmark = pytest.mark.gpu

COMPACT = capi.F_NO_SAMPLES | capi.F_COMPACT_SPLINES


def swept_batch(ctx, prob, ys, sres, steps, cap, trig=False):
    """knots -> per-path steps -> both sweeps on the library behind ctx"""
    b = capi.Batch(ctx, prob, [y.shape[1] for y in ys], cap)
    for k, y in enumerate(ys):
        b.upload_knots(k, [np.ascontiguousarray(y)], [sres])
    b.set_path_integ_res(0, list(steps))
    if trig:
        helpers.precompute_with_trig(ctx, b, prob, len(ys))
    else:
        b.precompute(1)
    b.sweep(-1); b.sweep(+1)
    return b


def params(base, integ_res, out_res, smooth):
    return capi.OutputParams(base.n_joints, base.path_type, integ_res, out_res, smooth)


def reinterpolated(steps, out_res):
    """the paths whose output is sampled finer than they integrate (reference ba.cpp:1668-1675)"""
    return [out_res < h for h in steps]


class Expected:
    """per-path results of the checker for one swept batch, computed once per (out_res, smoothing factor) and left unchanged"""

    def __init__(self, batch, base, steps):
        self.batch, self.base, self.steps, self.cache = batch, base, list(steps), {}

    def get(self, out_res, smooth):
        key = (out_res, smooth)
        if key not in self.cache:
            rows = []
            for k, h in enumerate(self.steps):
                if not h > 0:      # NaN: the checker refuses the value as a step of a call; such a path has no trajectory
                    rows.append((0, None, None))
                    continue
                o = capi.Output(self.batch, params(self.base, h, out_res, smooth), k, 1)
                rows.append((int(o.n_pts[0]), float(o.sres[0]), o.rows(0)))
                rows[-1][2].setflags(write=False)
                self.channels = (o.n_theta, o.n_cart, o.n_trq)
                o.close()
            self.cache[key] = rows
        return self.cache[key]


def check_range(hb, exp, out_res, smooth, path0=0, n_paths=None, what=""):
    """one per-path-mode call on [path0, path0 + n_paths) against the checker's per-path calls and the device's own"""
    steps, base = exp.steps, exp.base
    n_paths = len(steps) - path0 if n_paths is None else n_paths
    want = exp.get(out_res, smooth)
    got = capi.Output(hb, params(base, 12345.0, out_res, smooth), path0, n_paths, per_path_steps=True)
    assert (got.n_theta, got.n_cart, got.n_trq) == exp.channels, what
    every = got.all_rows()
    assert len(every) == n_paths
    for k in range(n_paths):
        n, sres, rows = want[path0 + k]
        tag = f"{what} out_res={out_res} smooth={smooth} range=({path0},{n_paths}) path {path0 + k}"
        assert int(got.n_pts[k]) == n, tag
        if n == 0:
            assert got.rows(k).size == 0 and every[k].size == 0, tag
            continue
        assert float(got.sres[k]) == sres, tag
        assert got.rows(k).shape == rows.shape, tag
        assert_bit_equal(got.rows(k), rows, tag + ": download")
        assert_bit_equal(every[k], rows, tag + ": download_all")
        one = capi.Output(hb, params(base, steps[path0 + k], out_res, smooth), path0 + k, 1)   # the unchanged route
        assert int(one.n_pts[0]) == n and float(one.sres[0]) == sres, tag
        assert_bit_equal(one.rows(0), got.rows(k), tag + ": the device's one-path call")
        one.close()
    flat = np.concatenate([got.rows(k).ravel() for k in range(n_paths)]) if n_paths else np.zeros(0)
    assert_bit_equal(np.concatenate([e.ravel() for e in every]), flat, what + ": download_all = the per-path downloads back to back")
    return got


# ---- 1, 3, 7: the core batch ---------------------------------------------------------------------------------------
CORE_FACTORS = (1.0, 0.5, 1.25, 2.0, 0.8)


def core_inputs():
    case = Case("synth_gen7dof_s0")
    h = case.problem.integ_res
    ys = [case.y, case.y[:, :400], case.y, case.y[:, :150], case.y[:, :400]]
    return case, h, ys, [h * f for f in CORE_FACTORS]


@pytest.fixture(scope="module")
def core_expected(oracle_ctx):
    case, h, ys, steps = core_inputs()
    ob = swept_batch(oracle_ctx, case.problem, ys, case.sres, steps, 3 * case.max_steps())
    yield Expected(ob, output_params(case.name), steps)
    ob.close()


def core_device_batch(ctx, flags=0):
    case, h, ys, steps = core_inputs()
    prob = capi.Problem.from_buffer_copy(bytes(case.problem))
    prob.flags |= flags
    return swept_batch(ctx, prob, ys, case.sres, steps, 3 * case.max_steps())


@pytest.mark.parametrize("flags", [0, COMPACT])
def test_mixed_range_matches_the_checker_path_by_path(hip_ctx, core_expected, flags):
    """five paths, five steps: with out_res = 1.1 h paths 2 and 3 (steps 1.25 h and 2 h, coarser than out_res) are re-interpolated
    and 0, 1, 4 take the plain route; every smoothing branch; then no path and every path re-interpolated; and a sub-range"""
    case, h, ys, steps = core_inputs()
    hb = core_device_batch(hip_ctx, flags)
    assert hb.results().tobytes() == core_expected.batch.results().tobytes()
    mixed = reinterpolated(steps, 1.1 * h)
    assert mixed == [False, False, True, True, False] and any(mixed) and not all(mixed)
    for out_res, smooth in ((1.1 * h, 1.0), (1.1 * h, 5.0), (1.1 * h, 1.6), (1.1 * h, 9.0), (3.0 * h, 1.0), (3.0 * h, 5.0), (0.3 * h, 1.0), (0.3 * h, 5.0)):
        full = check_range(hb, core_expected, out_res, smooth, what=f"flags={flags}")
        sub = check_range(hb, core_expected, out_res, smooth, 1, 3, what=f"flags={flags} sub-range")
        for k in range(3):
            assert_bit_equal(sub.rows(k), full.rows(1 + k), f"sub-range (1, 3), path {1 + k}")
        full.close(); sub.close()
    assert not any(reinterpolated(steps, 3.0 * h)) and all(reinterpolated(steps, 0.3 * h))
    hb.close()


def test_chunked_mixed_range_equals_one_chunk(hip_lib, hip_ctx, core_expected):
    """a tiny scratch budget cuts the range into chunks: the result must not depend on the chunking"""
    case, h, ys, steps = core_inputs()
    ctx = capi.Context(hip_lib, 0)
    small, big = core_device_batch(ctx), core_device_batch(hip_ctx)
    # 1 MiB: a chunk per path; 4 MiB: the short paths share chunks that mix both routes, the long ones stay alone
    for budget, out_res, smooth in ((1 << 20, 1.1 * h, 1.0), (1 << 20, 1.1 * h, 5.0), (4 << 20, 1.1 * h, 1.0), (4 << 20, 1.1 * h, 5.0)):
        ctx.set_workspace_budget(output_bytes=budget)
        a = check_range(small, core_expected, out_res, smooth, what=f"chunked, budget {budget}")
        prm = params(core_expected.base, 0.0, out_res, smooth)
        b = capi.Output(big, prm, 0, len(steps), per_path_steps=True)
        assert np.array_equal(a.n_pts, b.n_pts) and a.sres.tobytes() == b.sres.tobytes()
        for k in range(len(steps)):
            assert_bit_equal(a.rows(k), b.rows(k), f"chunked = one chunk, path {k}")
        a.close(); b.close()
    small.close(); big.close()


def test_poisoned_scratch_and_chunk_cuts_together(hip_lib, core_expected):
    """every route of every chunk starts from scratch filled with 0xFF bytes, and 1 MiB cuts the range into four chunks of which
    the last mixes two routes and stages its rows (tests/test_output_plan.py checks that plan on the CPU): a launch sequence that
    read what another chunk or route left in the workspace would now read NaNs"""
    case, h, ys, steps = core_inputs()
    ctx = capi.Context(hip_lib, 0)
    ctx.set_poison(True)
    ctx.set_workspace_budget(output_bytes=1 << 20)
    hb = core_device_batch(ctx)
    check_range(hb, core_expected, 1.1 * h, 5.0, what="poisoned, budget 1 MiB").close()
    hb.close()
    ctx.close()


def test_the_old_contract_stands(hip_ctx, oracle_ctx, core_expected):
    case, h, ys, steps = core_inputs()
    base = core_expected.base
    hb = core_device_batch(hip_ctx)
    # a positive integ_res states the step of the whole range: a path that disagrees is named
    with pytest.raises(capi.BatotpError, match=r"path 1 integrates with step"):
        capi.Output(hb, params(base, h, 0.008, 5.0), 0, 5)
    # the checker serves one step per call and refuses the sentinel: what the host library's fallback relies on
    with pytest.raises(capi.BatotpError):
        capi.Output(core_expected.batch, params(base, h, 0.008, 5.0), 0, 5, per_path_steps=True)
    hb.close()
    # a uniform range: the positive value and the sentinel give the same bytes
    ub = swept_batch(hip_ctx, case.problem, ys[:4], case.sres, [h] * 4, 3 * case.max_steps())
    for out_res, smooth in ((0.008, 5.0), (h, 1.0), (2.5 * h, 4.0)):
        a = capi.Output(ub, params(base, h, out_res, smooth), 0, 4)
        b = capi.Output(ub, params(base, h, out_res, smooth), 0, 4, per_path_steps=True)
        assert np.array_equal(a.n_pts, b.n_pts) and a.sres.tobytes() == b.sres.tobytes() and int(a.n_pts.min()) > 0
        for x, y in zip(a.all_rows(), b.all_rows()):
            assert x.tobytes() == y.tobytes()
        a.close(); b.close()
    ub.close()


# ---- 2: more than a wavefront of paths -------------------------------------------------------------------------------
def test_seventy_paths_with_seventy_steps(hip_ctx, oracle_ctx):
    """the grids with a wavefront or a block per path (k_out_segmax, the series kernels) and the binary search over the
    offsets, with both routes interleaved"""
    case = Case("synth_gen7dof_s0")
    h = case.problem.integ_res
    steps = [h * (0.6 + 0.02 * k) for k in range(70)]
    assert len(set(steps)) == 70
    ys = [case.y[:, :150]] * 70
    mixed = reinterpolated(steps, 1.3 * h)
    assert any(mixed) and not all(mixed)
    hb = swept_batch(hip_ctx, case.problem, ys, case.sres, steps, case.max_steps())
    ob = swept_batch(oracle_ctx, case.problem, ys, case.sres, steps, case.max_steps())
    assert hb.results().tobytes() == ob.results().tobytes()
    exp = Expected(ob, output_params(case.name), steps)
    for smooth in (1.0, 5.0):
        check_range(hb, exp, 1.3 * h, smooth, what="70 paths").close()
    hb.close(); ob.close()


# ---- 4: paths without a trajectory, and a short curve, inside a mixed range ---------------------------------------
def test_failed_paths_and_a_short_curve_inside_a_mixed_range(hip_ctx, oracle_ctx):
    case = Case("synth_gen7dof_s0")
    h = case.problem.integ_res
    ys = [case.y[:, :400], case.y[:, :150], case.y[:, :400], case.y[:, :150], case.y[:, :150]]
    steps = [h, float("nan"), 0.01 * h, 200.0 * h, 0.7 * h]
    cap = 3 * case.max_steps()
    hb = swept_batch(hip_ctx, case.problem, ys, case.sres, steps, cap)
    ob = swept_batch(oracle_ctx, case.problem, ys, case.sres, steps, cap)
    res, ores = hb.results(), ob.results()
    for k in (0, 3, 4):      # (the step counters of a path whose sweep gave up are not part of the contract; its status is)
        assert res[k].tobytes() == ores[k].tobytes(), k
    for r in (res, ores):
        assert int(r[1]["status_rev"] | r[1]["status_fwd"]) & capi.ST_MAX_INTEG_TIME
        assert int(r[2]["status_rev"] | r[2]["status_fwd"]) & capi.ST_CAPACITY
    assert int(res[3]["status_fwd"]) & capi.ST_SHORT and int(res[3]["n_fwd"]) == 4
    assert float(res[3]["t_total"]) / 3. != steps[3]       # the curve's time step is t_total / 3, not the path's step
    exp = Expected(ob, output_params(case.name), steps)
    for out_res, smooth in ((0.8 * h, 1.0), (0.8 * h, 5.0), (h, 1.6)):
        mixed = [r for r, k in zip(reinterpolated(steps, out_res), range(5)) if k in (0, 3, 4)]
        assert any(mixed) and not all(mixed)
        got = check_range(hb, exp, out_res, smooth, what="failed paths")
        assert int(got.n_pts[1]) == 0 and int(got.n_pts[2]) == 0 and min(int(got.n_pts[k]) for k in (0, 3, 4)) >= 4
        got.close()
    hb.close(); ob.close()


# ---- 5: every robot branch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synth_cspr_s3", "CSPR3DOF_par", "RR", "KUKA_trq", "KUKA-LWR-IV", "UR5"])
def test_every_robot_branch_with_per_path_steps(hip_ctx, oracle_ctx, name):
    """cable tensions (per-path time factors), closed-form torques with host trig, the chain model, kinematics only, pose rows"""
    case = Case(name)
    h = case.problem.integ_res
    short = np.ascontiguousarray(case.y[:, :max(40, case.n // 3)])
    ys = [case.y, short, case.y]
    steps = [h, 0.7 * h, 1.6 * h]
    base = output_params(name) if name in helpers.OUTPUT_CASES else capi.OutputParams(case.problem.n_joints, capi.PATH_JOINT, h, 0.008, 5.0)
    cap = 2 * case.max_steps()
    hb = swept_batch(hip_ctx, case.problem, ys, case.sres, steps, cap, trig=True)
    ob = swept_batch(oracle_ctx, case.problem, ys, case.sres, steps, cap, trig=True)
    assert hb.results().tobytes() == ob.results().tobytes()
    exp = Expected(ob, base, steps)
    mixed = reinterpolated(steps, 1.2 * h)
    assert any(mixed) and not all(mixed)
    for out_res in (base.out_res, 1.2 * h):
        for smooth in (1.0, 5.0):
            got = check_range(hb, exp, out_res, smooth, what=name)
            assert int(got.n_pts.min()) >= 4, name
            got.close()
    hb.close(); ob.close()


# ---- 6: long series -------------------------------------------------------------------------------------------------
def test_long_series_on_both_sides_of_the_wavefront_solve_in_one_mixed_call(hip_ctx, oracle_ctx):
    """a forward curve above and one below the 16 386 points from which a series is solved by the lanes of a wavefront
    (spline_lanes.hip.h), one of the two re-interpolated, in one call"""
    case = Case("synth_ur_s7_100k")
    h = case.problem.integ_res
    ys = [case.y[:, :66000], case.y[:, :68000]]
    steps = [h, 0.9 * h]
    out_res = 0.95 * h
    assert reinterpolated(steps, out_res) == [True, False]
    cap = int(case.max_steps() / 0.9) + 64
    hb = swept_batch(hip_ctx, case.problem, ys, case.sres, steps, cap)
    ob = swept_batch(oracle_ctx, case.problem, ys, case.sres, steps, cap)
    assert hb.results().tobytes() == ob.results().tobytes()
    fwd = [int(r["n_fwd"]) for r in hb.results()]
    assert fwd[1] > 16386 > fwd[0] > 15000, fwd
    exp = Expected(ob, capi.OutputParams(case.problem.n_joints, capi.PATH_JOINT, h, out_res, 1.0), steps)
    for smooth in (1.0, 5.0):
        check_range(hb, exp, out_res, smooth, what="long series").close()
    hb.close(); ob.close()
