"""GPU (-m gpu): the register window of the reverse curve in the forward batch kernels (batotp_amd/csrc/mvc_window.h, driven by
sweep8_mvcwalk.inc inside k_sweep8_lock and k_sweep8<G, FEAT, 1>).

Every case runs its batch three ways -- through the lockstep kernel k_sweep8_lock, through the general kernel k_sweep, which walks
the reverse curve with its own code and does not include the fragment (flat form 0 with the nested loops; the launch is asserted), and
through the oracle -- and every field of every result row and both curves of every path must be bit-equal across all three.  The
shapes are those at which a window around the cursor can go wrong: reverse curves so short that the window is clamped at one end or
the other all the time, curves kept in place (the window reads behind the cursor, where the forward curve is being written) at an
ample and at the tightest useful capacity, partly filled wavefronts with both knot layouts, paths of one wavefront whose cursors move
at very different rates, and paths that crawl along the reverse curve.

A sweep of the library never leaves a reverse curve of fewer than four points (one that ends after fewer than three steps is
re-interpolated to four, BATOTP_ST_SHORT), but batotp_hip_upload_curve takes any curve of two points or more, and the forward kernels
follow it: the curves of 2, 3 and 4 points of the first test are uploaded.  On two points the cursor never leaves segment 0 and both
neighbours of the window are clamped throughout; on three the lower one is clamped on the first segment and the upper one on the last."""
import numpy as np
import pytest

from helpers import Case, random_knots
from batotp_amd import capi
from test_gpu_sweep8_lockstep import COMPACT, _failing_batch, _hip_ctx, _run, _same, _with_flags

pytestmark = pytest.mark.gpu


def _general_ctx(hip_lib, ppw, ff=True):
    """the general kernel k_sweep with its nested loops in both directions"""
    ctx = capi.Context(hip_lib, 0)
    ctx.set_sweep_group(8)
    ctx.set_paths_per_wave(ppw)
    ctx.set_sweep_hold(-1, -1)
    ctx.set_flat_form(0)
    ctx.set_fast_forward(ff)
    return ctx


def _three_ways(hip_lib, oracle_out, prob, ys, sres, cap, ppw, ff=True, what="", **kw):
    """lockstep kernel, general kernel, oracle: all equal; returns the lockstep run"""
    ctx = _hip_ctx(hip_lib, 1, ppw, ff)
    lock = _run(ctx, prob, ys, sres, cap, hip=True, **kw)
    ctx.close()
    assert lock[3] == (8, ppw, 8), (what, "lockstep launch", lock[3])
    ctx = _general_ctx(hip_lib, ppw, ff)
    gen = _run(ctx, prob, ys, sres, cap, hip=True, **kw)
    ctx.close()
    assert gen[3] == (8, ppw, -1), (what, "general kernel launch", gen[3])
    _same(lock, gen, f"{what}: lockstep kernel against the general kernel")
    _same(lock, oracle_out, f"{what}: lockstep kernel against the oracle")
    return lock


def _va_problem(rng, nJ=7, integ_res=0.01):
    return capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=list(rng.uniform(0.5, 8.0, nJ)), jnt_acc_max=list(rng.uniform(1.0, 40.0, nJ)),
                             integ_res=integ_res, max_integ_time=1e5)


# ---- uploaded reverse curves of 2, 3 and 4 points -------------------------------------------------------------------------------

def _run_uploaded(ctx, prob, ys, sres, cap, uploads, hip=False):
    """as _run, but between the sweeps the reverse curves of the paths in `uploads` ({path: (s, sdot)}) are replaced through
    batotp_hip_upload_curve"""
    b = capi.Batch(ctx, prob, [y.shape[1] for y in ys], cap)
    b.upload_knots(0, ys, sres)
    b.precompute(0)
    b.sweep(-1)
    for k, (s, sd) in uploads.items():
        b.upload_curve(k, s, sd)
    rev = [b.curve(k, -1) for k in range(len(ys))]
    b.sweep(+1)
    res = b.results()
    fwd = [b.curve(k, +1) for k in range(len(ys))]
    launch = b.last_sweep_launch(+1) if hip else None
    b.close()
    return res, rev, fwd, launch


@pytest.mark.parametrize("compact", [True, False])
def test_uploaded_reverse_curves_of_two_three_and_four_points(hip_lib, oracle_ctx, compact):
    """eight paths in one wavefront; five of them get a reverse curve of 2, 3, 4, 2 and 3 points from 0 to the path end through
    batotp_hip_upload_curve, at speeds below the ordinary reverse curve's (so the forward sweep rides on them: every stage interpolates
    on the uploaded segments) -- and one of the 3-point curves stops at 60 % of the path, so that the cursor asks to move up on its
    last segment for the rest of the sweep and the clamp refuses.  Three ordinary paths between them.  The in-kernel first loads of the
    window, its refills, the end snap's read of the last point and the result rows: lockstep kernel = general kernel = oracle"""
    rng = np.random.default_rng(909)
    prob = _va_problem(rng)
    lengths = (40, 64, 33, 90, 57, 48, 72, 40)
    ys = [random_knots(rng, 7, n, rng.uniform(0.5, 2.0)) for n in lengths]
    sres = [0.05] * len(ys)
    cap = 8000
    ordinary = _run(oracle_ctx, prob, ys, sres, cap)
    assert not np.any(ordinary[0]["status_fwd"]) and int(ordinary[0]["n_rev"].min()) > 100
    shapes = {0: [0.0, 1.0], 2: [0.0, 0.4, 1.0], 4: [0.0, 0.2, 0.7, 1.0], 5: [0.0, 1.0], 7: [0.0, 0.3, 0.6]}
    uploads = {}
    for k, frac in shapes.items():
        s_end = sres[k] * (lengths[k] - 1)
        low = 0.3 * float(np.median(ordinary[1][k][1]))   # well below the path's own reverse curve over most of its length
        s = np.array(frac) * s_end
        sd = low * (1.0 + 0.5 * np.sin(1.0 + 2.0 * np.arange(len(frac)) + k))
        uploads[k] = (s, sd)
    p = _with_flags(prob, COMPACT if compact else 0)
    oracle_out = _run_uploaded(oracle_ctx, prob, ys, sres, cap, uploads)
    ro = oracle_out[0]
    assert [int(ro["n_rev"][k]) for k in sorted(shapes)] == [2, 3, 4, 2, 3]
    assert all(int(ro["n_fwd"][k]) >= 4 for k in range(len(ys))), ro["n_fwd"]
    for k in shapes:
        assert float(ro["t_total"][k]) > 1.5 * float(ordinary[0]["t_total"][k]), "the forward sweep is meant to ride on the uploaded curve"
    ctx = _hip_ctx(hip_lib, 1, 8)
    lock = _run_uploaded(ctx, p, ys, sres, cap, uploads, hip=True)
    ctx.close()
    assert lock[3] == (8, 8, 8), lock[3]
    ctx = _general_ctx(hip_lib, 8)
    gen = _run_uploaded(ctx, p, ys, sres, cap, uploads, hip=True)
    ctx.close()
    assert gen[3] == (8, 8, -1), gen[3]
    _same(lock, gen, f"uploaded curves, compact {compact}: lockstep kernel against the general kernel")
    _same(lock, oracle_out, f"uploaded curves, compact {compact}: lockstep kernel against the oracle")


# ---- reverse curves of the fewest points ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("compact", [True, False])
def test_shortest_reverse_curves_beside_ordinary_ones(hip_lib, oracle_ctx, compact):
    """the shortest reverse curves a sweep of the library itself leaves.  Eight paths in one wavefront: five with knots scaled by 1e-5 (next to no move: no limit applies, the sweeps are through after a
    few steps) at integration steps that give reverse curves of four points made of three (BATOTP_ST_SHORT), of four points proper and
    of five or six, between three ordinary paths.  On four points the window's lower neighbour is clamped on segment 0 and the upper
    one on segment 2, the last: a clamp is in force at every position but one from the first step on."""
    rng = np.random.default_rng(77)
    prob = _va_problem(rng)
    ys = [random_knots(rng, 7, n, rng.uniform(0.5, 2.0)) for n in (16, 40, 16, 90, 16, 16, 64, 16)]
    tiny = (0, 2, 4, 5, 7)
    for k in tiny:
        ys[k] = np.ascontiguousarray(ys[k] * 1e-5)
    sres = [0.05] * len(ys)
    integ = [0.05, 0.01, 0.03, 0.01, 0.01, 0.01, 0.01, 0.015]
    cap = 8000
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap, integ=integ)
    ro = oracle_out[0]
    n_rev = [int(ro["n_rev"][k]) for k in tiny]
    short = [bool(ro["status_rev"][k] & capi.ST_SHORT) for k in tiny]
    assert any(n == 4 and s for n, s in zip(n_rev, short)), "a reverse curve of three points, re-interpolated to four"
    assert any(n == 4 and not s for n, s in zip(n_rev, short)), "a reverse curve of four points"
    assert any(n in (5, 6) for n in n_rev) and max(n_rev) <= 6 and min(n_rev) == 4
    assert all(int(ro["n_fwd"][k]) >= 4 for k in range(len(ys)))
    _three_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT if compact else 0), ys, sres, cap, 8, integ=integ, what=f"shortest reverse curves, compact {compact}")


# ---- curves in place -------------------------------------------------------------------------------------------------------------

def test_window_stays_inside_the_margin_of_curves_in_place(hip_lib, oracle_ctx):
    """BATOTP_F_CURVES_IN_PLACE | BATOTP_F_MVC_IN_CURVES, 11 paths of 64 to 128 knots, 7 joints: the window reads one point behind
    the cursor's segment and two ahead, inside the margin of 64 points the kernels keep between the forward curve and the reverse
    points still to be read.  Once with ample capacity; once with the tightest capacity at which the kernel of before the window
    (k_sweep8's flat loop ran the same capacity rule; found here with the general kernel, which has no window) ends some paths, not
    all, with BATOTP_ST_CAPACITY: the same paths must end, with the same rows"""
    rng = np.random.default_rng(31)
    nJ = 7
    prob = capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON | COMPACT | capi.F_CURVES_IN_PLACE | capi.F_MVC_IN_CURVES,
                             jnt_vel_max=list(rng.uniform(0.5, 8.0, nJ)), jnt_acc_max=list(rng.uniform(1.0, 40.0, nJ)), integ_res=0.01, max_integ_time=1e5)
    ys = [random_knots(rng, nJ, n, rng.uniform(0.5, 2.0)) for n in (120, 100, 80, 120, 64, 110, 96, 128, 72, 100, 88)]
    sres = [0.05] * len(ys)
    floor = (3 * max(y.shape[1] for y in ys) + 1) // 2   # the pointwise values of a path must fit its curve slot
    ample = 8000
    oracle_out = _run(oracle_ctx, prob, ys, sres, ample, pointwise=True)
    got = _three_ways(hip_lib, oracle_out, prob, ys, sres, ample, 8, pointwise=True, what="in place, ample")
    assert not np.any(got[0]["status_fwd"] & capi.ST_CAPACITY) and int(got[0]["n_fwd"].min()) > floor
    # capacities from the longest forward curve downwards, with the general kernel: the first at which some path, not all, ends by capacity
    ctx = _general_ctx(hip_lib, 8)
    tight = None
    for cap in sorted({max(floor, int(n) + 40) for n in got[0]["n_fwd"]}, reverse=True):
        r = _run(ctx, prob, ys, sres, cap, pointwise=True)[0]
        full = ((r["status_fwd"] | r["status_rev"]) & capi.ST_CAPACITY) != 0
        if 0 < full.sum() < len(ys) and np.any((r["status_fwd"] & capi.ST_CAPACITY) != 0):
            tight = cap
            break
    ctx.close()
    assert tight is not None, "no capacity at which the general kernel ends some paths by capacity"
    oracle_out = _run(oracle_ctx, prob, ys, sres, tight, pointwise=True)
    got = _three_ways(hip_lib, oracle_out, prob, ys, sres, tight, 8, pointwise=True, what=f"in place, capacity {tight}")
    full = (got[0]["status_fwd"] & capi.ST_CAPACITY) != 0
    assert 0 < full.sum() < len(ys)


# ---- partly filled wavefronts, both knot layouts -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden21(oracle_ctx):
    """the seven GEN7DOF golden paths of tests/test_gpu_sweep8_lockstep.py, three times: 21 paths, and their oracle run"""
    names = ["synth_gen7dof_s0", "GEN7DOF", "synth_gen7dof_s1_vel", "GEN7DOF", "synth_gen7dof_s0", "GEN7DOF", "GEN7DOF"]
    cases = [Case(n) for n in names] * 3
    prob = cases[0].problem
    ys, sres = [c.y for c in cases], [c.sres for c in cases]
    cap = 4 * max(c.max_steps() for c in cases)
    return prob, ys, sres, cap, _run(oracle_ctx, prob, ys, sres, cap)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("ppw", [8, 5, 1])
def test_golden_paths_per_wavefront_and_knot_layout(hip_lib, golden21, ppw, compact):
    """21 golden GEN7DOF paths at 8, 5 and 1 paths per wavefront, compact pairs (FEAT -1) and coefficient rows (FEAT 0)"""
    prob, ys, sres, cap, oracle_out = golden21
    _three_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT if compact else 0), ys, sres, cap, ppw, what=f"ppw {ppw} compact {compact}")


# ---- cursors of one wavefront that move at very different rates ------------------------------------------------------------------

def _points_crossed(rev, fwd):
    """the largest number of reverse-curve points inside one step of the forward curve"""
    idx = np.searchsorted(np.sort(rev[0]), fwd[0], side="right")
    return int(np.max(np.diff(idx)))


def test_integration_steps_from_0p002_to_0p02_in_one_wavefront(hip_lib, oracle_ctx):
    """11 paths with per-path integration steps from 0.002 to 0.02 (geometric): while one path of the wavefront takes a step another
    takes ten, so walks in which one cursor moves and seven reload what they hold are the rule.  From the oracle's curves: some
    forward steps contain two and three points of the reverse curve (the cursor moves two and three segments in one walk, the second
    move onto a point loaded by the first), and steps that contain none exist on every path."""
    rng = np.random.default_rng(2024)
    prob = _va_problem(rng)
    lengths = [64, 100, 80, 128, 72, 90, 110, 64, 120, 96, 70]
    ys = [random_knots(rng, 7, n, rng.uniform(0.5, 2.0)) for n in lengths]
    sres = [float(rng.uniform(0.02, 0.1)) for _ in lengths]
    integ = list(np.geomspace(0.002, 0.02, len(lengths)))
    cap = 40000
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap, integ=integ)
    crossed = [_points_crossed(oracle_out[1][k], oracle_out[2][k]) for k in range(len(ys))]
    assert max(crossed) >= 3 and sum(c >= 2 for c in crossed) >= 3, crossed
    assert not np.any(oracle_out[0]["status_fwd"]) and int(oracle_out[0]["n_fwd"].min()) > 500
    _three_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT), ys, sres, cap, 8, integ=integ, what="integration steps 0.002 .. 0.02")


# ---- paths that crawl along the reverse curve ------------------------------------------------------------------------------------

@pytest.mark.parametrize("ff", [True, False])
def test_failing_bisections_crawl_along_the_reverse_curve(hip_lib, oracle_ctx, ff):
    """the failing-bisection batch of tests/test_gpu_sweep8_lockstep.py: paths on which every bisection fails advance by next to
    nothing per step, thousands of walks without a move between two moves"""
    prob, ys, sres, cap = _failing_batch()
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap)
    got = _three_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT), ys, sres, cap, 8, ff=ff, what=f"failing bisections, fast-forward {ff}")
    assert np.array_equal(got[0]["n_bisect_fail_fwd"], oracle_out[0]["n_bisect_fail_fwd"])
