"""GPU (-m gpu): the lockstep form of the forward sweep (k_sweep8_lock, batotp_amd/csrc/sweep8_fwd.hip.h).

Every case runs its batch three ways -- through the lockstep kernel, through the previous form (k_sweep8's flat loop in the
forward sweep too, batotp_hip_set_flat_form 2) and through the oracle -- and every field of every result row and both curves
of every path must be bit-equal across all three.  The shapes are the smallest at which the kernel's control structure can go
wrong: partly filled wavefronts and idle lane groups, paths of one wavefront that end at different steps (by their length, by the
time limit in the reverse sweep, by a curve of fewer than four points), stages that bisect (with the certified fast-forward and
without it), bisections that fail and leave the stage value of the step before in place, knot values of 1e308 (spline coefficients
and theta' that are inf or NaN; the stage values themselves stay finite, see that test), and the capacity rule of curves kept in place."""
import numpy as np
import pytest

from helpers import Case, assert_bit_equal, random_knots
from batotp_amd import capi

pytestmark = pytest.mark.gpu

COMPACT = capi.F_NO_SAMPLES | capi.F_COMPACT_SPLINES


def _run(ctx, prob, ys, sres, cap, integ=None, pointwise=False, hip=False):
    """knots -> precompute -> (pointwise values) -> both sweeps of one batch.  The reverse curve is fetched between the sweeps
    (curves in place: the forward sweep consumes it).  Returns (result rows, reverse curves, forward curves, forward launch);
    hip="both": the last entry is (reverse launch, forward launch)."""
    b = capi.Batch(ctx, prob, [y.shape[1] for y in ys], cap)
    b.upload_knots(0, ys, sres)
    if integ is not None:
        b.set_path_integ_res(0, integ)
    b.precompute(0)
    if pointwise:
        b.pointwise_mvc()
    b.sweep(-1)
    rev = [b.curve(k, -1) for k in range(len(ys))]
    b.sweep(+1)
    res = b.results()
    fwd = [b.curve(k, +1) for k in range(len(ys))]
    launch = b.last_sweep_launch(+1) if hip else None
    if hip == "both":
        launch = (b.last_sweep_launch(-1), launch)
    b.close()
    return res, rev, fwd, launch


def _hip_ctx(hip_lib, form, ppw, ff=True):
    ctx = capi.Context(hip_lib, 0)
    ctx.set_sweep_group(8)
    ctx.set_paths_per_wave(ppw)
    ctx.set_sweep_hold(4, 8)
    ctx.set_flat_form(form)
    ctx.set_fast_forward(ff)
    return ctx


def _same(a, b, what):
    ra, reva, fwda = a[:3]
    rb, revb, fwdb = b[:3]
    for f in ra.dtype.names:
        assert np.array_equal(ra[f], rb[f]), (what, f, ra[f], rb[f])
    for k in range(len(reva)):
        for name, ca, cb in (("reverse", reva[k], revb[k]), ("forward", fwda[k], fwdb[k])):
            assert_bit_equal(ca[0], cb[0], f"{what}: path {k} {name} s")
            assert_bit_equal(ca[1], cb[1], f"{what}: path {k} {name} sdot")


def _three_ways(hip_lib, oracle_out, prob, ys, sres, cap, ppw, ff=True, what="", **kw):
    """lockstep kernel, previous form, oracle: all equal; returns the lockstep run"""
    outs = {}
    for form in (1, 2):
        ctx = _hip_ctx(hip_lib, form, ppw, ff)
        outs[form] = _run(ctx, prob, ys, sres, cap, hip=True, **kw)
        ctx.close()
        assert outs[form][3] == (8, ppw, 8), (what, form, outs[form][3])
    _same(outs[1], outs[2], f"{what}: lockstep kernel against the previous form")
    _same(outs[1], oracle_out, f"{what}: lockstep kernel against the oracle")
    return outs[1]


def _with_flags(prob, extra):
    p = capi.Problem.from_buffer_copy(bytes(prob))
    p.flags |= extra
    return p


# ---- partly filled wavefronts and idle lane groups ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden21(oracle_ctx):
    """the seven GEN7DOF golden paths of test_flat_sweep_loop_with_paths_drifting_apart, three times: 21 paths, and their oracle run"""
    names = ["synth_gen7dof_s0", "GEN7DOF", "synth_gen7dof_s1_vel", "GEN7DOF", "synth_gen7dof_s0", "GEN7DOF", "GEN7DOF"]
    cases = [Case(n) for n in names] * 3
    prob = cases[0].problem
    ys, sres = [c.y for c in cases], [c.sres for c in cases]
    cap = 4 * max(c.max_steps() for c in cases)
    return prob, ys, sres, cap, _run(oracle_ctx, prob, ys, sres, cap)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("ppw", [8, 5, 3, 1])
def test_partial_wavefronts_and_idle_groups(hip_lib, golden21, ppw, compact):
    """21 paths at 8, 5, 3 and 1 paths per wavefront (the last wavefront partly filled, lane groups that leave at once), compact
    pairs (FEAT -1) and coefficient rows (FEAT 0)"""
    prob, ys, sres, cap, oracle_out = golden21
    _three_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT if compact else 0), ys, sres, cap, ppw, what=f"ppw {ppw} compact {compact}")


# ---- paths of one wavefront that end at different steps ----------------------------------------------------------------------

def _ragged_population():
    """ten random velocity / acceleration paths of 16 to 300 knots with differing integration steps.  Path 3 hardly moves its joints
    (every theta' below the threshold: no limit applies), so it is through after two steps and its forward curve has fewer than four
    points; path 6 is far longer in time than the others, so a time limit between its duration and theirs ends it, and only it, in
    the reverse sweep."""
    rng = np.random.default_rng(4242)
    nJ = 6
    prob = capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=list(rng.uniform(0.5, 8.0, nJ)), jnt_acc_max=list(rng.uniform(1.0, 40.0, nJ)),
                             integ_res=0.01, max_integ_time=1e5)
    lengths = [16, 300, 57, 16, 128, 211, 300, 33, 90, 171]
    ys = [random_knots(rng, nJ, n, rng.uniform(0.2, 3.0)) for n in lengths]
    ys[3] = np.ascontiguousarray(ys[3] * 1e-5)    # next to no move ...
    ys[6] = np.ascontiguousarray(ys[6] * 15.0)    # ... and a long one
    sres = [float(rng.uniform(0.01, 0.2)) for _ in lengths]
    integ = [0.01, 0.004, 0.02, 0.01, 0.01, 0.004, 0.002, 0.02, 0.01, 0.005]
    return prob, ys, sres, integ, 60000


@pytest.mark.parametrize("compact", [True, False])
def test_paths_of_a_wavefront_that_end_at_different_steps(hip_lib, oracle_ctx, compact):
    prob, ys, sres, integ, cap = _ragged_population()
    # the time limit: between the duration of the slowest path and everything else (from an oracle run without a limit)
    free = _run(oracle_ctx, prob, ys, sres, cap, integ=integ)[0]
    slow = int(np.argmax(free["t_rev"]))
    others = np.delete(np.arange(len(ys)), slow)
    rest = max(float(free["t_rev"][others].max()), float(free["t_total"][others].max()))
    assert float(free["t_rev"][slow]) > 1.5 * rest, "the population is meant to have one path far longer in time than the others"
    prob.max_integ_time = 1.25 * rest
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap, integ=integ)
    ro = oracle_out[0]
    late = (ro["status_rev"] & capi.ST_MAX_INTEG_TIME) != 0
    assert late.sum() == 1 and late[slow] and int(ro["n_rev"][slow]) < 2, "exactly one path ends by the time limit, in the reverse sweep"
    assert not np.any(ro["status_fwd"][others] & capi.ST_MAX_INTEG_TIME)
    short = (ro["status_fwd"] & capi.ST_SHORT) != 0
    assert short.sum() >= 1 and not short[slow], "one forward curve of fewer than four points (re-interpolated to four)"
    assert len(set(int(v) for v in ro["steps_fwd"][others])) >= 6, "the paths end at different steps"
    got = _three_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT if compact else 0), ys, sres, cap, 8, integ=integ, what=f"ragged compact {compact}")
    assert int(got[0]["n_fwd"][slow]) == 0


# ---- stages that bisect, bisections that fail ---------------------------------------------------------------------------------

def _hard_problem(seed):
    """velocity / acceleration-only problems near the edges of the fast-forward certificate (the population of
    tests/test_gpu_fuzz.py: limits over six decades, nearly parallel joints, a joint standing still)"""
    rng = np.random.default_rng(7000 + seed)
    nJ = int(rng.integers(2, 9))
    n_paths = int(rng.integers(4, 12))
    decades = rng.uniform(-3, 3, nJ)
    vmax = list(10.0 ** rng.uniform(-1, 1.5, nJ))
    amax = list(10.0 ** decades)
    prob = capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=vmax, jnt_acc_max=amax,
                             integ_res=float(rng.choice([0.002, 0.005, 0.02])), max_integ_time=1e5)
    ys = []
    for _ in range(n_paths):
        n = int(rng.integers(16, 300))
        y = random_knots(rng, nJ, n, rng.uniform(0.2, 3.0))
        kind = rng.integers(0, 4)
        if kind == 0:      # a joint that barely moves: theta' around the threshold
            y[rng.integers(0, nJ)] *= 10.0 ** rng.uniform(-9, -4)
        elif kind == 1:    # two joints with the same shape (nearly parallel constraint lines)
            a, b = rng.integers(0, nJ, 2)
            y[b] = y[a] * (1.0 + 10.0 ** rng.uniform(-12, -3))
        elif kind == 2:    # a joint that stands still exactly on part of the path
            j = rng.integers(0, nJ)
            y[j, n // 3: 2 * n // 3] = y[j, n // 3]
        ys.append(np.ascontiguousarray(y))
    sres = [float(rng.uniform(0.01, 0.2)) for _ in range(n_paths)]
    return prob, ys, sres, 80000


def _failing_batch():
    """jnt_acc_max[0] = -1: wherever joint 0 moves no sddot is admissible and every bisection fails.  Joint 0 hovers around the
    zero-velocity threshold on some paths (they fail now and then and finish), moves on others (they fail at every stage and run into
    the step capacity in the reverse sweep already) and stands still on one (the recipe of
    test_flat_sweep_loop_on_stalled_velocity_acceleration_paths)"""
    rng = np.random.default_rng(500)
    nJ = 3
    amax = [-1.0, float(rng.uniform(5, 30)), float(rng.uniform(5, 30))]
    prob = capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=list(rng.uniform(1, 6, nJ)), jnt_acc_max=amax, integ_res=0.01, max_integ_time=1e5)
    ys = [random_knots(rng, nJ, int(rng.integers(40, 300)), rng.uniform(0.5, 2.0)) for _ in range(8)]
    ys[3][0, :] = 0.25
    for k, f in ((0, 3e-6), (1, 1e-5), (2, 3e-5), (4, 1e-4), (5, 2e-6), (6, 1e-6)):
        ys[k][0] *= f
    sres = [float(rng.uniform(0.02, 0.1)) for _ in ys]
    return prob, ys, sres, 3000


@pytest.mark.parametrize("seed", [0, 1, 2, 3, "fail"])
def test_forward_bisections_with_and_without_the_fast_forward(hip_lib, oracle_ctx, seed):
    """four seeds of the hard-problem population, and one batch ("fail") in which every bisection of a moving joint 0 fails: the
    stage value of the step before (w_st, w6) must survive in its register, and the failure count of the forward sweep must be the
    oracle's"""
    prob, ys, sres, cap = _failing_batch() if seed == "fail" else _hard_problem(seed)
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap)
    if seed == "fail":
        ro = oracle_out[0]
        done = ro["n_fwd"] > 0
        assert int((ro["n_bisect_fail_fwd"][done] > 100).sum()) >= 2, "forward sweeps that finish with hundreds of failed bisections"
    for ff in (True, False):
        got = _three_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT), ys, sres, cap, 8, ff=ff, what=f"seed {seed} fast-forward {ff}")
        assert np.array_equal(got[0]["n_bisect_fail_fwd"], oracle_out[0]["n_bisect_fail_fwd"])


# ---- knot values of 1e308 ---------------------------------------------------------------------------------------------------------

def test_knot_values_of_1e308(hip_lib, oracle_ctx):
    """knot values of 1e308 beside ordinary paths (one joint at one knot; two joints with opposite signs; every joint at one knot): the
    second derivatives of the spline overflow, so the coefficients of the segments around those knots and theta', theta'' of the
    stages evaluated there are inf or NaN.  Status bits, rows and curves as the previous form and the oracle.

    What this does NOT reach is a non-finite STAGE value (v_k, w_k), the situation k_sweep8's literal tableau combination exists for:
    every comparison of the check ignores a NaN bound, so v and w stay finite here (asserted below on the oracle's curves).  Through
    the library's interface a forward sweep cannot meet one at all: w is infinite only where the acceleration cap 2 s_end / h^2
    overflows, that holds for the reverse sweep of the same path too, whose second stage then forms inf - inf, and a path whose
    reverse sweep ended without a curve is not swept forward."""
    rng = np.random.default_rng(99)
    nJ = 7
    prob = capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=list(rng.uniform(0.5, 8.0, nJ)), jnt_acc_max=list(rng.uniform(1.0, 40.0, nJ)),
                             integ_res=0.01, max_integ_time=1e5)
    ys = [random_knots(rng, nJ, n, 1.0) for n in (40, 64, 150, 64, 90)]
    ys[1][2, 30] = 1e308
    ys[3][0, 5] = 1e308
    ys[3][4, 40] = -1e308
    ys[4][:, 45] = 1e308
    sres = [0.05] * len(ys)
    cap = 4000
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap)
    assert all(np.isfinite(c[0]).all() and np.isfinite(c[1]).all() and len(c[0]) >= 4 for c in oracle_out[2]), "every forward curve is finite"
    for extra in (COMPACT, 0):
        _three_ways(hip_lib, oracle_out, _with_flags(prob, extra), ys, sres, cap, 8, what=f"knots of 1e308, flags {extra}")


# ---- curves in place ---------------------------------------------------------------------------------------------------------------

def test_curves_in_place_ample_and_tight(hip_lib, oracle_ctx):
    """BATOTP_F_CURVES_IN_PLACE | BATOTP_F_MVC_IN_CURVES: once with ample capacity, once with a capacity at which the previous form
    ends at least one path (not all) with BATOTP_ST_CAPACITY -- found with the previous form -- where the lockstep kernel must end the
    same paths and leave the same rows"""
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
    # capacities from the longest forward curve downwards, with the previous form: the first at which some path, not all, ends by capacity
    ctx = _hip_ctx(hip_lib, 2, 8)
    tight = None
    for cap in sorted({max(floor, int(n) + 40) for n in got[0]["n_fwd"]}, reverse=True):
        r = _run(ctx, prob, ys, sres, cap, pointwise=True)[0]
        full = ((r["status_fwd"] | r["status_rev"]) & capi.ST_CAPACITY) != 0
        if 0 < full.sum() < len(ys) and np.any((r["status_fwd"] & capi.ST_CAPACITY) != 0):
            tight = cap
            break
    ctx.close()
    assert tight is not None, "no capacity at which the previous form ends some paths by capacity"
    oracle_out = _run(oracle_ctx, prob, ys, sres, tight, pointwise=True)
    _three_ways(hip_lib, oracle_out, prob, ys, sres, tight, 8, pointwise=True, what=f"in place, capacity {tight}")
