"""GPU (-m gpu): the knot window of the compact layout in the batch sweep kernels (batotp_amd/csrc/knot_window.h: the segment change of
k_sweep8_lock and of k_sweep8<G, -1, DIR>, both directions, G = 8 and 4).

Every case runs its batch
  * through the lockstep forward kernel with the flat reverse kernel, and through the general kernel k_sweep, which has no window
    (_three_ways of tests/test_gpu_fwd_curve_window.py),
  * through k_sweep8's flat loop in both directions (flat form 2), with the reverse sweep's certificate phase at hold 3 and off,
and every field of every result row and both curves of every path must be bit-equal to the oracle's.  The forward launch triple is
asserted, so a case cannot silently run another kernel.

The shapes are the smallest at which a window of two knots around the knot cursor can go wrong, and each test asserts from the ORACLE's
result rows (step counts against knot counts) that its shape does what it is for:
  * paths of 4 knots -- the smallest count the library accepts -- and of 5, 6 and 7: the prefetch index is clamped at the far end from
    the first or second change on, in the reverse direction at knot 0; with 1, 7 and 8 joints (lane 7 off, every lane on);
  * one wavefront of eight paths of the same length and about the same number of steps, with 6 to 3600 knots: on the densest path a
    stage crosses two or more segments on average (a missed prefetch, the literal route, every time), on the sparsest ones a path
    stays ten steps and more on a segment and reloads the knot it holds whenever another path of the wavefront changes;
  * the same population at 3 and 5 paths per wavefront with 11 paths (partly filled wavefronts, a last one with fewer paths);
  * paths that end early by capacity and by the time limit while their neighbours in the wavefront go on changing segments;
  * two joints per lane (G = 4) at 7 joints;
  * the lean layout of the headline (curves in place, pointwise values in the curves) at an ample and at the tightest useful capacity.

NOT known to be reached by any input here: a knot cursor that moves AGAINST the sweep inside the kernels.  The result rows do not tell
whether a stage ever fell back behind the segment of the stage before it (the stage positions of a step grow with speeds that are never
negative, and the next step starts where the last one ended, so it would take a tableau combination with a negative net weight), and no
case is built to force it.  The "against" moves that tests/test_knot_window.py replays on the CPU -- a miss, the literal route -- are
covered there alone."""
import numpy as np
import pytest

from helpers import random_knots
from batotp_amd import capi
from test_gpu_sweep8_lockstep import COMPACT, _hip_ctx, _run, _same, _with_flags
from test_gpu_fwd_curve_window import _general_ctx, _three_ways

pytestmark = pytest.mark.gpu

LEAN = capi.F_CURVES_IN_PLACE | capi.F_MVC_IN_CURVES


def _problem(rng, nJ=7, integ_res=0.01, flags=0, max_integ_time=1e5):
    return capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON | flags, jnt_vel_max=list(rng.uniform(0.5, 8.0, nJ)),
                             jnt_acc_max=list(rng.uniform(1.0, 40.0, nJ)), integ_res=integ_res, max_integ_time=max_integ_time)


def _flat_both_directions(hip_lib, oracle_out, prob, ys, sres, cap, ppw, what, group=8, **kw):
    """k_sweep8's flat loop in both directions (G = 4: k_sweep8<4, ., .>, which has no lockstep form), certificate hold 3 and off"""
    for cert in (3, 0):
        ctx = _hip_ctx(hip_lib, 2 if group == 8 else 1, ppw)
        ctx.set_sweep_group(group)
        ctx.set_cert_hold(cert)
        out = _run(ctx, prob, ys, sres, cap, hip=True, **kw)
        ctx.close()
        assert out[3] == (group, ppw, 8), (what, cert, "flat form launch", out[3])
        _same(out, oracle_out, f"{what}: flat form, {group} lanes per path, certificate hold {cert}, against the oracle")


def _all_ways(hip_lib, oracle_out, prob, ys, sres, cap, ppw, what, **kw):
    lock = _three_ways(hip_lib, oracle_out, prob, ys, sres, cap, ppw, what=what, **kw)
    _flat_both_directions(hip_lib, oracle_out, prob, ys, sres, cap, ppw, what, **kw)
    return lock


# ---- the smallest knot counts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nJ", [1, 7, 8])
def test_paths_of_four_to_seven_knots(hip_lib, oracle_ctx, nJ):
    """eight paths of 4, 5, 6, 7, 4, 5, 6, 7 knots in one wavefront.  On three segments the forward prefetch is clamped from the second
    change on (knot 4 of 0..3 does not exist), the reverse one from the second change on as well (knot -1).  From the oracle: no path
    ends early, and every path takes more steps than it has segments in both directions, so every segment is entered by a change"""
    rng = np.random.default_rng(500 + nJ)
    prob = _problem(rng, nJ)
    lengths = (4, 5, 6, 7, 4, 5, 6, 7)
    ys = [random_knots(rng, nJ, n, rng.uniform(0.5, 2.0)) for n in lengths]
    sres = [float(rng.uniform(0.05, 0.2)) for _ in lengths]
    cap = 8000
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap)
    ro = oracle_out[0]
    assert not np.any(ro["status_fwd"]) and not np.any(ro["status_rev"] & ~np.uint32(capi.ST_SHORT))
    for k, n in enumerate(lengths):
        assert int(ro["steps_rev"][k]) > 2 * (n - 1) and int(ro["steps_fwd"][k]) > 2 * (n - 1), (k, n, ro["steps_rev"][k], ro["steps_fwd"][k])
    _all_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT), ys, sres, cap, 8, f"4 to 7 knots, {nJ} joints")


# ---- knot spacings from a fraction of a stage to dozens of steps, in one wavefront ------------------------------------------------------

SPACING_KNOTS = (3600, 600, 300, 150, 75, 38, 12, 6)


def _spacing_population(nJ=7, n_paths=8, seed=612, knots=SPACING_KNOTS, integ_res=0.08):
    """paths of the same length in s (1.5) and the same kind of shape with 3600 down to 6 knots: about the same number of steps each, so
    the segments per step go from some twenty down to a few hundredths"""
    rng = np.random.default_rng(seed)
    prob = _problem(rng, nJ, integ_res=integ_res)   # (0.08, a coarse step: a hundred to two hundred steps per path)
    lengths = [knots[k % len(knots)] for k in range(n_paths)]
    ys = [random_knots(rng, nJ, n, 1.0) for n in lengths]
    sres = [1.5 / (n - 1) for n in lengths]
    return prob, lengths, ys, sres, 20000


def _assert_spacings(ro, lengths):
    """from the oracle's rows: the densest paths cross two or more segments per stage on average (a step has six stages; the smallest
    stage increment is 4/45 of a step, so 23 segments per step), the sparsest stay at least ten steps on a segment, and the ratios
    between span the issue's range of 50 and more"""
    assert not np.any(ro["status_fwd"]) and not np.any(ro["status_rev"])
    per_step_fwd = np.array([(n - 1) / float(s) for n, s in zip(lengths, ro["steps_fwd"])])
    per_step_rev = np.array([(n - 1) / float(s) for n, s in zip(lengths, ro["steps_rev"])])
    for per_step in (per_step_fwd, per_step_rev):
        assert per_step.max() >= 12.0, per_step        # two segments per stage of a six-stage step, on average
        assert per_step.min() <= 0.1, per_step         # ten steps and more per segment
        assert np.sum((per_step > 0.25) & (per_step < 4.0)) >= 2, per_step   # and the ordinary case between
    return per_step_fwd, per_step_rev


@pytest.fixture(scope="module")
def spacing8(oracle_ctx):
    prob, lengths, ys, sres, cap = _spacing_population()
    return prob, lengths, ys, sres, cap, _run(oracle_ctx, prob, ys, sres, cap)


def test_knot_spacings_from_a_fraction_of_a_stage_to_dozens_of_steps(hip_lib, spacing8):
    prob, lengths, ys, sres, cap, oracle_out = spacing8
    _assert_spacings(oracle_out[0], lengths)
    _all_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT), ys, sres, cap, 8, "knot spacings, one wavefront")


def test_two_joints_per_lane(hip_lib, spacing8):
    """the same wavefront through k_sweep8<4, -1, +-1> (G = 4: joints j and j + 4 in lane j, two knot windows per lane) at 7 joints"""
    prob, lengths, ys, sres, cap, oracle_out = spacing8
    _assert_spacings(oracle_out[0], lengths)
    _flat_both_directions(hip_lib, oracle_out, _with_flags(prob, COMPACT), ys, sres, cap, 8, "knot spacings, G = 4", group=4)


@pytest.fixture(scope="module")
def spacing11(oracle_ctx):
    prob, lengths, ys, sres, cap = _spacing_population(n_paths=11, seed=613)
    return prob, lengths, ys, sres, cap, _run(oracle_ctx, prob, ys, sres, cap)


@pytest.mark.parametrize("ppw", [3, 5])
def test_partly_filled_wavefronts(hip_lib, spacing11, ppw):
    """11 paths at 3 and 5 paths per wavefront: lane groups that are idle from the start, and a last wavefront with 2 and 1 paths"""
    prob, lengths, ys, sres, cap, oracle_out = spacing11
    assert len(ys) % ppw != 0
    _assert_spacings(oracle_out[0], lengths)
    _all_ways(hip_lib, oracle_out, _with_flags(prob, COMPACT), ys, sres, cap, ppw, f"knot spacings, {ppw} paths per wavefront")


# ---- paths that end early while their neighbours go on changing segments ------------------------------------------------------------------

def test_paths_that_end_by_capacity_and_by_the_time_limit(hip_lib, oracle_ctx):
    """the spacing population, two paths of it five times the size of the others (knot values and spacing).  A capacity between the others' point counts and
    theirs ends both long paths in the reverse sweep (BATOTP_ST_CAPACITY) while the six others go on; then, at an ample capacity, a time
    limit between the others' durations and theirs ends them by BATOTP_ST_MAX_INTEG_TIME.  From the oracle: exactly the long paths carry
    a nonzero status, the others none, and the others take more steps than the long ones were allowed"""
    prob, lengths, ys, sres, _ = _spacing_population(seed=614)
    long_ones = (1, 4)
    for k in long_ones:
        sres[k] *= 5.0
        ys[k] = np.ascontiguousarray(ys[k] * 5.0)
    others = [k for k in range(len(ys)) if k not in long_ones]
    free = _run(oracle_ctx, prob, ys, sres, 60000)[0]
    assert not np.any(free["status_fwd"]) and not np.any(free["status_rev"])
    n_others = max(int(free["n_rev"][others].max()), int(free["n_fwd"][others].max()))
    n_long = min(int(free["n_rev"][list(long_ones)].min()), int(free["n_fwd"][list(long_ones)].min()))
    assert n_long > 1.5 * n_others, (n_long, n_others)
    p = _with_flags(prob, COMPACT)
    # by capacity
    cap = (n_others + n_long) // 2
    oracle_out = _run(oracle_ctx, prob, ys, sres, cap)
    ro = oracle_out[0]
    for k in range(len(ys)):
        ended = ((int(ro["status_rev"][k]) | int(ro["status_fwd"][k])) & capi.ST_CAPACITY) != 0
        assert ended == (k in long_ones), (k, ro["status_rev"][k], ro["status_fwd"][k])
    assert int(ro["steps_rev"][others].min()) > 50 and int(ro["steps_fwd"][others].min()) > 50   # the neighbours go on
    _all_ways(hip_lib, oracle_out, p, ys, sres, cap, 8, f"capacity {cap}")
    # by the time limit
    t_others = max(float(free["t_rev"][others].max()), float(free["t_total"][others].max()))
    t_long = min(float(free["t_rev"][list(long_ones)].min()), float(free["t_total"][list(long_ones)].min()))
    assert t_long > 1.5 * t_others
    prob.max_integ_time = 0.5 * (t_others + t_long)
    p = _with_flags(prob, COMPACT)
    oracle_out = _run(oracle_ctx, prob, ys, sres, 60000)
    ro = oracle_out[0]
    for k in range(len(ys)):
        late = ((int(ro["status_rev"][k]) | int(ro["status_fwd"][k])) & capi.ST_MAX_INTEG_TIME) != 0
        assert late == (k in long_ones), (k, ro["status_rev"][k], ro["status_fwd"][k])
    _all_ways(hip_lib, oracle_out, p, ys, sres, 60000, 8, "time limit")


# ---- the lean layout of the headline ----------------------------------------------------------------------------------------------------

def test_lean_layout_ample_and_tight(hip_lib, oracle_ctx):
    """BATOTP_F_CURVES_IN_PLACE | BATOTP_F_MVC_IN_CURVES (the layout of the headline batch): 11 paths of 150 down to 6 knots at a
    quarter of the other tests' integration step (the pointwise values of a path, one and a half times its knot count, must fit its
    curve slot, so the curves have to be longer than that), once with ample capacity, once with the tightest capacity at which the
    general kernel, which has no window, ends some paths, not all, by capacity -- the same paths must end, with the same rows.  From
    the oracle: between a segment every three steps and one every ten and more"""
    prob, lengths, ys, sres, _ = _spacing_population(n_paths=11, seed=616, knots=(150, 75, 38, 12, 6), integ_res=0.02)
    p = _with_flags(prob, COMPACT | LEAN)
    floor = (3 * max(lengths) + 1) // 2
    ample = 20000
    oracle_out = _run(oracle_ctx, p, ys, sres, ample, pointwise=True)
    ro = oracle_out[0]
    assert not np.any(ro["status_fwd"]) and not np.any(ro["status_rev"])
    per_step = np.array([(n - 1) / float(s) for n, s in zip(lengths, ro["steps_fwd"])])
    assert per_step.max() > 0.25 and per_step.min() <= 0.1, per_step
    got = _all_ways(hip_lib, oracle_out, p, ys, sres, ample, 8, "lean layout, ample", pointwise=True)
    assert int(got[0]["n_fwd"].min()) > floor
    ctx = _general_ctx(hip_lib, 8)
    tight = None
    for cap in sorted({max(floor, int(n) + 40) for n in got[0]["n_fwd"]}, reverse=True):
        r = _run(ctx, p, ys, sres, cap, pointwise=True)[0]
        full = ((r["status_fwd"] | r["status_rev"]) & capi.ST_CAPACITY) != 0
        if 0 < full.sum() < len(ys) and np.any((r["status_fwd"] & capi.ST_CAPACITY) != 0):
            tight = cap
            break
    ctx.close()
    assert tight is not None, "no capacity at which the general kernel ends some paths by capacity"
    oracle_out = _run(oracle_ctx, p, ys, sres, tight, pointwise=True)
    got = _all_ways(hip_lib, oracle_out, p, ys, sres, tight, 8, f"lean layout, capacity {tight}", pointwise=True)
    full = (got[0]["status_fwd"] & capi.ST_CAPACITY) != 0
    assert 0 < full.sum() < len(ys)
