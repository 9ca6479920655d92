"""GPU (-m gpu): the clamp chain of a sweep stage's prologue in its one-instruction form (batotp_amd/csrc/device_math.h:
clamp_chain_fast / clamp_chain_literal) and the guards that combine the masks of their comparisons (S8_MASK, sweep8.hip.h).

1. Small ragged batches, 9 to 17 paths of 300 to 3000 knots (a full and a partly filled wavefront), from the GEN7DOF and the 6-DOF
   path generators of the benchmark (batotp_amd/pathgen.py), as compact pairs and as coefficient rows, with curves in place and not,
   each through every form that shares the code: k_sweep8_lock, the flat k_sweep8 forward (flat form 2), the flat reverse sweep at
   certificate hold 3 and 0, and two joints per lane (G = 4).  Result rows and both curves are bit-equal to the oracle's
   (as tests/test_gpu_knot_window.py compares them).  The batches are configured so that each clamp binds somewhere, and each case
   asserts that from the ORACLE's curves:
     * joint velocity limits tight enough that lim1 decides most points of the forward curve;
     * a low sdotCap (a path that three integration steps cover): sdotCap = s_end / h is a thousandth of what the joints would allow;
     * the forward sweep riding the reverse curve (the points of the forward curve lie on the reverse curve's polyline);
     * a path with a standing start (all joints stand still over the first knots: no joint limits the speed there);
     * a path whose acceleration cap 2 s_end / h^2 overflows: its reverse sweep meets stage values that are not finite (inf - inf)
       and takes the literal route; the forward sweep does not run for it;
     * sdotMin = 0: reached in the reverse sweep with jnt_acc_max[0] = 0 (the bootstrap's 0.1 h w0 is 0 where joint 0 moves); such a
       path runs the literal chain in every stage.  sdotMin < 0, and sdotMin <= 0 in the forward sweep, are not reached by any input
       tried (test_zero_sdot_min_runs_the_literal_chain says why): the known-answer test covers that branch alone.
2. The known-answer test of the chain on the device (batotp_hip_clamp_kat, include/batotp_hip_clamp_kat.h)."""
import itertools

import numpy as np
import pytest

from batotp_amd import capi, pathgen
from test_gpu_sweep8_lockstep import COMPACT, _run, _with_flags
from test_gpu_knot_window import LEAN, _all_ways, _flat_both_directions

pytestmark = pytest.mark.gpu

DEG = 3.14159265358979323846 / 180.0


def _gen(kind, seed, n):
    """n knots of one generated path, [joints][n] float64 (gen7: 7 joints, values in [0, 5]; ur6: 6 joints, degrees -> radians)"""
    n_coarse = n // 20 + 2
    x = np.asarray(pathgen.gen7dof_fine(seed, n_coarse) if kind == "gen7" else pathgen.ur_like_fine(seed, n_coarse), dtype=np.float64)
    nJ = 7 if kind == "gen7" else 6
    if x.shape[0] != nJ:
        x = x.T
    assert x.shape[0] == nJ and x.shape[1] >= n, x.shape
    return np.ascontiguousarray(x[:, :n] * (1.0 if kind == "gen7" else DEG))


def _lengths(rng, n_paths):
    ns = [300, 3000] + [int(v) for v in rng.integers(300, 3001, n_paths - 2)]
    rng.shuffle(ns)
    return ns


def _batch(kind, seed, n_paths, vmax, amax, integ_res, sres=0.01):
    rng = np.random.default_rng(seed)
    nJ = 7 if kind == "gen7" else 6
    prob = capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=[vmax] * nJ, jnt_acc_max=[amax] * nJ, integ_res=integ_res,
                             max_integ_time=1e5)
    ns = _lengths(rng, n_paths)
    ys = [_gen(kind, 9000 + seed * 100 + k, n) for k, n in enumerate(ns)]
    return prob, ys, [sres] * n_paths


def _on_reverse_curve(fwd, rev):
    """fraction of the forward curve's points that lie on the reverse curve's polyline (relative 1e-9)"""
    s, v = fwd
    want = np.interp(s, rev[0], rev[1])
    return float(np.mean(np.abs(v - want) <= 1e-9 * np.maximum(np.abs(want), 1e-300)))


def _theta_prime_bound(y, sres, s, vmax):
    """min over the joints of vmax / |theta'| at the positions s, theta' by central differences of the knots: what lim1 is, roughly"""
    d = np.abs(np.gradient(y, sres, axis=1))
    at = np.clip(np.rint(s / sres).astype(int), 0, y.shape[1] - 1)
    return vmax / np.maximum(d[:, at].max(axis=0), 1e-300)


def _check(hip_lib, oracle_ctx, prob, ys, sres, cap, what, flagsets, claim=None, ppw=8):
    """one oracle run per flag set (the layouts do not change the results, the lean layout needs the pointwise values in the curves),
    the claim about the batch asserted on it, then every form of the kernels"""
    for flags in flagsets:
        lean = bool(flags & capi.F_CURVES_IN_PLACE)
        p = _with_flags(prob, flags)
        oracle_out = _run(oracle_ctx, p if lean else prob, ys, sres, cap, pointwise=lean)
        if claim is not None:
            claim(oracle_out)
        tag = f"{what}, flags {flags:#x}"
        _all_ways(hip_lib, oracle_out, p, ys, sres, cap, ppw, tag, pointwise=lean)
        _flat_both_directions(hip_lib, oracle_out, p, ys, sres, cap, ppw, tag + ", G = 4", group=4, pointwise=lean)


CASES = [
    # (id, generator, paths, flag sets)
    ("gen7-17-compact", "gen7", 17, (COMPACT,)),
    ("gen7-9-rows-and-lean", "gen7", 9, (0, COMPACT | LEAN)),
    ("ur6-13-compact", "ur6", 13, (COMPACT,)),
    ("ur6-11-rows", "ur6", 11, (0,)),
]


@pytest.mark.parametrize("name,kind,n_paths,flagsets", CASES, ids=[c[0] for c in CASES])
def test_ordinary_batches_ride_the_reverse_curve(hip_lib, oracle_ctx, name, kind, n_paths, flagsets):
    """the benchmark's limits in kind (velocity 5, acceleration 10 for gen7; 160 and 573 deg for the 6-DOF arm, in radians): the forward
    sweep accelerates from its start and then rides the reverse curve to the end -- from the oracle: on every path at least a fifth of
    the forward points lie on the reverse curve (the clamp against the interpolated reverse speed decides them)"""
    vmax, amax = (5.0, 10.0) if kind == "gen7" else (160 * DEG, 573 * DEG)
    prob, ys, sres = _batch(kind, 1 + n_paths, n_paths, vmax, amax, integ_res=0.02)

    def claim(out):
        ro = out[0]
        assert not np.any(ro["status_fwd"]) and not np.any(ro["status_rev"])
        on = [_on_reverse_curve(out[2][k], out[1][k]) for k in range(n_paths)]
        assert min(on) >= 0.2, on

    _check(hip_lib, oracle_ctx, prob, ys, sres, 40000, name, flagsets, claim)


@pytest.mark.parametrize("kind,n_paths", [("gen7", 12), ("ur6", 10)])
def test_velocity_limits_decide_most_stages(hip_lib, oracle_ctx, kind, n_paths):
    """velocity limits a hundred times tighter than the acceleration limits need: lim1 = min_j vmax_j / |theta'_j| decides the speed
    nearly everywhere -- from the oracle: on every path more than half of the forward points have sdot within 2 % of that bound
    (theta' by central differences of the knots)"""
    vmax = 0.05 if kind == "gen7" else 1.6 * DEG
    amax = 10.0 if kind == "gen7" else 573 * DEG
    prob, ys, sres = _batch(kind, 40 + n_paths, n_paths, vmax, amax, integ_res=0.5)

    def claim(out):
        ro = out[0]
        assert not np.any(ro["status_fwd"]) and not np.any(ro["status_rev"])
        for k in range(n_paths):
            s, v = out[2][k]
            bound = _theta_prime_bound(ys[k], sres[k], s, vmax)
            assert np.mean(np.abs(v - bound) <= 0.02 * bound) > 0.5, (k, float(np.mean(np.abs(v - bound) <= 0.02 * bound)))

    _check(hip_lib, oracle_ctx, prob, ys, sres, 40000, f"tight velocity limits {kind}", (COMPACT, 0), claim)


def test_low_sdot_cap_and_a_standing_start(hip_lib, oracle_ctx):
    """11 gen7 paths; paths 2 and 7 are 300 knots over s_end = 0.0299 with h = 0.02 and joints that hardly move: sdotCap = s_end / h
    = 1.495 where the joint limits would allow thousands, and the acceleration cap 2 s_end / h^2 carries a stage value from rest past
    sdotCap within one step.  Path 4 stands still over its first 40 knots (no joint limits the speed there: lim1 = inf, the cap and the
    reverse curve decide).  From the oracle: both curves of the short paths start at sdotMin = 0.1 h (2 s_end / h^2) = 0.2 sdotCap and
    the paths are through in two to four steps.  (Whether a STAGE value was cut at sdotCap does not show in the published points;
    the known-answer test has the cap binding.)"""
    n_paths = 11
    prob, ys, sres = _batch("gen7", 77, n_paths, 5.0, 10.0, integ_res=0.02)
    short = (2, 7)
    for k in short:
        ys[k] = np.ascontiguousarray(ys[k][:, :300] * 1e-6)
        sres[k] = 1e-4
    ys[4][:, :40] = ys[4][:, 40:41]
    caps = {k: sres[k] * (ys[k].shape[1] - 1) / 0.02 for k in short}

    def claim(out):
        for k in short:
            assert np.isclose(float(out[2][k][1][0]), 0.2 * caps[k], rtol=1e-12) and np.isclose(float(out[1][k][1][-1]), 0.2 * caps[k], rtol=1e-12)
            assert 2 <= int(out[0]["steps_fwd"][k]) <= 4 and 2 <= int(out[0]["steps_rev"][k]) <= 4, out[0][k]
        assert not np.any(out[0]["status_fwd"] & ~np.uint32(capi.ST_SHORT))

    _check(hip_lib, oracle_ctx, prob, ys, sres, 40000, "low sdotCap, standing start", (COMPACT, COMPACT | LEAN), claim)


def test_overflowing_acceleration_cap_takes_the_literal_route(hip_lib, oracle_ctx):
    """9 ur6 paths; path 5 has a knot spacing of 1e302: s_end / h is finite and 2 s_end / h^2 is not, so the reverse sweep starts
    with an infinite acceleration and forms inf - inf in its second stage.  From the oracle: that path's reverse sweep ends without a
    usable curve or with BATOTP_ST_NONFINITE, and the other eight are untouched by it"""
    n_paths = 9
    prob, ys, sres = _batch("ur6", 91, n_paths, 160 * DEG, 573 * DEG, integ_res=0.02)
    sres[5] = 1e302

    def claim(out):
        ro = out[0]
        others = [k for k in range(n_paths) if k != 5]
        assert not np.any(ro["status_fwd"][others]) and not np.any(ro["status_rev"][others])
        rev = out[1][5]
        assert (int(ro["status_rev"][5]) != 0) or not (np.isfinite(rev[0]).all() and np.isfinite(rev[1]).all()), ro[5]

    _check(hip_lib, oracle_ctx, prob, ys, sres, 6000, "overflowing acceleration cap", (COMPACT, 0), claim)


def test_zero_sdot_min_runs_the_literal_chain(hip_lib, oracle_ctx):
    """jnt_acc_max[0] = 0 on 9 gen7 paths of 300 to 700 knots.  Where joint 0 moves at the start of a sweep the only admissible
    acceleration at rest is 0, so the bootstrap's w0 and with it sdotMin = 0.1 h w0 are 0: the fast chain's condition sdotMin > 0 fails
    for the whole path, which never gains speed and ends by capacity.  On paths 1 and 4 joint 0 stands still throughout and both
    sweeps finish; on paths 0, 3 and 6 it stands still over the last third, so the reverse sweep starts ordinarily and meets the joint
    later.  From the oracle: the paths whose joint 0 moves at the end of the path use up the capacity of the reverse sweep without a
    curve, the two others finish both sweeps.
    sdotMin < 0 is not reached by any input tried: with a negative acceleration limit the bootstrap's check is violated at rest, its
    bisection fails and w0 keeps a positive value (point 0 of every curve of test_gpu_sweep8_lockstep's failing batch is positive).  In
    the FORWARD sweep sdotMin <= 0 is not reached here either (a path whose joint 0 moves at s = 0 does not survive its reverse sweep):
    the known-answer test below covers that branch of the lockstep kernel's condition alone."""
    rng = np.random.default_rng(5)
    nJ, n_paths, cap = 7, 9, 1500
    prob = capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=[5.0] * nJ, jnt_acc_max=[0.0] + [10.0] * (nJ - 1), integ_res=0.02,
                             max_integ_time=1e5)
    ys = [_gen("gen7", 700 + k, int(n)) for k, n in enumerate(rng.integers(300, 701, n_paths))]
    for k in (0, 3, 6):
        n = ys[k].shape[1]
        ys[k][0, 2 * n // 3:] = ys[k][0, 2 * n // 3]
    for k in (1, 4):
        ys[k][0, :] = ys[k][0, 0]
    sres = [0.01] * n_paths

    def claim(out):
        ro = out[0]
        for k in (2, 5, 7, 8):
            assert int(ro["steps_rev"][k]) == cap and int(ro["n_rev"][k]) == 0 and (int(ro["status_rev"][k]) & capi.ST_CAPACITY), ro[k]
        for k in (1, 4):
            assert int(ro["n_rev"][k]) > 4 and int(ro["status_rev"][k]) == 0, ro[k]

    _check(hip_lib, oracle_ctx, prob, ys, sres, cap, "sdotMin = 0", (COMPACT,), claim)


# ---- the known-answer test of the chain -----------------------------------------------------------------------------------------------

def _np_dmax(a, b):
    return np.where(a < b, b, a)    # std::max(a, b) = (a < b) ? b : a


def _np_dmin(a, b):
    return np.where(b < a, b, a)    # std::min(a, b) = (b < a) ? b : a


def _np_literal(raw, interp, cap, smin, lim1):
    with np.errstate(invalid="ignore"):
        v = _np_dmax(raw, np.zeros_like(raw))
        m = _np_dmax(interp, smin)
        v = np.where(v > m, m, v)
        v = _np_dmin(v, cap)
        v = _np_dmax(v, smin)
        return _np_dmin(v, lim1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_clamp_chain_known_answers(hip_ctx):
    """every tuple (raw vN, raw interpolation, sdotCap, sdotMin, lim1) over {NaN, +-0, +-smallest denormal, +-1, two nearly equal normals,
    +-inf, 1e300} -- lim1 too, though the kernels only ever form a fabs or +inf -- plus 10^4 random finite tuples:
    (a) the device's literal chain equals the numpy restatement of the compare-and-select forms bit for bit;
    (b) wherever the validity flag is set, the one-instruction chain equals the literal one bit for bit;
    (c) the flag is set for EVERY tuple without a NaN among raw, interpolation and sdotCap and with sdotMin > 0, and cleared for
        every other one"""
    den = 4.9406564584124654e-324
    near = 1.0 + 2.0 ** -52
    vals = np.array([np.nan, 0.0, -0.0, den, -den, 1.0, -1.0, near, 1.0 - 2.0 ** -53, np.inf, -np.inf, 1e300])
    grid = np.array(list(itertools.product(vals, vals, vals, vals, vals)))
    rng = np.random.default_rng(2024)
    rnd = rng.standard_normal((10000, 5)) * 10.0 ** rng.uniform(-3, 3, (10000, 5))
    rnd[:, 4] = np.abs(rnd[:, 4])
    rnd[::2, 3] = np.abs(rnd[::2, 3])           # half of the random tuples with sdotMin > 0
    t = np.ascontiguousarray(np.concatenate([grid, rnd]).T)
    raw, interp, cap, smin, lim1 = t
    literal, fast, valid = capi.clamp_kat(hip_ctx, raw, interp, cap, smin, lim1)
    want = _np_literal(raw, interp, cap, smin, lim1)
    assert np.array_equal(_bits(literal), _bits(want)), int(np.sum(_bits(literal) != _bits(want)))          # (a)
    assert np.array_equal(_bits(fast)[valid], _bits(literal)[valid]), int(np.sum(_bits(fast)[valid] != _bits(literal)[valid]))   # (b)
    ok = ~np.isnan(raw) & ~np.isnan(interp) & ~np.isnan(cap) & (smin > 0.0)
    assert np.array_equal(valid, ok)                                                                        # (c)
    assert int(ok[: len(grid)].sum()) > 10000 and int(ok[len(grid):].sum()) > 4000    # the fast route is not vacuous
