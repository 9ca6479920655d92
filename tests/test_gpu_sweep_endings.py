"""GPU (-m gpu): the entry and the ending of a path in every sweep kernel (batotp_amd/csrc/sweep_frame.hip.h: the row of a path
without a reverse curve, the capacity rule, the time limit, the end snap, a curve of fewer than four points made four, the result row).

The four kernels share that code and differ in how they feed it: k_sweep and k_sweep1 read the early points of a short curve back
from the curve, the two 8-lane kernels keep them in registers and flush the last group of four points from LDS; two count steps in
64 bits and two in 32.  So every kernel, selected with the developer switches and with its launch asserted, runs small populations
that reach every ending, with compact pairs and with coefficient rows where it has both, and all result rows and both curves must
be bit-equal to the oracle's.  Each test first asserts on the oracle's own rows that the endings it is named for are there.

Not covered: a curve of TWO points.  None occurred in any oracle run of these paths (integration steps from 0.5 down to 0.004,
knot spacings from 0.01 to 0.2): a sweep that is through after one step did not turn up."""
import numpy as np
import pytest

from helpers import random_knots
from batotp_amd import capi
from test_gpu_sweep8_lockstep import COMPACT, _ragged_population, _run, _same, _with_flags

pytestmark = pytest.mark.gpu

# name: (lanes per path, paths per wavefront, hold (reverse, forward) or None, flat form or None, expected launch (reverse, forward),
#        knot layouts: True = compact pairs, False = coefficient rows)
KERNELS = {
    "k_sweep nested, 8 lanes": (8, 8, (-1, -1), 0, ((8, 8, -1), (8, 8, -1)), (True, False)),
    "k_sweep nested, 32 lanes": (32, 2, None, None, ((32, 2, -1), (32, 2, -1)), (True, False)),
    "k_sweep FLAT": (8, 8, (4, 8), 0, ((8, 8, 4), (8, 8, 8)), (True, False)),
    "k_sweep8 both directions": (8, 8, (4, 8), 2, ((8, 8, 4), (8, 8, 8)), (True, False)),
    "k_sweep8<4>": (4, 8, (4, 8), 2, ((4, 8, 4), (4, 8, 8)), (True, False)),
    "k_sweep8_lock": (8, 8, (4, 8), 1, ((8, 8, 4), (8, 8, 8)), (True, False)),
    "k_sweep1, one path per wavefront": (64, 1, None, None, ((64, 1, -1), (64, 1, -1)), (True, False)),
    "k_sweep1, two paths per wavefront": (64, 2, None, None, ((64, 2, -1), (64, 2, -1)), (True,)),
}
CASES = [pytest.param(name, compact, id=f"{name}-{'pairs' if compact else 'rows'}") for name, k in KERNELS.items() for compact in k[5]]


def _kernel_run(hip_lib, kernel, compact, pop):
    """the population through one kernel; launch asserted, everything bit-equal to the oracle"""
    prob, ys, sres, integ, cap, oracle_out = pop
    lanes, ppw, hold, form, launch, _ = KERNELS[kernel]
    ctx = capi.Context(hip_lib, 0)
    ctx.set_sweep_group(lanes)
    ctx.set_paths_per_wave(ppw)
    if hold is not None:
        ctx.set_sweep_hold(*hold)
    if form is not None:
        ctx.set_flat_form(form)
    got = _run(ctx, _with_flags(prob, COMPACT if compact else 0), ys, sres, cap, integ=integ, hip="both")
    ctx.close()
    assert got[3] == launch, (kernel, got[3])
    _same(got, oracle_out, f"{kernel}, {'pairs' if compact else 'rows'}: against the oracle")


def _va_problem(rng, nJ, max_integ_time=1e5):
    return capi.make_problem(nJ, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=list(rng.uniform(0.5, 8.0, nJ)), jnt_acc_max=list(rng.uniform(1.0, 40.0, nJ)),
                             integ_res=0.01, max_integ_time=max_integ_time)


def _paths():
    """7 joints: four ordinary paths of 40, 64, 90 and 33 knots, and six of 16 knots that hardly move (knots scaled by 1e-5: no
    limit applies and a sweep is through after a few steps -- how few depends on the integration step)"""
    rng = np.random.default_rng(77)
    prob = _va_problem(rng, 7)
    ordinary = [random_knots(rng, 7, n, rng.uniform(0.5, 2.0)) for n in (40, 64, 90, 33)]
    tiny = [np.ascontiguousarray(random_knots(rng, 7, 16, rng.uniform(0.5, 2.0)) * 1e-5) for _ in range(6)]
    return prob, ordinary, tiny


def _with_oracle(oracle_ctx, prob, ys, sres, integ, cap):
    return prob, ys, sres, integ, cap, _run(oracle_ctx, prob, ys, sres, cap, integ=integ)


# ---- short curves ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def short_curves(oracle_ctx):
    """ten paths: tiny ones at integration steps from 0.05 to 0.006 between three ordinary ones"""
    prob, ordinary, tiny = _paths()
    ys = [tiny[0], ordinary[0], tiny[1], tiny[2], ordinary[1], tiny[3], tiny[4], ordinary[3], tiny[5], tiny[1]]
    integ = [0.05, 0.01, 0.03, 0.02, 0.01, 0.015, 0.012, 0.01, 0.01, 0.006]
    return _with_oracle(oracle_ctx, prob, ys, [0.05] * len(ys), integ, 8000)


@pytest.mark.parametrize("kernel, compact", CASES)
def test_curves_of_three_to_six_points(hip_lib, short_curves, kernel, compact):
    """reverse curves of three points made four (BATOTP_ST_SHORT, two steps) and of exactly 4, 5 and 6 points, a forward curve of
    three points made four, between ordinary paths"""
    ro = short_curves[5][0]
    n_rev, short_rev = [int(v) for v in ro["n_rev"]], [bool(v & capi.ST_SHORT) for v in ro["status_rev"]]
    assert any(n == 4 and s and int(st) == 2 for n, s, st in zip(n_rev, short_rev, ro["steps_rev"])), "a reverse curve of three points made four"
    assert any(n == 4 and not s for n, s in zip(n_rev, short_rev)), "a reverse curve of four points"
    assert 5 in n_rev and 6 in n_rev, n_rev
    assert any(int(n) == 4 and int(st) == 2 and int(s) == capi.ST_SHORT for n, st, s in zip(ro["n_fwd"], ro["steps_fwd"], ro["status_fwd"])), \
        "a forward curve of three points made four"
    assert sum(n > 500 for n in n_rev) == 3, "three ordinary paths among them"
    _kernel_run(hip_lib, kernel, compact, short_curves)


@pytest.fixture(scope="module")
def forward_short(oracle_ctx):
    """6 joints: path 3 of the ragged population of tests/test_gpu_sweep8_lockstep.py (through after two forward steps behind a
    reverse curve of four points proper) between its paths of 16, 33, 57 and 90 knots"""
    prob, ys, sres, integ, _ = _ragged_population()
    pick = [0, 3, 7, 2, 8]
    return _with_oracle(oracle_ctx, prob, [ys[k] for k in pick], [sres[k] for k in pick], [integ[k] for k in pick], 4000)


@pytest.mark.parametrize("kernel, compact", CASES)
def test_forward_curve_of_three_points_made_four(hip_lib, forward_short, kernel, compact):
    ro = forward_short[5][0]
    assert int(ro["steps_fwd"][1]) == 2 and int(ro["n_fwd"][1]) == 4 and int(ro["status_fwd"][1]) == capi.ST_SHORT
    assert int(ro["n_rev"][1]) == 4 and not (int(ro["status_rev"][1]) & capi.ST_SHORT), "behind a reverse curve of four points proper"
    assert all(int(ro["n_fwd"][k]) > 100 and int(ro["status_fwd"][k]) == 0 for k in (0, 2, 3, 4))
    _kernel_run(hip_lib, kernel, compact, forward_short)


# ---- ordinary endings, capacity, time limit: the four ordinary paths -----------------------------------------------------------------

def _ordinary(oracle_ctx, cap=8000, max_integ_time=None):
    prob, ordinary, _ = _paths()
    if max_integ_time is not None:
        prob.max_integ_time = max_integ_time
    return _with_oracle(oracle_ctx, prob, ordinary, [0.05] * 4, None, cap)


@pytest.fixture(scope="module")
def ordinary(oracle_ctx):
    return _ordinary(oracle_ctx)


@pytest.mark.parametrize("kernel, compact", CASES)
def test_ordinary_endings_at_every_fill_of_the_last_group_of_four(hip_lib, ordinary, kernel, compact):
    """the 8-lane kernels flush the last, partly filled group of four points from LDS: curve lengths of every residue modulo 4"""
    ro = ordinary[5][0]
    assert not np.any(ro["status_rev"]) and not np.any(ro["status_fwd"]) and int(ro["n_rev"].min()) > 500
    assert {int(n) % 4 for n in ro["n_rev"]} | {int(n) % 4 for n in ro["n_fwd"]} == {0, 1, 2, 3}, (ro["n_rev"], ro["n_fwd"])
    _kernel_run(hip_lib, kernel, compact, ordinary)


@pytest.fixture(scope="module")
def capacity_reverse(oracle_ctx, ordinary):
    # (a curve of n points fits a capacity of n: one below the second-largest reverse curve ends the two largest)
    return _ordinary(oracle_ctx, cap=int(np.sort(ordinary[5][0]["n_rev"])[-2]) - 1)


@pytest.mark.parametrize("kernel, compact", CASES)
def test_capacity_ends_two_reverse_sweeps(hip_lib, capacity_reverse, kernel, compact):
    ro = capacity_reverse[5][0]
    full = (ro["status_rev"] & capi.ST_CAPACITY) != 0
    assert full.sum() == 2 and np.all(ro["n_rev"][full] == 0) and np.all(ro["steps_rev"][full] == capacity_reverse[4])
    assert np.all(ro["n_fwd"][full] == 0) and np.all(ro["status_fwd"][full] == capi.ST_CAPACITY), "and the row of a path without a reverse curve"
    assert np.all(ro["status_rev"][~full] == 0) and np.all(ro["status_fwd"][~full] == 0) and np.all(ro["n_fwd"][~full] > 500), "two finish"
    _kernel_run(hip_lib, kernel, compact, capacity_reverse)


@pytest.fixture(scope="module")
def capacity_forward(oracle_ctx, ordinary):
    return _ordinary(oracle_ctx, cap=int(ordinary[5][0]["n_fwd"].max()) - 2)


@pytest.mark.parametrize("kernel, compact", CASES)
def test_capacity_ends_one_forward_sweep(hip_lib, capacity_forward, kernel, compact):
    ro = capacity_forward[5][0]
    assert not np.any(ro["status_rev"]) and int(ro["n_rev"].min()) > 500, "every reverse sweep finishes"
    full = (ro["status_fwd"] & capi.ST_CAPACITY) != 0
    assert full.sum() == 1 and int(ro["n_fwd"][full][0]) == 0 and not np.any(ro["status_fwd"][~full])
    _kernel_run(hip_lib, kernel, compact, capacity_forward)


@pytest.fixture(scope="module")
def time_limit_reverse(oracle_ctx, ordinary):
    t = np.sort(ordinary[5][0]["t_total"])
    return _ordinary(oracle_ctx, max_integ_time=0.5 * float(t[1] + t[2]))   # between the second and the third smallest duration


@pytest.mark.parametrize("kernel, compact", CASES)
def test_time_limit_ends_two_reverse_sweeps(hip_lib, time_limit_reverse, kernel, compact):
    ro = time_limit_reverse[5][0]
    late = (ro["status_rev"] & capi.ST_MAX_INTEG_TIME) != 0
    assert late.sum() == 2 and np.all(ro["n_rev"][late] == 0) and np.all(ro["status_fwd"][late] == (capi.ST_MAX_INTEG_TIME | capi.ST_CAPACITY))
    assert not np.any(ro["status_rev"][~late]) and not np.any(ro["status_fwd"][~late]) and np.all(ro["n_fwd"][~late] > 500)
    _kernel_run(hip_lib, kernel, compact, time_limit_reverse)


@pytest.fixture(scope="module")
def time_limit_forward(oracle_ctx, ordinary):
    ro = ordinary[5][0]
    k = int(np.argmax(ro["t_total"] - ro["t_rev"]))   # the path whose forward sweep takes longest beyond its reverse sweep
    return _ordinary(oracle_ctx, max_integ_time=0.5 * float(ro["t_rev"][k] + ro["t_total"][k]))


@pytest.mark.parametrize("kernel, compact", CASES)
def test_time_limit_in_either_sweep(hip_lib, time_limit_forward, kernel, compact):
    """a limit between the durations of one path's two sweeps: paths that end by it in the reverse sweep (and get the row of a path
    without a reverse curve), in the forward sweep only, and not at all"""
    ro = time_limit_forward[5][0]
    late_rev = (ro["status_rev"] & capi.ST_MAX_INTEG_TIME) != 0
    late_fwd = ~late_rev & ((ro["status_fwd"] & capi.ST_MAX_INTEG_TIME) != 0)
    assert late_rev.sum() >= 1 and np.all(ro["status_fwd"][late_rev] == (capi.ST_MAX_INTEG_TIME | capi.ST_CAPACITY)) and np.all(ro["n_fwd"][late_rev] == 0)
    assert late_fwd.sum() >= 1 and np.all(ro["n_rev"][late_fwd] > 500) and np.all(ro["n_fwd"][late_fwd] == 0), "in the forward sweep only"
    assert (~late_rev & ~late_fwd).sum() >= 1 and not np.any(ro["status_fwd"][~late_rev & ~late_fwd])
    _kernel_run(hip_lib, kernel, compact, time_limit_forward)
