"""What happens to the taught points before the resampler's first arc-length pass -- close-point removal, the stretch of short
paths, input smoothing / decimation / smoothing -- restated in plain Python (tests/conditioning_reference.py) and compared with
the checker, bit for bit: stage 0 of a traced one-path call is the checksum of exactly these rows (all rows, after the cable
lengths of the cable robot were recomputed from the filtered platform position, include/batotp_hip.h).  The same cases run
against the device in tests/test_gpu_taught_conditioning.py, which takes its shapes and builders from here."""
import numpy as np
import pytest

import conditioning_reference as cr
from batotp_amd import capi
from helpers import ResampleCase, assert_bit_equal

DECIMS = (2, 3, 4, 5, 6, 7, 9, 16)
SMOOTH_WINDOWS = (1, 3)
RESTATED_KINDS = ("synth_gen7dof_s0", "synth_cspr_s3")                     # GENJNT joint paths, cable paths
KINDS = RESTATED_KINDS + ("KUKA_cartacc", "UR5", "UR5_pos3")              # + forward kinematics, poses, positions taught with joints


def prefix_lengths(d, n_taught):
    """3d decimates to three points (refused); 3d+1 .. 7d leave 4 .. 7 points, where the second smoothing's window is clamped to
    the path length; 4d+1 is the exact fit of the decimation (the last kept sample is the regular one)"""
    return [3 * d, 3 * d + 1, 3 * d + 2, 4 * d, 4 * d + 1, 5 * d + 1, 6 * d + 1, 7 * d, min(n_taught, 40 * d + 3)]


def with_windows(params, d, smooth_window, thresh=None):
    p = capi.ResampleParams.from_buffer_copy(bytes(params))
    p.input_decim_fact, p.smooth_window = d, smooth_window
    if thresh is not None:
        p.jnt_thresh = p.cart_thresh = thresh
    return p


def is_cable(p):
    return p.path_type == capi.PATH_CART


def driving_rows(p):
    return range(p.n_joints, p.n_joints + p.n_cart) if is_cable(p) else range(0, p.n_joints)


_taught = {}


def taught_points(name):
    """(ResampleCase, its taught points from where the path moves): the UR5 recordings begin with the arm at rest -- its joints
    jitter by hundredths of a degree, and a prefix whose joint arc length stays below the joint resolution ends as "all points
    identical" -- so their slices start at the first taught step that is at least one joint resolution long"""
    if name not in _taught:
        c = ResampleCase(name)
        x = c.x
        if name.startswith("UR5"):
            step = np.sqrt(np.sum(np.diff(x[:c.params.n_joints], axis=1) ** 2, axis=0))
            first = int(np.argmax(step >= c.params.theta_norm_res))
            assert 0 < first < 30
            x = np.ascontiguousarray(x[:, first:])
        _taught[name] = (c, x)
    return _taught[name]


def restated(p, x, sres):
    """the conditioned rows of a GENJNT joint path or a cable path by the plain restatement: ([C][n'] array, sres', status)"""
    nJ = p.n_joints
    rows = [list(map(float, r)) for r in x]
    if is_cable(p):
        y, s, st = cr.condition(rows, sres, driving_rows(p), p.cart_thresh, p.input_decim_fact, p.smooth_window)
        if not st:
            y = cr.cable_lengths(y, nJ, list(p.pmat))       # the joint rows follow the filtered platform position
    else:
        assert p.path_type == capi.PATH_JOINT and p.robot_type == capi.ROBOT_GENJNT
        for c in range(nJ, len(rows)):
            rows[c] = [0.0] * len(rows[c])                  # a robot without kinematic model carries zero Cartesian rows
        y, s, st = cr.condition(rows, sres, driving_rows(p), p.jnt_thresh, p.input_decim_fact, p.smooth_window)
    return np.array(y, dtype=np.float64), s, st


def traced_one_path(ctx, p, x, sres):
    """(status, stage-0 checksum, knots or None, n_knots, sres) of a one-path call on a context that keeps the stage trace"""
    r = capi.Resampled(ctx, p, [np.ascontiguousarray(x)], [sres])
    st = int(r.status[0])
    out = (st, int(r.trace()[0]) if not st else None, r.knots(0) if not st else None, int(r.n_knots[0]), float(r.sres[0]))
    r.close()
    return out


# ---- close points: taught paths built on the parameters of a golden case, threshold 2^-10 -----------------------------------------
CLOSE_THRESH = 2.0 ** -10


def _runs(x, where, length):
    """x with point `where` repeated so that `length` identical points stand there"""
    cols = list(range(where + 1)) + [where] * (length - 1) + list(range(where + 1, x.shape[1]))
    return np.ascontiguousarray(x[:, cols])


STEP = 2.0 ** -4


def _staircase(p, n, steps, start=0.0):
    """a path on which only the first driving channel moves: `start`, then the running sum of `steps`, then steps of 2^-4 up to n
    points; every other row constant at 0.5.  With steps that are sums of few powers of two around 0 the coordinates, their
    differences and the squared distances are exact"""
    C = p.n_joints + p.n_cart
    x = np.full((C, n), 0.5)
    inc = list(steps) + [STEP] * (n - 1 - len(steps))
    x[list(driving_rows(p))[0]] = np.cumsum([start] + inc)
    return x


def close_point_paths(name):
    """{label: taught points} on the parameters of `name` (used with threshold CLOSE_THRESH)"""
    c, x = taught_points(name)
    p = c.params
    base = np.ascontiguousarray(x[:, :160])
    assert np.min(np.sum(np.diff(base[list(driving_rows(p))], axis=1) ** 2, axis=0)) > 4 * CLOSE_THRESH ** 2   # nothing close by itself
    out = {}
    for k in (2, 3, 4, 5):
        out[f"run{k}_interior"] = _runs(base, 77, k)
        out[f"run{k}_start"] = _runs(base, 0, k)
        out[f"run{k}_end"] = _runs(base, base.shape[1] - 1, k)          # the tail rule
    out["ends_as_three"] = _runs(_runs(np.ascontiguousarray(base[:, :3]), 2, 4), 0, 3)      # 3 distinct points among 8
    out["ends_as_two"] = _runs(_runs(np.ascontiguousarray(base[:, :2]), 1, 5), 0, 2)        # 2 distinct points among 7
    t = CLOSE_THRESH
    # three consecutive points, each closer than the threshold to its predecessor, the first and third further apart: only the
    # middle one goes
    out["chain_of_three"] = _staircase(p, 40, [STEP, STEP, 0.75 * t, 0.75 * t, STEP])
    # one step of exactly the threshold (not strictly closer: kept) / of the next double below it (dropped), taken from
    # coordinate 0 so that the step is the difference of the two coordinates exactly
    out["step_at_threshold"] = _staircase(p, 40, [STEP, STEP, t], start=-2 * STEP)
    out["step_below_threshold"] = _staircase(p, 40, [STEP, STEP, float(np.nextafter(t, 0.0))], start=-2 * STEP)
    for label in ("step_at_threshold", "step_below_threshold"):
        row = out[label][list(driving_rows(p))[0]]
        assert row[2] == 0.0 and row[3] == (t if label == "step_at_threshold" else np.nextafter(t, 0.0)) and row[3] - row[2] == row[3]
    # two neighbours that differ in the rows that do NOT drive only (dropped) / whose driving rows differ (kept)
    other = [r for r in range(p.n_joints + p.n_cart) if r not in driving_rows(p)]
    only_other = _runs(base, 50, 2)
    only_other[other, 51] += 0.25
    out["only_other_rows_differ"] = only_other
    flat_other = base.copy()
    flat_other[other] = 0.5                                  # ... and the reverse: the rows that do not drive never change
    out["other_rows_constant"] = flat_other
    return out


def expected_kept(label, n_in):
    """how many points close-point removal must leave, where the construction says so"""
    if label.startswith("run"):
        return n_in - (int(label[3]) - 1)
    return {"chain_of_three": n_in - 1, "step_at_threshold": n_in, "step_below_threshold": n_in - 1, "only_other_rows_differ": None, "other_rows_constant": n_in,
            "ends_as_three": 3, "ends_as_two": 2}[label]


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced(oracle_lib):
    ctx = capi.Context(oracle_lib, 0)
    ctx.set_resample_trace(True)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", RESTATED_KINDS)
@pytest.mark.parametrize("d", DECIMS)
def test_restatement_equals_the_checkers_conditioned_rows(traced, name, d):
    """window x length matrix: stage 0 of the checker (all rows; for the cable robot after the cable lengths were recomputed) =
    the checksum of the restatement's rows; a prefix of 3d points is refused by both, every longer one accepted by both"""
    c, x = taught_points(name)
    for sw in SMOOTH_WINDOWS:
        p = with_windows(c.params, d, sw)
        for n in prefix_lengths(d, x.shape[1]):
            st, sum0, _, _, _ = traced_one_path(traced, p, x[:, :n], c.sres_in)
            y, sres, rst = restated(p, x[:, :n], c.sres_in)
            assert (st != 0) == (n == 3 * d) and st == rst, (name, d, sw, n, st, rst)
            if st:
                continue
            assert y.shape[1] == (n - 1) // d + 1 and sres == c.sres_in * d, (name, d, sw, n, y.shape, sres)
            assert cr.stage_checksum(y) == sum0, (name, d, sw, n)


@pytest.mark.parametrize("name", RESTATED_KINDS)
def test_restatement_equals_the_checker_on_close_points(traced, name):
    c, _ = taught_points(name)
    for d, sw in ((1, 1), (5, 3)):
        p = with_windows(c.params, d, sw, CLOSE_THRESH)
        for label, x in close_point_paths(name).items():
            st, sum0, _, _, _ = traced_one_path(traced, p, x, c.sres_in)
            y, _, rst = restated(p, x, c.sres_in)
            assert st == rst, (name, label, d, st, rst)
            kept = cr.remove_close_points([list(r) for r in x], driving_rows(p), CLOSE_THRESH)
            want = expected_kept(label, x.shape[1])
            if label == "only_other_rows_differ":
                # the cable robot's joint rows and the Cartesian rows of a joint path do not drive: the pair counts as one point
                want = x.shape[1] - 1
                moved = x.copy()
                moved[list(driving_rows(p))[0], 51:] += 0.25          # ... whereas a step in a driving row is kept
                assert len(cr.remove_close_points([list(r) for r in moved], driving_rows(p), CLOSE_THRESH)[0]) == x.shape[1]
            assert len(kept[0]) == want, (name, label, len(kept[0]), want)
            if not st:
                assert cr.stage_checksum(y) == sum0, (name, label, d)
            else:
                assert label in ("ends_as_three", "ends_as_two") and d == 5   # four points decimate to one


@pytest.mark.parametrize("name", RESTATED_KINDS)
def test_settings_that_smooth_nothing_are_identities(oracle_ctx, name):
    """half width = w/2 + w%2 - 1 of the DECIMATION factor: factor 2 smooths nothing whatever smooth_window says, and factor 1
    with smooth_window 3 is no filter at all -- on the restatement's rows and on the checker's knots"""
    c, x = taught_points(name)
    x = np.ascontiguousarray(x[:, :333])
    knots, rows = {}, {}
    for d, sw in ((2, 1), (2, 3), (1, 1), (1, 3)):
        p = with_windows(c.params, d, sw)
        r = capi.Resampled(oracle_ctx, p, [x], [c.sres_in])
        assert int(r.status[0]) == 0
        knots[d, sw] = r.knots(0)
        r.close()
        rows[d, sw] = restated(p, x, c.sres_in)[0]
    for d in (1, 2):
        assert_bit_equal(rows[d, 1], rows[d, 3], f"{name}: restated rows, factor {d}")
        assert_bit_equal(knots[d, 1], knots[d, 3], f"{name}: knots, factor {d}")
    assert rows[2, 1].shape[1] == 167 and not np.array_equal(knots[1, 1], knots[2, 1])


def with_a_constant_row(p, x, value=0.125):
    """x with its last driving row held at 2^-3: k equal values sum exactly, so every window average is the value itself"""
    x = np.ascontiguousarray(x).copy()
    x[list(driving_rows(p))[-1]] = value
    return x


@pytest.mark.parametrize("name", RESTATED_KINDS)
@pytest.mark.parametrize("d", DECIMS)
def test_filters_keep_the_end_points_and_constant_rows(oracle_ctx, name, d):
    """the first and the last conditioned point of every driving row are the taught ones, bit for bit (on the restatement's rows,
    which the stage-0 checksums tie to the checker's; the KNOTS at both ends come out of a spline evaluation and may differ from
    the taught values in the last bit); a constant row stays constant for every window, in the conditioned rows and in the knots"""
    c, x = taught_points(name)
    rows = list(driving_rows(c.params))
    for sw in SMOOTH_WINDOWS:
        p = with_windows(c.params, d, sw)
        xs = [with_a_constant_row(p, x[:, :n]) for n in prefix_lengths(d, x.shape[1])[1:]]
        r = capi.Resampled(oracle_ctx, p, xs, [c.sres_in] * len(xs))
        assert not r.status.any()
        for k, xin in enumerate(xs):
            y, _, st = restated(p, xin, c.sres_in)
            what = f"{name} d={d} sw={sw} n={xin.shape[1]}"
            assert st == 0
            assert_bit_equal(y[rows, 0], xin[rows, 0], what + ": first point")
            assert_bit_equal(y[rows, -1], xin[rows, -1], what + ": last point")
            assert np.all(y[rows[-1]] == 0.125), what
            assert np.all(r.knots(k)[rows[-1]] == 0.125), what + ": knots"
        r.close()


def test_stage_checksum_is_the_sum_the_knot_checksum_test_spells_out():
    rng = np.random.default_rng(3)
    y = rng.normal(size=(5, 37))

    def mix(v):
        v = v ^ (v >> np.uint64(30)); v = v * np.uint64(0xBF58476D1CE4E5B9)
        v = v ^ (v >> np.uint64(27)); v = v * np.uint64(0x94D049BB133111EB)
        return v ^ (v >> np.uint64(31))
    with np.errstate(over="ignore"):
        bits = y.reshape(-1).view(np.uint64)
        idx = (np.arange(bits.size, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        assert int(mix(bits ^ idx).sum(dtype=np.uint64)) == cr.stage_checksum(y.tolist())
