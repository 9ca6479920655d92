"""GPU (-m gpu): the four kernels in front of the resampler's first arc-length pass -- k_rs_close_any, k_rs_remclose (close-point
removal), k_rs_smooth and k_rs_decimate (input smoothing / decimation) -- against the checker and against the plain restatement
of tests/conditioning_reference.py, bit for bit: status, knot count, spacing and knots of every accepted path, and, for one-path
traced calls, the checksum of stage 0 (the conditioned rows themselves), which isolates these kernels from everything behind
them.  Shapes and path builders are those of tests/test_conditioning_cpu.py, where the restatement is compared with the checker."""
import numpy as np
import pytest

import conditioning_reference as cr
from batotp_amd import capi
from helpers import assert_bit_equal
from test_conditioning_cpu import (CLOSE_THRESH, DECIMS, KINDS, RESTATED_KINDS, SMOOTH_WINDOWS, close_point_paths, driving_rows,
                                   prefix_lengths, restated, taught_points, traced_one_path, with_a_constant_row, with_windows)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_traced(hip_lib):
    ctx = capi.Context(hip_lib, 0)
    ctx.set_resample_trace(True)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def oracle_traced(oracle_lib):
    ctx = capi.Context(oracle_lib, 0)
    ctx.set_resample_trace(True)
    yield ctx
    ctx.close()


def both(hip_ctx, oracle_ctx, p, xs, sres):
    """the batch on the device and on the checker; status, knot counts and spacings equal, knots of every accepted path equal.
    Returns (device result, checker result), open."""
    sr = [sres] * len(xs)
    h = capi.Resampled(hip_ctx, p, xs, sr)
    o = capi.Resampled(oracle_ctx, p, xs, sr)
    assert np.array_equal(h.status, o.status), (h.status, o.status)
    assert np.array_equal(h.n_knots, o.n_knots), (h.n_knots, o.n_knots)
    assert h.sres.tobytes() == o.sres.tobytes(), (h.sres, o.sres)
    for k in range(len(xs)):
        if not int(o.status[k]):
            assert_bit_equal(h.knots(k), o.knots(k), f"path {k} of {len(xs)} ({xs[k].shape[1]} taught points)")
    return h, o


def one_path_three_ways(hip_traced, oracle_traced, p, x, sres, what):
    """a traced one-path call on the device and on the checker: status, stage 0, knots equal; for the restated path kinds stage 0 is
    also the checksum of the restatement's rows.  Returns (status, device knots)."""
    hs, h0, hk, hn, hr = traced_one_path(hip_traced, p, x, sres)
    os_, o0, ok, on, or_ = traced_one_path(oracle_traced, p, x, sres)
    assert (hs, hn) == (os_, on) and np.float64(hr).tobytes() == np.float64(or_).tobytes(), (what, hs, os_, hn, on, hr, or_)
    if p.robot_type in (capi.ROBOT_GENJNT, capi.ROBOT_CSPR3DOF) and p.path_type != capi.PATH_BOTH:
        y, _, rst = restated(p, x, sres)
        assert rst == os_, (what, rst, os_)
        if not rst:
            assert cr.stage_checksum(y) == o0, f"{what}: restatement against the checker's stage 0"
    if not os_:
        assert h0 == o0, f"{what}: conditioned rows (stage 0) differ between device and checker"
        assert_bit_equal(hk, ok, f"{what}: knots of the one-path call")
    return hs, hk


# ---- a. window x length matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DECIMS)
@pytest.mark.parametrize("name", KINDS)
def test_window_length_matrix(hip_ctx, oracle_ctx, hip_traced, oracle_traced, name, d):
    """prefixes of 3d .. 40d+3 taught points as one ragged batch per (factor, smooth_window): 3d points decimate to three and are
    refused -- those paths and no others carry a status -- and 3d+1 .. 7d points leave 4 .. 7, where the window of the second
    smoothing is clamped to the path and, for d >= 9, all three branches of the moving average fall on a 5- or 6-point path; then
    every accepted prefix alone, traced"""
    c, x = taught_points(name)
    lens = prefix_lengths(d, x.shape[1])
    assert lens[-1] > lens[-2], (name, d, x.shape)
    xs = [np.ascontiguousarray(x[:, :n]) for n in lens]
    for sw in SMOOTH_WINDOWS:
        p = with_windows(c.params, d, sw)
        h, o = both(hip_ctx, oracle_ctx, p, xs, c.sres_in)
        assert [int(s) != 0 for s in o.status] == [True] + [False] * (len(lens) - 1), (name, d, sw, o.status)
        for k in range(1, len(lens)):
            _, hk = one_path_three_ways(hip_traced, oracle_traced, p, xs[k], c.sres_in, f"{name} d={d} sw={sw} n={lens[k]}")
            assert_bit_equal(h.knots(k), hk, f"{name} d={d} sw={sw} n={lens[k]}: inside the batch and alone")
        h.close(); o.close()


@pytest.mark.parametrize("name", KINDS)
def test_settings_that_smooth_nothing_give_the_same_knots_on_the_device(hip_ctx, oracle_ctx, name):
    """the half width comes from the decimation factor: factor 2 with smooth_window 1 and 3, factor 1 with 1 and 3"""
    c, x = taught_points(name)
    x = np.ascontiguousarray(x[:, :min(x.shape[1], 333)])
    knots = {}
    for d, sw in ((2, 1), (2, 3), (1, 1), (1, 3)):
        h, o = both(hip_ctx, oracle_ctx, with_windows(c.params, d, sw), [x], c.sres_in)
        assert int(h.status[0]) == 0
        knots[d, sw] = h.knots(0)
        h.close(); o.close()
    assert_bit_equal(knots[2, 1], knots[2, 3], f"{name}: factor 2")
    assert_bit_equal(knots[1, 1], knots[1, 3], f"{name}: factor 1")
    assert knots[1, 1].shape != knots[2, 1].shape or not np.array_equal(knots[1, 1], knots[2, 1])


@pytest.mark.parametrize("name", RESTATED_KINDS)
def test_a_constant_driving_row_stays_constant_on_the_device(hip_ctx, oracle_ctx, name):
    """value 2^-3: sums of k equal values are exact, so every window -- full, shrinking, clamped -- returns the value, and so do
    the splines behind the filter"""
    c, x = taught_points(name)
    row = list(driving_rows(c.params))[-1]
    for d in DECIMS:
        for sw in SMOOTH_WINDOWS:
            p = with_windows(c.params, d, sw)
            xs = [with_a_constant_row(p, x[:, :n]) for n in prefix_lengths(d, x.shape[1])[1:]]
            h, o = both(hip_ctx, oracle_ctx, p, xs, c.sres_in)
            assert not o.status.any()
            for k in range(len(xs)):
                assert np.all(h.knots(k)[row] == 0.125), (name, d, sw, xs[k].shape[1])
            h.close(); o.close()


# ---- b. batch plumbing around the filter ---------------------------------------------------------------------------------------------
def _with_every_4th_repeated(x):
    cols = [i for k in range(x.shape[1]) for i in ([k, k] if k % 4 == 3 else [k])]
    return np.ascontiguousarray(x[:, cols])


@pytest.mark.parametrize("edge", [255, 256, 257])
@pytest.mark.parametrize("name", KINDS)
def test_batch_plumbing_around_the_filter(hip_ctx, oracle_ctx, name, edge):
    """factor 5: paths that carry a status before the filter (identical points: first, in the middle, last) beside accepted ones, a
    path that close-point removal shortens (the filter must read rows of the new stride), one that it leaves with three points
    (stretched to four, decimated to one: refused), a path boundary at flat point index `edge` (blocks of 256 threads look their
    path up by offset), and the whole golden path, whose knots are those of a call of its own"""
    c, x = taught_points(name)
    p = with_windows(c.params, 5, 3)
    rows, thresh = driving_rows(p), p.jnt_thresh if p.path_type != capi.PATH_CART else p.cart_thresh
    n = x.shape[1]
    same = np.ascontiguousarray(np.repeat(x[:, :1], 16, axis=1))
    # accepted prefixes that fill the batch up to the edge: the path after them starts at flat point index `edge`
    fill, room = [], edge - 16
    while room:
        take = room if room <= min(n, 130) else min(n, 130) - 30
        fill.append(np.ascontiguousarray(x[:, :take]))
        room -= take
    assert all(f.shape[1] >= 21 for f in fill) and 16 + sum(f.shape[1] for f in fill) == edge
    repeated = _with_every_4th_repeated(x[:, :min(n, 120)])
    three = np.ascontiguousarray(np.repeat(x[:, 2:5], 4, axis=1))
    assert len(cr.remove_close_points(three.tolist(), rows, thresh)[0]) == 3
    assert len(cr.remove_close_points(repeated.tolist(), rows, thresh)[0]) == min(n, 120)
    xs = [same] + fill + [repeated, same, three, c.x, np.ascontiguousarray(x[:, 7:7 + 61]), same]
    whole = len(fill) + 4
    h, o = both(hip_ctx, oracle_ctx, p, xs, c.sres_in)
    st = [int(s) for s in o.status]
    refused = {0, len(fill) + 2, len(fill) + 3, len(xs) - 1}
    assert [k for k, s in enumerate(st) if s] == sorted(refused), (name, st)
    in_batch = h.knots(whole)                    # (the next call on the context takes the workspace the knots live in)
    alone, alone_o = both(hip_ctx, oracle_ctx, p, [c.x], c.sres_in)
    assert int(alone.status[0]) == 0
    assert_bit_equal(in_batch, alone.knots(0), f"{name}: the whole path inside the batch and alone")
    for r in (h, o, alone, alone_o):
        r.close()


# ---- c. close points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,sw", [(1, 1), (5, 3)])
@pytest.mark.parametrize("name", RESTATED_KINDS)
def test_close_points(hip_ctx, oracle_ctx, hip_traced, oracle_traced, name, d, sw):
    """runs of 2 .. 5 identical points inside, at the start and at the end (the tail rule), paths that end as three and as two
    points, a chain of three close points of which only the middle one goes although k_rs_close_any sees two close pairs, a step of
    exactly the threshold (kept) and of the double below it (dropped), and neighbours that differ in rows that do not drive -- the
    joint rows of a cable path, the Cartesian rows of a joint path -- which count as one point: as one batch, then each path alone
    and traced, against the checker and the restatement.  How many points each construction keeps is asserted on the restatement in
    tests/test_conditioning_cpu.py."""
    c, _ = taught_points(name)
    p = with_windows(c.params, d, sw, CLOSE_THRESH)
    paths = close_point_paths(name)
    xs = list(paths.values())
    h, o = both(hip_ctx, oracle_ctx, p, xs, c.sres_in)
    short = {k for k, label in enumerate(paths) if label.startswith("ends_as")}
    assert {k for k in range(len(xs)) if int(o.status[k])} == (short if d > 1 else set()), (name, d, o.status)
    for k, (label, x) in enumerate(paths.items()):
        st, hk = one_path_three_ways(hip_traced, oracle_traced, p, x, c.sres_in, f"{name} {label} d={d}")
        if not st:
            assert_bit_equal(h.knots(k), hk, f"{name} {label} d={d}: inside the batch and alone")
    h.close(); o.close()


@pytest.mark.parametrize("name", RESTATED_KINDS)
def test_only_one_path_of_a_batch_has_close_points(hip_ctx, oracle_ctx, name):
    """k_rs_remclose returns at once for the paths k_rs_close_any did not flag: with the flagged path first, in the middle and
    last, the others come out as in calls of their own"""
    c, x = taught_points(name)
    p = with_windows(c.params, 5, 3, CLOSE_THRESH)
    clean = [np.ascontiguousarray(x[:, a:a + m]) for a, m in ((0, 100), (30, 77), (60, 131), (11, 256), (5, 48))]
    flagged = close_point_paths(name)["run3_interior"]
    alone = []
    for xc in clean:
        h, o = both(hip_ctx, oracle_ctx, p, [xc], c.sres_in)
        assert int(h.status[0]) == 0
        alone.append(h.knots(0))
        h.close(); o.close()
    for at in (0, 2, len(clean)):
        xs = clean[:at] + [flagged] + clean[at:]
        h, o = both(hip_ctx, oracle_ctx, p, xs, c.sres_in)
        assert not o.status.any()
        for k, want in enumerate(alone):
            assert_bit_equal(h.knots(k if k < at else k + 1), want, f"{name}: unflagged path {k} beside a flagged one at {at}")
        h.close(); o.close()
