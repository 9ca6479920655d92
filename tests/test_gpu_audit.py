"""GPU (-m gpu): the audit of finished trajectories on the device (include/batotp_hip_audit.h) against tests/audit_reference.py on
the same rows.  Tolerance 0 everywhere: integers by ==, doubles bit for bit.

Known-answer shapes go through capi.output_from_rows, i.e. through the same launch function as the audit of a real output; real
trajectories are swept and passed through the output stage on the device first."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
from helpers import Case, OUTPUT_CASES, output_params, run_to_output
from audit_reference import audit_reference, assert_audit_equal
from batotp_amd import capi

pytestmark = pytest.mark.gpu

BP = capi.AUDIT_BLOCK_POINTS
NT, NC, NQ = 7, 3, 3
R = NT + NC + NQ
FAM_FLAGS = {capi.AUDIT_JNT_ACC: capi.F_JNT_ACC_ON, capi.AUDIT_CART_VEL: capi.F_CART_VEL_ON, capi.AUDIT_CART_ACC: capi.F_CART_ACC_ON,
             capi.AUDIT_TRQ: capi.F_TRQ_ON}
ALL_ON = capi.F_JNT_ACC_ON | capi.F_TRQ_ON | capi.F_CART_VEL_ON | capi.F_CART_ACC_ON | capi.F_PARALLEL
LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 66, 255, 256, 257, BP - 1, BP, BP + 1, BP + 2, 3 * BP + 5]
H = 0.008


def problem(flags=ALL_ON):
    """a cable-robot-like problem (torque rows = Cartesian rows) with seven joint rows and every family on"""
    return capi.make_problem(NT, NC, capi.ROBOT_CSPR3DOF, flags,
                             jnt_vel_max=[2.0, 1.5, 4.0, 1.0, 3.0, 2.5, 0.5], jnt_acc_max=[8.0, 16.0, 4.0, 2.0, 32.0, 1.0, 64.0],
                             jnt_trq_max=[10.0, 7.0, 3.0], jnt_trq_min=[-6.0, 1.0, -3.0], cart_vel_max=1.25, cart_acc_max=6.0)


def exact_problem(flags=ALL_ON):
    """every limit a power of two, torque range symmetric: with h = 0.5 and rows of small integers every difference, product and
    reciprocal of the definition is exact"""
    return capi.make_problem(NT, NC, capi.ROBOT_CSPR3DOF, flags, jnt_vel_max=[4.0] * NT, jnt_acc_max=[16.0] * NT,
                             jnt_trq_max=[4.0] * NQ, jnt_trq_min=[-4.0] * NQ, cart_vel_max=8.0, cart_acc_max=32.0)


def base_rows(seed=20240607, lengths=LENGTHS, scale=1e-4):
    """random rows far inside every limit (utilisations of a few per cent), so that whatever a test plants is the peak"""
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.standard_normal((R, n)) * scale) for n in lengths]


def peaks(a, fam):
    return [(float(x["fam"][fam]["peak"]), int(x["fam"][fam]["at"]), int(x["fam"][fam]["row"])) for x in a]


def device_audit(ctx, rows, sres, prob, tol=0.0, shape=(NT, NC, NQ)):
    out = capi.output_from_rows(ctx, rows, sres, *shape)
    assert [int(n) for n in out.n_pts] == [r.shape[1] for r in rows]
    got = out.audit(prob, tol)
    assert out.audit_ms() >= 0.0
    out.close()
    return got


def check(ctx, rows, sres, prob, tol=0.0, what="", shape=(NT, NC, NQ)):
    got = device_audit(ctx, rows, sres, prob, tol, shape)
    want = audit_reference(rows, sres, *shape, prob, tol)
    assert_audit_equal(got, want, what)
    return got


# ---- the known-answer batch ---------------------------------------------------------------------------------------------
def test_from_rows_is_a_genuine_output(hip_ctx):
    rows = base_rows()
    sres = [H * (1 + 0.1 * k) for k in range(len(rows))]
    out = capi.output_from_rows(hip_ctx, rows, sres, NT, NC, NQ)
    assert (out.n_theta, out.n_cart, out.n_trq, out.n_rows) == (NT, NC, NQ, R)
    assert [int(n) for n in out.n_pts] == LENGTHS and out.sres.tobytes() == np.asarray(sres).tobytes()
    for k, (a, b) in enumerate(zip(out.all_rows(), rows)):
        helpers.assert_bit_equal(a, b, f"download_all, path {k}")
        helpers.assert_bit_equal(out.rows(k), b, f"download, path {k}")
    with pytest.raises(capi.BatotpError):
        out.audit_ms()          # no audit yet
    out.close()


def test_random_rows_of_the_ragged_batch(hip_ctx):
    rows = base_rows(scale=0.01)     # utilisations around and above 1: n_over counts many points
    for tol in (0.0, 0.05, 3.0):
        got = check(hip_ctx, rows, H, problem(), tol, f"random rows, tol {tol}")
    assert [int(x) for x in got["n_pts"]] == LENGTHS
    assert int(check(hip_ctx, rows, H, problem(), 0.0)["n_over"].sum()) > 1000


def plant_difference(x, fam, i, big):
    """make point i the peak of a difference family of one path: velocity by raising x[i+1] and lowering x[i-1], acceleration by a
    spike at x[i]"""
    row = {capi.AUDIT_JNT_VEL: 3, capi.AUDIT_JNT_ACC: 5, capi.AUDIT_CART_VEL: NT + 1, capi.AUDIT_CART_ACC: NT + 2}[fam]
    if fam in (capi.AUDIT_JNT_VEL, capi.AUDIT_CART_VEL):
        x[row, i + 1] += big; x[row, i - 1] -= big
    else:
        x[row, i] += big
    return row if row < NT else 0


@pytest.mark.parametrize("fam", [capi.AUDIT_JNT_VEL, capi.AUDIT_JNT_ACC, capi.AUDIT_CART_VEL, capi.AUDIT_CART_ACC])
def test_planted_peaks_of_the_difference_families(hip_ctx, fam):
    """(a) at i = 1, at i = n - 2, at the last point of a block and at the first point of the next one (those need the halo)"""
    prob = problem()
    for where in ("first", "last", "block_end", "block_start", "second_block_end"):
        rows = base_rows()
        expect = {}
        for k, x in enumerate(rows):
            n = x.shape[1]
            i = {"first": 1, "last": n - 2, "block_end": BP - 1, "block_start": BP, "second_block_end": 2 * BP - 1}[where]
            if n >= 3 and 1 <= i <= n - 2:
                expect[k] = (i, plant_difference(x, fam, i, 0.05))
        assert expect
        got = check(hip_ctx, rows, H, prob, 0.0, f"{capi.AUDIT_FAMILIES[fam]} planted at {where}")
        for k, (i, row) in expect.items():
            assert peaks(got, fam)[k][1:] == (i, row), (where, k, peaks(got, fam)[k])
            assert int(got[k]["n_over"]) >= 1
        for k, x in enumerate(rows):
            if x.shape[1] < 3:
                assert peaks(got, fam)[k] == (-1.0, -1, -1)


def test_planted_torque_peaks_at_both_ends(hip_ctx):
    """(b) the torque family is evaluated at EVERY point: peaks at i = 0 and at i = n - 1, paths of one and two points included"""
    prob = problem()
    for end in (0, -1):
        rows = base_rows()
        for x in rows:
            if x.shape[1]:
                x[NT + NC + 1, end] = 7.0 + 4.0   # row 1: mid 4, half 3
        got = check(hip_ctx, rows, H, prob, 0.0, f"torque peak at end {end}")
        for k, x in enumerate(rows):
            n = x.shape[1]
            want = (-1.0, -1, -1) if n == 0 else (7.0 * (1.0 / 3.0), 0 if end == 0 else n - 1, 1)
            assert peaks(got, capi.AUDIT_TRQ)[k] == want, (end, k)


def exact_rows(lengths=(3 * BP + 5, 66, 2 * BP)):
    return [np.zeros((R, n)) for n in lengths]


TIE_SITES = [  # (point p, row a), (point q, row b) of two equal peaks, and the winner
    ((BP - 1, 4), (BP + 40, 2), (BP - 1, 4)),       # lowest point wins although its row is higher
    ((BP + 40, 2), (BP - 1, 4), (BP - 1, 4)),       # ... in either order of planting
    ((BP, 5), (BP, 1), (BP, 1)),                    # same point: lowest row
    ((BP, 1), (BP, 5), (BP, 1)),
    ((2 * BP - 1, 0), (2 * BP, 4), (2 * BP - 1, 0)),  # neighbours across a block edge
    ((30, 6), (10, 6), (10, 6)),
]


@pytest.mark.parametrize("fam", range(5))
def test_exact_ties_go_to_the_lowest_point_then_the_lowest_row(hip_ctx, fam):
    """(c) rows of small integers with h = 0.5: the tied utilisations are equal to the last bit, so only the tie rule decides"""
    prob = exact_problem()
    for (p, a), (q, b), (wp, wr) in TIE_SITES:
        rows = exact_rows()
        x = rows[0]
        cart = fam in (capi.AUDIT_CART_VEL, capi.AUDIT_CART_ACC)
        for (i, r) in ((p, a), (q, b)):
            if fam == capi.AUDIT_JNT_VEL:
                x[r, i + 1] += 2.0; x[r, i - 1] -= 2.0      # v = 4 at i, -2 at i - 2 and i + 2
            elif fam == capi.AUDIT_JNT_ACC:
                x[r, i] += 2.0                               # a = -16 at i, 8 beside it
            elif fam == capi.AUDIT_CART_VEL:
                x[NT + r % 3, i + 1] += 2.0; x[NT + r % 3, i - 1] -= 2.0
            elif fam == capi.AUDIT_CART_ACC:
                x[NT + r % 3, i] += 2.0
            else:
                x[NT + NC + r % 3, i] = 3.0 if r % 2 else -3.0
        got = check(hip_ctx, rows, 0.5, prob, 0.0, f"ties, family {capi.AUDIT_FAMILIES[fam]}, sites {(p, a), (q, b)}")
        pk = peaks(got, fam)[0]
        if cart:
            assert pk[1:] == (wp, 0), pk
        elif fam == capi.AUDIT_TRQ:
            assert pk == (0.75, wp, min(a % 3, b % 3) if p == q else wr % 3), pk
        else:
            assert pk == (1.0, wp, wr), pk
        assert int(got[0]["n_over"]) == 0      # u == 1.0 exactly is within the limit
        assert peaks(got, fam)[1] == (0.0, 1 if fam != capi.AUDIT_TRQ else 0, 0)   # an all-zero path: every point ties at 0


def test_nonfinite_values_are_counted_and_drop_out(hip_ctx):
    """(d) NaN and +-Inf at isolated points, block edges included: n_nonfinite counts them, the utilisations they reach drop out of the
    peaks and of n_over, and nothing else does"""
    prob = problem()
    rows = base_rows(scale=0.004)
    planted = 0
    for k, x in enumerate(rows):
        n = x.shape[1]
        sites = [(0, 0, np.nan), (1, NT, np.inf), (n - 1, R - 1, -np.inf), (n // 2, 3, np.nan), (BP - 1, 2, np.nan), (BP, NT + 2, -np.inf),
                 (BP + 1, NT + NC, np.inf), (2 * BP, 6, np.inf), (2 * BP - 1, NT + NC + 2, np.nan)]
        seen = set()
        for i, r, bad in sites:
            if 0 <= i < n and (i, r) not in seen:
                seen.add((i, r)); x[r, i] = bad; planted += 1
    for tol in (0.0, 0.05):
        got = check(hip_ctx, rows, H, prob, tol, "non-finite values")
    assert int(got["n_nonfinite"].sum()) == planted
    # a planted peak next to a NaN of the same row is gone, the peak of another row stays
    rows = base_rows()
    x = rows[-1]
    plant_difference(x, capi.AUDIT_JNT_VEL, BP, 0.05)       # row 3
    x[1, 200] += 0.04; x[1, 198] -= 0.04                     # row 1, point 199: the runner-up
    assert peaks(check(hip_ctx, rows, H, prob), capi.AUDIT_JNT_VEL)[-1][1:] == (BP, 3)
    x[3, BP + 1] = np.nan
    got = check(hip_ctx, rows, H, prob, 0.0, "NaN beside the peak")
    assert peaks(got, capi.AUDIT_JNT_VEL)[-1][1:] == (199, 1) and int(got[-1]["n_nonfinite"]) == 1
    # a path of nothing but NaN: every family -1, every value counted, nothing over
    nan_rows = [np.full((R, 300), np.nan)]
    got = check(hip_ctx, nan_rows, H, prob, 0.0, "all NaN")
    assert all(peaks(got, f)[0] == (-1.0, -1, -1) for f in range(5)) and int(got[0]["n_nonfinite"]) == R * 300 and int(got[0]["n_over"]) == 0


def test_the_bound_is_strict(hip_ctx):
    """(e) u == 1.0 + tol exactly is within the limit, one ulp above is over"""
    only_vel_trq = exact_problem(capi.F_PARALLEL | capi.F_TRQ_ON)
    for tol, at_bound in ((0.0, 4.0), (0.25, 5.0), (0.5, 6.0)):
        rows = exact_rows((40, BP + 7))
        up = float(np.nextafter(at_bound, np.inf))
        for x in rows:
            n = x.shape[1]
            x[NT + NC, 3] = at_bound         # torque: u = at_bound / 4 = 1 + tol
            x[NT + NC + 2, n - 1] = -at_bound
            x[NT + NC + 1, 7] = up           # one ulp above
            x[2, 21] = at_bound              # joint velocity at points 20 and 22: |x[21] - 0| * 1 / 4 = 1 + tol
        check(hip_ctx, rows, 0.5, exact_problem(), tol, f"strict bound, tol {tol}, every family")
        got = check(hip_ctx, rows, 0.5, only_vel_trq, tol, f"strict bound, tol {tol}")
        for k in range(2):
            assert int(got[k]["n_over"]) == 1, (tol, k, int(got[k]["n_over"]))       # point 7 alone
            assert peaks(got, capi.AUDIT_TRQ)[k] == (up * 0.25, 7, 1)
            assert peaks(got, capi.AUDIT_JNT_VEL)[k] == (1.0 + tol, 20, 2)
        rows[1][2, 21] = up                  # ... and an ulp above: points 20 and 22 count too
        check(hip_ctx, rows, 0.5, exact_problem(), tol, f"strict bound, tol {tol}, every family, an ulp above")
        got = check(hip_ctx, rows, 0.5, only_vel_trq, tol, f"strict bound, tol {tol}, joint velocity an ulp above")
        assert [int(x) for x in got["n_over"]] == [1, 3]
        assert peaks(got, capi.AUDIT_JNT_VEL)[1] == (up * 0.25, 20, 2)


def test_each_flag_off_in_turn(hip_ctx):
    """(f) the family of a cleared flag is -1, the other families are unchanged"""
    rows = base_rows(scale=0.003)
    full = check(hip_ctx, rows, H, problem(), 0.0, "all on")
    for fam, flag in FAM_FLAGS.items():
        got = check(hip_ctx, rows, H, problem(ALL_ON & ~flag), 0.0, f"{capi.AUDIT_FAMILIES[fam]} off")
        for f in range(5):
            if f == fam:
                assert all(p == (-1.0, -1, -1) for p in peaks(got, f))
            else:
                assert got["fam"][:, f].tobytes() == full["fam"][:, f].tobytes()
        assert got["n_nonfinite"].tobytes() == full["n_nonfinite"].tobytes()
    got = check(hip_ctx, rows, H, problem(capi.F_PARALLEL), 0.0, "joint velocity only")
    assert got["fam"][:, 0].tobytes() == full["fam"][:, 0].tobytes()
    # outputs without Cartesian / torque rows: the flags of the problem alone do not audit a family
    jrows = [np.ascontiguousarray(x[:NT]) for x in rows]
    got = check(hip_ctx, jrows, H, problem(), 0.0, "joint rows only", shape=(NT, 0, 0))
    assert got["fam"][:, :2].tobytes() == full["fam"][:, :2].tobytes()
    assert all(peaks(got, f)[k] == (-1.0, -1, -1) for f in (2, 3, 4) for k in range(len(rows)))
    # one and two position rows: the terms of the rows that do not exist are left out
    for nc in (1, 2):
        p = problem(); p.n_cart = nc
        p.flags &= ~capi.F_TRQ_ON
        crows = [np.ascontiguousarray(x[:NT + nc]) for x in rows]
        check(hip_ctx, crows, H, p, 0.0, f"{nc} Cartesian rows", shape=(NT, nc, 0))


# ---- grids ----------------------------------------------------------------------------------------------------------------
def test_many_short_paths_and_empty_paths(hip_ctx):
    prob = problem()
    rng = np.random.default_rng(5)
    rows = [np.ascontiguousarray(rng.standard_normal((R, 5)) * 0.004) for _ in range(130)]
    got = check(hip_ctx, rows, [H * (1 + k % 7) for k in range(130)], prob, 0.05, "130 paths of 5 points")
    assert len(set(peaks(got, 0))) > 100
    lengths = [0] * 73
    for k in (0, 41, 72):
        lengths[k] = 300
    rows = [np.ascontiguousarray(rng.standard_normal((R, n)) * 0.004) for n in lengths]
    got = check(hip_ctx, rows, H, prob, 0.0, "70 empty paths and 3 of 300 points")
    assert [int(n) for n in got["n_pts"]] == lengths
    assert all(peaks(got, f)[1] == (-1.0, -1, -1) for f in range(5)) and int(got[1]["n_over"]) == 0
    got = check(hip_ctx, [np.zeros((R, 0))] * 3, H, prob, 0.0, "nothing but empty paths")
    assert int(got["n_pts"].sum()) == 0


def test_more_blocks_than_the_lanes_of_the_finishing_wavefront(hip_ctx):
    """a path of more than 64 blocks (the finishing kernel strides over its partials), its peaks in the last block and in block 64"""
    prob = problem()
    n = 70 * BP + 3
    rows = base_rows(seed=9, lengths=[n, 5, 66 * BP])
    plant_difference(rows[0], capi.AUDIT_JNT_ACC, n - 2, 0.05)
    plant_difference(rows[0], capi.AUDIT_CART_VEL, 64 * BP, 0.05)
    rows[0][NT + NC, 65 * BP - 1] = 50.0
    got = check(hip_ctx, rows, H, prob, 0.0, "70 blocks")
    assert peaks(got, capi.AUDIT_JNT_ACC)[0][1:] == (n - 2, 5) and peaks(got, capi.AUDIT_CART_VEL)[0][1:] == (64 * BP, 0)
    assert peaks(got, capi.AUDIT_TRQ)[0][1:] == (65 * BP - 1, 0)


def test_same_bits_whatever_the_cut(hip_ctx):
    """the audit of the ragged batch = the audit of each of its paths alone in an output of its own"""
    prob = problem()
    rows = base_rows(scale=0.004)
    sres = [H * (1 + 0.25 * (k % 3)) for k in range(len(rows))]
    whole = check(hip_ctx, rows, sres, prob, 0.05, "ragged batch")
    for k, x in enumerate(rows):
        alone = device_audit(hip_ctx, [x], [sres[k]], prob, 0.05)
        assert alone[0].tobytes() == whole[k].tobytes(), k


def test_audit_device_leaves_the_rows_on_the_device(hip_ctx):
    """batotp_hip_output_audit_device writes the rows into device memory of the caller -- exactly n_paths of them (guard bytes on both
    sides).  The memory comes from the HIP runtime the library is bound to (hipMalloc through ctypes), as in tests/test_gpu_gather.py."""
    hip = C.CDLL("libamdhip64.so.7", mode=os.RTLD_NOLOAD | os.RTLD_NOW)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    prob = problem()
    rows = base_rows(scale=0.004)
    out = capi.output_from_rows(hip_ctx, rows, H, NT, NC, NQ)
    guard, size = 256, len(rows) * C.sizeof(capi.PathAudit)
    host = np.full(size + 2 * guard, 0xA5, dtype=np.uint8)
    base = C.c_void_p()
    assert hip.hipMalloc(C.byref(base), host.nbytes) == 0
    assert hip.hipMemcpy(base, host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0
    hip_ctx.library.check(hip_ctx.library.lib.batotp_hip_output_audit_device(out.handle, C.byref(prob), 0.05, C.c_void_p(base.value + guard)), "audit_device")
    assert out.audit_ms() >= 0.0
    assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), base, host.nbytes, 2) == 0
    assert hip.hipFree(base) == 0
    assert (host[:guard] == 0xA5).all() and (host[guard + size:] == 0xA5).all()
    assert host[guard:guard + size].tobytes() == out.audit(prob, 0.05).tobytes()
    out.close()


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_touch_nothing(hip_ctx):
    lib = hip_ctx.library.lib
    rows = base_rows(lengths=[40, 0, 7])
    out = capi.output_from_rows(hip_ctx, rows, H, NT, NC, NQ)
    good = out.audit(problem(), 0.0)
    buf = np.full(3, 0x5A, dtype=np.uint8).repeat(C.sizeof(capi.PathAudit))
    sentinel = buf.copy()

    def audit_rc(prob, tol, handle=out.handle, dst=buf):
        return lib.batotp_hip_output_audit(handle, C.byref(prob) if prob is not None else None, tol, dst.ctypes.data_as(C.c_void_p) if dst is not None else None)

    bad = []
    for tol in (-1e-300, -1.0, float("nan"), float("inf"), float("-inf")):
        bad.append(("tol", audit_rc(problem(), tol)))
    bad.append(("NULL output", audit_rc(problem(), 0.0, handle=None)))
    bad.append(("NULL problem", audit_rc(None, 0.0)))
    bad.append(("NULL rows", audit_rc(problem(), 0.0, dst=None)))
    bad.append(("NULL device rows", lib.batotp_hip_output_audit_device(out.handle, C.byref(problem()), 0.0, None)))
    p = problem(); p.n_joints = NT - 1
    bad.append(("n_joints", audit_rc(p, 0.0)))
    p = problem(); p.n_cart = 2          # a parallel mechanism's torque rows are its Cartesian rows: 2 < 3
    bad.append(("torque rows", audit_rc(p, 0.0)))
    for field, j, v in (("jnt_vel_max", 6, 0.0), ("jnt_vel_max", 0, float("nan")), ("jnt_acc_max", 2, float("inf")), ("jnt_acc_max", 3, -1.0),
                        ("jnt_trq_max", 1, 1.0), ("jnt_trq_min", 2, float("-inf"))):
        p = problem(); getattr(p, field)[j] = v
        bad.append((f"{field}[{j}] = {v}", audit_rc(p, 0.0)))
    for field, v in (("cart_vel_max", 0.0), ("cart_acc_max", float("nan"))):
        p = problem(); setattr(p, field, v)
        bad.append((f"{field} = {v}", audit_rc(p, 0.0)))
    for what, rc in bad:
        assert rc == -1, (what, rc)                        # BATOTP_ERR_ARG
    assert buf.tobytes() == sentinel.tobytes()
    # a limit of a family that is not audited is not looked at
    p = problem(ALL_ON & ~capi.F_JNT_ACC_ON); p.jnt_acc_max[0] = 0.0
    assert audit_rc(p, 0.0) == 0
    # ... and a good call still works
    assert out.audit(problem(), 0.0).tobytes() == good.tobytes()
    assert_audit_equal(good, audit_reference(rows, H, NT, NC, NQ, problem(), 0.0), "after the refusals")

    # batotp_hip_output_from_rows
    n_pts = np.array([4, 0, 3], dtype=np.int64); sres = np.array([H, -1.0, H]); flat = np.zeros(7 * R)
    handle = C.c_void_p(0x1234)

    def from_rows_rc(ctx=hip_ctx.handle, k=3, n=n_pts, s=sres, shape=(NT, NC, NQ), x=flat, dst=handle):
        return lib.batotp_hip_output_from_rows(ctx, k, n.ctypes.data_as(C.POINTER(C.c_int64)) if n is not None else None,
                                               capi._dptr(s) if s is not None else None, *shape, capi._dptr(x) if x is not None else None,
                                               C.byref(dst) if dst is not None else None)

    assert from_rows_rc(ctx=None) == -1 and from_rows_rc(k=-1) == -1 and from_rows_rc(n=None) == -1 and from_rows_rc(s=None) == -1
    assert from_rows_rc(x=None) == -1 and from_rows_rc(dst=None) == -1 and from_rows_rc(shape=(NT, -1, NQ)) == -1 and from_rows_rc(shape=(0, 0, 0)) == -1
    assert from_rows_rc(shape=(9, 0, 0)) == -1 and from_rows_rc(n=np.array([4, -1, 3], dtype=np.int64)) == -1
    for v in (0.0, -H, float("nan"), float("inf")):
        assert from_rows_rc(s=np.array([H, H, v])) == -1, v
    assert handle.value == 0x1234                          # nothing touched
    assert from_rows_rc() == 0 and handle.value not in (None, 0x1234)   # the bad step belongs to the path without points
    assert lib.batotp_hip_output_destroy(handle) == 0
    out.close()


# ---- real trajectories ------------------------------------------------------------------------------------------------------
def check_real(out, prob, what):
    rows = out.all_rows()
    for tol in (0.0, 0.05):
        got = out.audit(prob, tol)
        want = audit_reference(rows, out.sres, out.n_theta, out.n_cart, out.n_trq, prob, tol)
        assert_audit_equal(got, want, f"{what}, tol {tol}")
    for k in range(out.n_paths):
        print(f"AUDIT {what} path {k}: n_pts {int(got[k]['n_pts'])} n_over(tol 0.05) {int(got[k]['n_over'])} n_nonfinite {int(got[k]['n_nonfinite'])} " +
              " ".join(f"{name} {float(got[k]['fam'][f]['peak']):.4f}@{int(got[k]['fam'][f]['at'])}/{int(got[k]['fam'][f]['row'])}"
                       for f, name in enumerate(capi.AUDIT_FAMILIES)))
    assert int(got["n_nonfinite"].sum()) == 0, what
    return got


@pytest.mark.parametrize("name", OUTPUT_CASES)
def test_golden_cases(hip_ctx, name):
    """GEN7DOF, UR5 / UR5_pos3 (pose rows), KUKA with Cartesian limits, RR with torque limits, the cable robot with tensions: swept, passed
    through the output stage and audited with their own problem.  No bound on the peaks: finite differences of a smoothed trajectory may
    exceed 1 (DESIGN.md 4 records what was measured)."""
    case = Case(name)
    out, b = run_to_output(hip_ctx, [case])
    got = check_real(out, case.problem, name)
    assert int(got[0]["n_pts"]) == int(out.n_pts[0]) > 4 and float(got[0]["fam"][0]["peak"]) > 0.0
    out.close(); b.close()


def variants(base):
    """output parameters reaching the branches of the stage: plain, smoothing, re-interpolation, both, a coarse output"""
    return [capi.OutputParams(base.n_joints, base.path_type, base.integ_res, out_res, smooth)
            for out_res, smooth in ((base.integ_res, 1.0), (base.integ_res, 5.0), (base.integ_res * 0.8, 1.0), (base.integ_res * 0.8, 5.0),
                                    (base.integ_res * 2.5, 4.0))]


@pytest.mark.parametrize("name", ["synth_cspr_s3", "CSPR3DOF_par", "KUKA-LWR-IV", "RR", "RR_acc", "KUKA_trq"])
def test_robot_branches_of_the_output_stage(hip_ctx, name):
    """cable tensions, forward kinematics, serial torques: two paths of different length through every branch of the stage"""
    case = Case(name)
    short = np.ascontiguousarray(case.y[:, :max(40, case.n // 3)])
    base = output_params(name) if name in OUTPUT_CASES else capi.OutputParams(case.problem.n_joints, capi.PATH_JOINT, case.problem.integ_res, 0.008, 5.0)
    b = capi.Batch(hip_ctx, case.problem, [case.n, short.shape[1]], case.max_steps())
    b.upload_knots(0, [case.y], [case.sres]); b.upload_knots(1, [short], [case.sres])
    helpers.precompute_with_trig(hip_ctx, b, case.problem, 2)
    b.sweep(-1); b.sweep(+1)
    for prm in variants(base):
        out = capi.Output(b, prm, 0, 2)
        check_real(out, case.problem, f"{name} out_res={prm.out_res} smooth={prm.out_smooth_fact}")
        out.close()
    b.close()


def test_ragged_batch_sub_range_and_a_failed_path(hip_ctx):
    cases = [Case("synth_gen7dof_s0"), Case("synth_gen7dof_s0"), Case("synth_gen7dof_s0")]
    cases[1].y = np.ascontiguousarray(cases[1].y[:, :400])
    base = output_params("synth_gen7dof_s0")
    b = capi.Batch(hip_ctx, cases[0].problem, [c.n for c in cases], max(c.max_steps() for c in cases))
    for k, c in enumerate(cases):
        b.upload_knots(k, [c.y], [c.sres])
    b.optimize()
    for prm in variants(base):
        full = capi.Output(b, prm, 0, 3)
        sub = capi.Output(b, prm, 1, 2)             # a range with path0 > 0
        a = check_real(full, cases[0].problem, f"ragged out_res={prm.out_res} smooth={prm.out_smooth_fact}")
        s = check_real(sub, cases[0].problem, "sub-range")
        assert s.tobytes() == a[1:].tobytes()
        full.close(); sub.close()
    b.close()
    small = cases[0]
    b = capi.Batch(hip_ctx, small.problem, [small.n], 64)   # capacity far too small: the sweep fails, the output has no points
    b.upload_knots(0, [small.y], [small.sres])
    b.optimize()
    out = capi.Output(b, base, 0, 1)
    got = out.audit(small.problem, 0.0)
    assert int(out.n_pts[0]) == 0 and int(got[0]["n_pts"]) == 0 and int(got[0]["n_over"]) == 0 and int(got[0]["n_nonfinite"]) == 0
    assert all(peaks(got, f)[0] == (-1.0, -1, -1) for f in range(5))
    out.close(); b.close()


def test_per_path_steps(hip_ctx):
    """one call in per-path-step mode: plain and re-interpolated paths in one output, each audited with the sres the stage reports for
    it (the stage derives it per path; the known-answer batches above are where it really differs from path to path)"""
    case = Case("synth_gen7dof_s0")
    h = case.problem.integ_res
    ys = [case.y, case.y[:, :400], case.y, case.y[:, :150], case.y[:, :400]]
    steps = [h * f for f in (1.0, 0.5, 1.25, 2.0, 0.8)]
    b = capi.Batch(hip_ctx, case.problem, [y.shape[1] for y in ys], 3 * case.max_steps())
    for k, y in enumerate(ys):
        b.upload_knots(k, [np.ascontiguousarray(y)], [case.sres])
    b.set_path_integ_res(0, steps)
    b.precompute(1); b.sweep(-1); b.sweep(+1)
    base = output_params(case.name)
    for out_res, smooth in ((1.1 * h, 1.0), (1.1 * h, 5.0), (0.3 * h, 5.0)):
        out = capi.Output(b, capi.OutputParams(base.n_joints, base.path_type, 12345.0, out_res, smooth), 0, 5, per_path_steps=True)
        check_real(out, case.problem, f"per-path steps out_res={out_res} smooth={smooth}")
        out.close()
    b.close()


def test_baseline_size_path(hip_ctx):
    """a 1e5-knot path: tens of thousands of output points, 26 blocks of one path"""
    case = Case("synth_ur_s7_100k")
    prm = capi.OutputParams(case.problem.n_joints, capi.PATH_JOINT, case.problem.integ_res, 0.008, 5.0)
    b = capi.Batch(hip_ctx, case.problem, [case.n], case.max_steps())
    b.upload_knots(0, [case.y], [case.sres])
    b.optimize()
    out = capi.Output(b, prm, 0, 1)
    assert int(out.n_pts[0]) > 20 * BP
    check_real(out, case.problem, "synth_ur_s7_100k")
    out.close(); b.close()


# ---- host route --------------------------------------------------------------------------------------------------------------
HOST = os.path.join(helpers.ROOT, "batotp_amd", "host")


def stage_case(name, work):
    import shutil
    src = os.path.join(helpers.GOLD, name)
    for f in os.listdir(src):
        if not f.startswith("ref_") and not f.endswith(".npz") and not f.endswith(".json"):
            shutil.copy(os.path.join(src, f), work / f)


def test_batch_driver_prints_the_audit(tmp_path):
    """batest_batch <a GENJNT configuration> 4 --audit: exit status 0 and the summary line"""
    exe = os.path.join(HOST, "_build", "batest_batch")
    assert os.path.exists(exe), "build() must produce batest_batch"
    stage_case("synth_gen7dof_s0", tmp_path)
    r = subprocess.run([exe, "config.dat", "4", "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("audit (tol 0):")]
    assert len(line) == 1, r.stdout[-2000:]
    assert " jnt_vel 0." in line[0] or " jnt_vel 1." in line[0]
    assert " jnt_acc " in line[0] and " cart_vel -" in line[0] and " cart_acc -" in line[0] and " trq -" in line[0] and "; over:" in line[0]
    assert "(path 0, t " in line[0]          # four copies of one path: the first of the equal peaks is named
    r2 = subprocess.run([exe, "config.dat", "4", "--audit", "0.25"], cwd=tmp_path, capture_output=True, text=True)
    assert r2.returncode == 0 and "audit (tol 0.25):" in r2.stdout
    r3 = subprocess.run([exe, "config.dat", "2"], cwd=tmp_path, capture_output=True, text=True)
    assert r3.returncode == 0 and "audit" not in r3.stdout


@pytest.mark.parametrize("name, devices", [("synth_gen7dof_s0", False), ("CSPR3DOF", False), ("KUKA_cartacc", False), ("synth_gen7dof_s0", True)])
def test_host_library_audit_equals_the_c_abi(hip_ctx, tmp_path, name, devices):
    """BA::getLastAudit() after BA::optimizeBatch = the C-ABI's audit of the same paths swept and passed through the output stage here
    (tests/drivers/batch_audit_main.cpp); with --all-devices the ranges of the workers, one per GPU of the machine, are put back in path
    order (one GPU: one range)"""
    exe = tmp_path / "batch_audit"
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", f"-I{HOST}", f"-I{helpers.ROOT}/include", os.path.join(helpers.ROOT, "tests", "drivers", "batch_audit_main.cpp"),
           os.path.join(HOST, "_build", "libbatotp.a"), f"-L{helpers.ROOT}/batotp_amd/csrc", "-lbatotp_hip", f"-Wl,-rpath,{helpers.ROOT}/batotp_amd/csrc",
           "-pthread", "-lm", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    stage_case(name, tmp_path)
    n, tol = 3, 0.05
    args = [str(exe), "config.dat", str(n), str(tol)] + (["--all-devices"] if devices else [])
    r = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    case = Case(name)
    out, b = run_to_output(hip_ctx, [case] * n)
    want = out.audit(case.problem, tol)
    got = np.zeros(n, dtype=capi.AUDIT_DTYPE)
    seen = 0
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w and w[0] == "path":
            p = int(w[1])
            assert int(w[3]) == 1
            got[p]["n_pts"], got[p]["n_over"], got[p]["n_nonfinite"] = int(w[5]), int(w[7]), int(w[9])
            assert np.array([int(w[11], 16)], dtype=np.uint64).view(np.float64)[0] == out.sres[p]
        if w and w[0] == "peak":
            p, f = int(w[1]), int(w[2])
            got[p]["fam"][f]["peak"] = np.array([int(w[3], 16)], dtype=np.uint64).view(np.float64)[0]
            got[p]["fam"][f]["at"], got[p]["fam"][f]["row"] = int(w[4]), int(w[5])
            seen += 1
    assert seen == 5 * n
    assert_audit_equal(got, want, f"BA::getLastAudit, {name}")
    out.close(); b.close()
