"""GPU (-m gpu): finished trajectories stretched in time (include/batotp_hip_stretch.h) against tests/stretch_reference.py on the same
rows.  The tolerance is 0: rows are compared as uint64 (a NaN for a NaN).  Known-answer shapes enter through capi.output_from_rows;
real trajectories are swept and passed through the output stage on the device first."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import invdyn_reference as ir
import stretch_reference as sr
from audit_reference import assert_audit_equal
from batotp_amd import capi

pytestmark = pytest.mark.gpu

BP = capi.STRETCH_BLOCK_POINTS
# empty paths between full ones; every length around the block of new points
LENGTHS = [4, 0, 1, 2, 3, 5, BP - 1, 0, BP, BP + 1, 0, 2 * BP + 1]
SHAPES = [(7, 0), (6, 6), (3, 3), (1, 0)]
H = 0.008
ERR_ARG = -1      # BATOTP_ERR_ARG
HOST = os.path.join(helpers.ROOT, "batotp_amd", "host")


def n_out_of(mode, n):
    if n < 2:
        return n
    return {"same": n, "plus1": n + 1, "2n-1": 2 * n - 1, "7.3": sr.n_out_by(n, 7.3), "64n": 64 * n}[mode]


MODES = ["same", "plus1", "2n-1", "7.3", "64n"]


def batch_rows(shape, lengths=LENGTHS, seed=3):
    nT, nC = shape
    rng = np.random.default_rng(seed + 10 * nT + nC)
    # smooth rows with noise on top: every term of the cubic in play, values of both signs and of different magnitudes per row
    out = []
    for n in lengths:
        t = np.arange(n) * H
        base = np.sin(np.outer(np.arange(1, nT + nC + 1), t) * 3.0) * rng.uniform(0.1, 50.0, (nT + nC, 1))
        out.append(np.ascontiguousarray(base + rng.standard_normal((nT + nC, n)) * 0.01))
    return out


def steps(rows):
    return np.array([H * (1 + 0.1 * k) for k in range(len(rows))])


_ROWS, _WANT = {}, {}


def known_rows(shape):
    if shape not in _ROWS:
        rows = batch_rows(shape)
        for a in rows:
            a.setflags(write=False)
        _ROWS[shape] = rows
    return _ROWS[shape]


def known_answers(shape, mode):
    """(rows, n_out, expected rows) of the ragged batch -- computed once, shared, never modified"""
    key = (shape, mode)
    if key not in _WANT:
        rows = known_rows(shape)
        n_out = [n_out_of(mode, r.shape[1]) for r in rows]
        want = sr.stretch_to(rows, n_out)
        for a in want:
            a.setflags(write=False)
        _WANT[key] = (rows, n_out, want)
    return _WANT[key]


def check_output(new, want, what):
    got = new.all_rows()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        sr.assert_rows_equal(g, w, f"{what}, path {k} (download_all)")
    for k in (0, len(want) - 1):
        sr.assert_rows_equal(new.rows(k), want[k], f"{what}, path {k} (download)")


# ---- 1. known answers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_known_answers(hip_ctx, shape, mode):
    rows, n_out, want = known_answers(shape, mode)
    nT, nC = shape
    sres = steps(rows)
    out = capi.output_from_rows(hip_ctx, rows, sres, nT, nC, 0)
    new = out.stretch_to(n_out)
    assert (new.n_theta, new.n_cart, new.n_trq, new.n_rows) == (nT, nC, 0, nT + nC)
    assert [int(n) for n in new.n_pts] == n_out and new.sres.tobytes() == sres.tobytes()
    check_output(new, want, f"{shape}, {mode}")
    assert new.stretch_ms() >= 0.0 and new.stretch_ranges() == 1
    if mode == "same":
        for k, (g, r) in enumerate(zip(new.all_rows(), rows)):
            assert g.tobytes() == r.tobytes(), f"path {k} is a copy"
    # the input is untouched, and it is not a result of the call
    for k, (g, r) in enumerate(zip(out.all_rows(), rows)):
        assert g.tobytes() == r.tobytes(), k
    with pytest.raises(capi.BatotpError):
        out.stretch_ms()
    ptr, cnt = C.c_void_p(), C.c_int64(0)
    new.L.check(new.lib.batotp_hip_output_device(new.handle, C.byref(ptr), C.byref(cnt)), "output_device")
    assert ptr.value and cnt.value == sum(n_out) * (nT + nC)
    new.close(); out.close()


def test_paths_of_one_batch_with_targets_of_their_own(hip_ctx):
    """every mode in one call, path by path"""
    shape = (3, 3)
    rows = known_rows(shape)
    n_out = [n_out_of(MODES[k % len(MODES)], r.shape[1]) for k, r in enumerate(rows)]
    out = capi.output_from_rows(hip_ctx, rows, H, 3, 3, 0)
    new = out.stretch_to(n_out)
    check_output(new, sr.stretch_to(rows, n_out), "mixed targets")
    new.close(); out.close()


# ---- 2. stretch_by ---------------------------------------------------------------------------------------------------------
def test_stretch_by_is_stretch_to_of_the_stated_count(hip_ctx):
    shape = (7, 0)
    rows, n_out, want = known_answers(shape, "7.3")
    out = capi.output_from_rows(hip_ctx, rows, H, 7, 0, 0)
    new = out.stretch_by(7.3)
    assert [int(n) for n in new.n_pts] == n_out
    check_output(new, want, "stretch_by 7.3")
    new.close()
    factors = np.array([1.0, 1.05, 2.0, 1.0 + 2.0 ** -40, 3.999, 16.0, 1.5, 1.0, 2.0, 1.25, 9.0, 1.0 + 1e-9])
    n2 = [sr.n_out_by(r.shape[1], f) for r, f in zip(rows, factors)]
    assert n2[2] == 1 and n2[8] == 2 * BP - 1 and n2[11] == 2 * BP + 2
    new = out.stretch_by(factors)
    assert [int(n) for n in new.n_pts] == n2
    check_output(new, sr.stretch_to(rows, n2), "stretch_by, a factor per path")
    new.close(); out.close()


# ---- 3. values that are not finite -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plus1", "2n-1", "7.3"])
def test_values_that_are_not_finite_propagate_as_in_the_reference(hip_ctx, mode):
    shape = (3, 3)
    rows = [r.copy() for r in known_rows(shape)]
    for k, r in enumerate(rows):
        n = r.shape[1]
        if n >= 4:
            r[0, 0], r[5, n - 1] = np.nan, np.inf               # the ends
            r[1, 1], r[2, n - 2] = -np.inf, np.nan              # the cells next to them
        if n >= BP - 1:
            r[3, n // 2], r[4, n // 3], r[4, n // 3 + 1] = np.nan, np.inf, -np.inf
    n_out = [n_out_of(mode, r.shape[1]) for r in rows]
    want = sr.stretch_to(rows, n_out)
    assert any(np.isnan(w).any() and np.isinf(w).any() for w in want)
    out = capi.output_from_rows(hip_ctx, rows, H, 3, 3, 0)
    new = out.stretch_to(n_out)
    check_output(new, want, f"non-finite, {mode}")
    prob = capi.make_problem(3, 3, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0] * 3)
    got = new.audit(prob, 0.0)
    assert [int(v) for v in got["n_nonfinite"]] == [int(np.count_nonzero(~np.isfinite(w))) for w in want]
    new.close(); out.close()


# ---- 4. the same bits however it is cut ------------------------------------------------------------------------------------
def test_same_bits_under_a_workspace_budget(hip_lib):
    shape = (6, 6)
    rows, n_out, want = known_answers(shape, "7.3")
    ctx = capi.Context(hip_lib, 0)          # a context of its own: the budget is a property of the context
    out = capi.output_from_rows(ctx, rows, H, 6, 6, 0)
    whole = out.stretch_to(n_out)
    assert whole.stretch_ranges() == 1
    flat = [r.copy() for r in whole.all_rows()]
    ctx.set_workspace_budget(0, 40 + 8 * 9)   # the descriptors of a path of nine blocks: the small paths share ranges, the long ones do not
    cut = out.stretch_to(n_out)
    assert 3 <= cut.stretch_ranges() < len(rows), cut.stretch_ranges()
    ctx.set_workspace_budget(0, 1)            # every path a range of its own; a range of empty paths launches nothing
    each = out.stretch_to(n_out)
    assert each.stretch_ranges() == sum(1 for n in n_out if n > 0)
    for o, what in ((cut, "under a budget"), (each, "a range per path")):
        for k, (g, w) in enumerate(zip(o.all_rows(), flat)):
            assert g.tobytes() == w.tobytes(), (what, k)
        check_output(o, want, what)
    ctx.set_workspace_budget(0, 0)
    for o in (whole, cut, each, out):
        o.close()


# ---- 5. audit mode ---------------------------------------------------------------------------------------------------------
def audit_batch():
    """a ragged batch whose paths need factors of their own: quiet paths, paths over their velocity or acceleration limits, a path
    with a jump in velocity (one round is not enough for it), paths too short to audit, an empty one"""
    rng = np.random.default_rng(41)
    rows = []
    for k, n in enumerate([BP + 1, 0, 2, 3 * BP + 5, 1, 700, 90, 2 * BP, 333]):
        t = np.arange(n) * H
        amp = [0.05, 0, 1.0, 0.9, 0, 2.5, 0.3, 4.0, 0.2][k]
        r = amp * np.sin(np.outer([1.0, 1.3, 0.7, 2.0, 0.5, 0.9], t) * 2.0 + rng.uniform(0, 3, (6, 1))) if n else np.zeros((6, 0))
        if k == 6:      # a kink: the joint stands, then moves at constant velocity
            r[0] = np.where(np.arange(n) < 45, 0.0, (np.arange(n) - 45) * H * 0.8)
        rows.append(np.ascontiguousarray(r))
    prob = capi.make_problem(3, 3, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON | capi.F_CART_VEL_ON | capi.F_CART_ACC_ON,
                             jnt_vel_max=[1.0, 1.5, 2.0], jnt_acc_max=[4.0, 3.0, 5.0], cart_vel_max=2.5, cart_acc_max=6.0)
    return rows, prob


@pytest.mark.parametrize("args", [(1.0, 8, 16.0), (0.8, 8, 1.75), (1.0, 1, 16.0), (0.5, 2, 64.0)], ids=["plain", "cap", "one_round", "two_rounds"])
def test_audit_mode_synthetic_batch(hip_ctx, args):
    target, max_rounds, max_factor = args
    rows, prob = audit_batch()
    sres = steps(rows)
    want, report, final = sr.stretch_audit(rows, sres, 3, 3, prob, target, max_rounds, max_factor)
    st = [int(v) for v in report["status"]]
    # what each parameter set is there for
    if args == (1.0, 8, 16.0):
        assert set(st) == {capi.STRETCH_PASSES} and int(report["rounds"].max()) >= 2 and len(set(report["n_out"] - report["n_in"])) >= 4
    if args == (0.8, 8, 1.75):
        assert capi.STRETCH_CAPPED in st and capi.STRETCH_PASSES in st
        assert any(int(r["n_out"]) - 1 == int(np.floor((int(r["n_in"]) - 1) * 1.75)) for r in report if int(r["status"]) == capi.STRETCH_CAPPED)
    if max_rounds == 1:
        assert capi.STRETCH_ROUNDS in st and int(report["rounds"].max()) == 1
    out = capi.output_from_rows(hip_ctx, rows, sres, 3, 3, 0)
    new, got = out.stretch_audit(prob, target, max_rounds, max_factor)
    sr.assert_report_equal(got, report, f"report {args}")
    assert [int(n) for n in new.n_pts] == [int(n) for n in report["n_out"]]
    check_output(new, want, f"audit mode {args}")
    assert_audit_equal(new.audit(prob, 0.0), final, f"final audit {args}")
    assert new.stretch_ranges() == (int(report["rounds"].max()) or 1) and new.stretch_ms() >= 0.0
    new.close(); out.close()


_GOLDEN_RECORD = {}


@pytest.mark.parametrize("name", ["GEN7DOF", "KUKA-LWR-IV", "UR5"])
def test_audit_mode_golden_cases(hip_ctx, name):
    case = helpers.Case(name)
    out, b = helpers.run_to_output(hip_ctx, [case])
    prob = case.problem
    rows = [r.copy() for r in out.all_rows()]
    before = out.audit(prob, 0.0)
    new, got = out.stretch_audit(prob, 1.0, 8, 16.0)
    want, report, final = sr.stretch_audit(rows, out.sres, out.n_theta, out.n_cart, prob, 1.0, 8, 16.0)
    r = got[0]
    print(f"STRETCH {name}: {int(r['n_in'])} -> {int(r['n_out'])} points, factor {float(r['factor']):.4f}, rounds {int(r['rounds'])}, status {int(r['status'])}; "
          f"peaks before " + " ".join(f"{float(before[0]['fam'][f]['peak']):.4f}" for f in range(4)) +
          " after " + " ".join(f"{float(final[0]['fam'][f]['peak']):.4f}" for f in range(4)) + f"; kernels {new.stretch_ms():.3f} ms")
    sr.assert_report_equal(got, report, name)
    check_output(new, want, name)
    assert all(int(s) == capi.STRETCH_PASSES for s in got["status"]) and int(got["rounds"].max()) <= 8
    after = new.audit(prob, 0.0)
    assert_audit_equal(after, final, name)
    assert int(after[0]["n_over"]) == 0 and int(before[0]["n_over"]) > 0
    assert int(after[0]["n_nonfinite"]) == 0
    # the source is untouched
    for g, w in zip(out.all_rows(), rows):
        assert g.tobytes() == w.tobytes()
    new.close(); out.close(); b.close()


# ---- 6. stretch first, then the torque rows --------------------------------------------------------------------------------
def test_torque_rows_of_a_stretched_output(hip_ctx, oracle_lib):
    model = oracle_lib.builtin_serial_model(capi.ROBOT_KUKA)
    nl = model.n_links
    rng = np.random.default_rng(9)
    rows = [np.ascontiguousarray(np.cumsum(rng.uniform(-1.0, 1.0, (nl, n)), axis=1)) for n in (40, 0, 3, 17)]
    sres = steps(rows)
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    long = out.stretch_by(2.3)
    stretched = [r.copy() for r in long.all_rows()]
    for g, w in zip(stretched, sr.stretch_to(rows, [sr.n_out_by(r.shape[1], 2.3) for r in rows])):
        sr.assert_rows_equal(g, w, "stretched rows")
    new = long.torques(model, host_trig=True)
    for k, (g, w) in enumerate(zip(new.all_rows(), ir.with_torques(oracle_lib, model, stretched, sres, 0))):
        ir.assert_rows_bit_equal(g, w, f"torque rows of the stretched path {k}")
    # ... and not the other way round
    with pytest.raises(capi.BatotpError, match="torque rows"):
        new.stretch_by(2.0)
    for o in (new, long, out):
        o.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(hip_ctx, hip_lib):
    lib = hip_lib.lib
    rows = known_rows((3, 3))
    n_in = [r.shape[1] for r in rows]
    out = capi.output_from_rows(hip_ctx, rows, H, 3, 3, 0)
    with_trq = capi.output_from_rows(hip_ctx, [np.zeros((5, 6))], [H], 3, 0, 2)
    prob = capi.make_problem(3, 3, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON, jnt_vel_max=[1.0] * 3, jnt_acc_max=[1.0] * 3)
    I64P = C.POINTER(C.c_int64)

    def counts(v):
        return np.ascontiguousarray(v, dtype=np.int64)

    def refused(call, what, word=b"output_stretch"):
        h = C.c_void_p(0xdead)
        rc = call(C.byref(h))
        msg = lib.batotp_hip_last_error()
        assert rc == ERR_ARG and h.value is None and msg and word in msg, (what, rc, h.value, msg)

    ok = counts(n_in)
    refused(lambda h: lib.batotp_hip_output_stretch_to(None, ok.ctypes.data_as(I64P), h), "NULL output")
    refused(lambda h: lib.batotp_hip_output_stretch_to(out.handle, None, h), "NULL counts")
    assert lib.batotp_hip_output_stretch_to(out.handle, ok.ctypes.data_as(I64P), None) == ERR_ARG
    for k, v, what in ((0, n_in[0] - 1, "fewer points"), (1, 1, "points for an empty path"), (2, 2, "two points from one"),
                       (3, capi.STRETCH_MAX_POINTS + 1, "too many points"), (5, -1, "negative")):
        bad = counts(n_in); bad[k] = v
        refused(lambda h: lib.batotp_hip_output_stretch_to(out.handle, bad.ctypes.data_as(I64P), h), what)
    t1 = counts([6])
    refused(lambda h: lib.batotp_hip_output_stretch_to(with_trq.handle, t1.ctypes.data_as(I64P), h), "torque rows", b"torque rows")
    D = C.POINTER(C.c_double)
    for v in (0.999, np.nan, np.inf, -2.0, 1e30):
        f = np.full(len(rows), 1.5); f[4] = v
        refused(lambda h: lib.batotp_hip_output_stretch_by(out.handle, f.ctypes.data_as(D), h), f"factor {v}")
    f1 = np.ones(len(rows))
    refused(lambda h: lib.batotp_hip_output_stretch_by(None, f1.ctypes.data_as(D), h), "NULL output")
    refused(lambda h: lib.batotp_hip_output_stretch_by(out.handle, None, h), "NULL factors")
    refused(lambda h: lib.batotp_hip_output_stretch_by(with_trq.handle, f1.ctypes.data_as(D), h), "torque rows", b"torque rows")
    rep = np.zeros(len(rows), dtype=capi.STRETCH_DTYPE)
    rp = rep.ctypes.data_as(C.c_void_p)
    audit = lib.batotp_hip_output_stretch_audit
    refused(lambda h: audit(None, C.byref(prob), 1.0, 8, 16.0, h, rp), "NULL output")
    refused(lambda h: audit(out.handle, None, 1.0, 8, 16.0, h, rp), "NULL problem")
    refused(lambda h: audit(out.handle, C.byref(prob), 1.0, 8, 16.0, h, None), "NULL report")
    assert audit(out.handle, C.byref(prob), 1.0, 8, 16.0, None, rp) == ERR_ARG
    for target, rounds, factor, what in ((0.0, 8, 16.0, "target 0"), (1.0 + 1e-12, 8, 16.0, "target > 1"), (np.nan, 8, 16.0, "target NaN"),
                                         (1.0, 0, 16.0, "no rounds"), (1.0, 17, 16.0, "17 rounds"), (1.0, 8, 0.99, "max_factor < 1"),
                                         (1.0, 8, np.inf, "max_factor Inf"), (1.0, 8, np.nan, "max_factor NaN")):
        refused(lambda h: audit(out.handle, C.byref(prob), target, rounds, factor, h, rp), what)
    refused(lambda h: audit(with_trq.handle, C.byref(prob), 1.0, 8, 16.0, h, rp), "torque rows", b"torque rows")
    # ... and everything the audit refuses
    seven = capi.make_problem(7, 0, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0] * 7)
    refused(lambda h: audit(out.handle, C.byref(seven), 1.0, 8, 16.0, h, rp), "joint count", b"audit")
    nolimit = capi.make_problem(3, 3, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON, jnt_vel_max=[1.0] * 3, jnt_acc_max=[1.0, 0.0, 1.0])
    refused(lambda h: audit(out.handle, C.byref(nolimit), 1.0, 8, 16.0, h, rp), "a limit of 0", b"audit")
    assert not rep.view(np.uint8).any(), "a refused call writes no report"
    # the context still serves a valid call; no paths; paths without points
    new = out.stretch_by(1.0)
    for g, r in zip(new.all_rows(), rows):
        assert g.tobytes() == r.tobytes()
    new.close()
    empty = capi.output_from_rows(hip_ctx, [], [], 3, 3, 0)
    e, rep0 = empty.stretch_audit(prob)
    assert e.n_paths == 0 and (e.n_theta, e.n_cart, e.n_trq) == (3, 3, 0) and e.all_rows() == [] and rep0.shape == (0,) and e.stretch_ms() == 0.0
    e2 = empty.stretch_to([])
    hollow = capi.output_from_rows(hip_ctx, [np.zeros((6, 0))] * 3, [H] * 3, 3, 3, 0)
    h_, rep3 = hollow.stretch_audit(prob)
    assert [int(n) for n in h_.n_pts] == [0, 0, 0] and h_.stretch_ranges() == 0 and not rep3["status"].any() and [float(v) for v in rep3["factor"]] == [1.0] * 3
    for o in (e, e2, empty, h_, hollow, out, with_trq):
        o.close()


# ---- 8. the host route -----------------------------------------------------------------------------------------------------
def test_batch_driver_stretches_to_the_limits(tmp_path):
    """BA::setStretchToLimits through batest_batch --stretch on the reference's KUKA example"""
    exe = os.path.join(HOST, "_build", "batest_batch")
    assert os.path.exists(exe), "build() must produce batest_batch"
    src = os.path.join(helpers.GOLD, "KUKA-LWR-IV")
    for f in ("KUKApath.dat", "config.dat"):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    r = subprocess.run([exe, "config.dat", "3", "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0 and "stretch:" not in r.stdout, r.stdout[-2000:]
    plain = [ln for ln in r.stdout.splitlines() if ln.startswith("audit (tol 0):")]
    assert len(plain) == 1 and "; over: 0(" in plain[0], r.stdout[-2000:]
    r = subprocess.run([exe, "config.dat", "3", "--stretch", "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("stretch (target 1):")]
    assert len(lines) == 1, r.stdout[-2000:]
    w = lines[0].split()
    # stretch (target 1): 3 of 3 paths stretched, largest factor 1.55.. (path 0), 0 not passing, 0 skipped
    assert (w[3], w[5]) == ("3", "3") and 1.4 < float(w[10]) < 1.7 and w[w.index("not") - 1] == "0" and w[-2] == "0", lines[0]
    after = [ln for ln in r.stdout.splitlines() if ln.startswith("audit (tol 0):")]
    assert len(after) == 1 and after[0].endswith("; over: none"), r.stdout[-2000:]
    # the trajectory written for the first path is the stretched one
    n_plain = helpers.read_traj_out(os.path.join(helpers.GOLD, "KUKA-LWR-IV", "ref_traj_out.dat"), 7, 3)[1]
    sres, n, theta, cart, trq = helpers.read_traj_out(str(tmp_path / "out_first" / "traj_out.dat"), 7, 3)
    assert abs((n - 1) - (n_plain - 1) * float(w[10])) < 0.01 and theta.shape == (7, n) and cart is not None and trq is None
    r = subprocess.run([exe, "config.dat", "2", "--stretch", "0.5"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0 and any(ln.startswith("stretch (target 0.5): 2 of 2 paths stretched") for ln in r.stdout.splitlines()), r.stdout[-2000:]
    # planned with torque limits: the output carries the stage's own torque rows and is left as it is
    work = tmp_path / "rr"
    work.mkdir()
    for f in ("RRlemniscate.dat", "config.dat"):
        shutil.copy(os.path.join(helpers.GOLD, "RR", f), work / f)
    r = subprocess.run([exe, "config.dat", "2", "--stretch"], cwd=work, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert any(ln.startswith("stretch (target 1): 0 of 2 paths stretched") and ln.endswith("0 not passing, 2 skipped") for ln in r.stdout.splitlines()), r.stdout[-2000:]
    sres, n, theta, cart, trq = helpers.read_traj_out(str(work / "out_first" / "traj_out.dat"), 2, 3)
    assert n == helpers.read_traj_out(os.path.join(helpers.GOLD, "RR", "ref_traj_out.dat"), 2, 3)[1] and trq is not None
