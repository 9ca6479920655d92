"""CPU (-m "not gpu"): the time stretch of finished trajectories (include/batotp_hip_stretch.h) as far as it goes without a device --
the numpy reference of its definition against a naive per-point loop, what the cubic reproduces, how the audited peaks fall, the
struct layout, the exported symbols, and the rounds of the audit mode on the reference binary's own trajectories."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import helpers
import stretch_reference as sr
from audit_reference import audit_path
from batotp_amd import capi

ROOT = helpers.ROOT
LENGTHS = [0, 1, 2, 3, 4, 5, 33]


def targets(n):
    """n2 = n, n + 1, 2n - 1 (f = 0.5 exactly at every other point) and a factor of about 7.3 that is no integer"""
    if n < 2:
        return [n]
    return [n, n + 1, 2 * n - 1, sr.n_out_by(n, 7.3)]


def naive_stretch(rows, n2):
    """the definition point by point, in Python floats (binary64)"""
    R, n = rows.shape
    x = [[float(v) for v in rows[r]] for r in range(R)]
    if n2 == n or n < 2:
        return np.array(x, dtype=np.float64).reshape(R, n)
    rk = float(n - 1) / float(n2 - 1)
    y = np.empty((R, n2))
    for r in range(R):
        for p in range(n2 - 1):
            u = float(p) * rk
            j = min(int(u), n - 2)
            f = u - float(j)
            d = x[r][j + 1] - x[r][j]
            m0 = (x[r][j + 1] - x[r][j - 1]) * 0.5 if j >= 1 else d
            m1 = (x[r][j + 2] - x[r][j]) * 0.5 if j + 2 <= n - 1 else d
            c2 = (3.0 * d - 2.0 * m0) - m1
            c3 = (m0 + m1) - 2.0 * d
            y[r, p] = x[r][j] + f * (m0 + f * (c2 + f * c3))
        y[r, n2 - 1] = x[r][n - 1]
    return y


@pytest.mark.parametrize("R", [1, 3, 7])
def test_numpy_reference_equals_a_naive_loop(R):
    rng = np.random.default_rng(77 + R)
    for trial in range(3):
        for n in LENGTHS:
            rows = rng.standard_normal((R, n)) * [1.0, 1e-3, 1e6][trial]
            if trial == 2 and n >= 4:
                rows[0, 0], rows[R - 1, n - 1], rows[R // 2, n // 2] = np.inf, -np.inf, np.nan
            for n2 in targets(n):
                got, want = sr.stretch_rows(rows, n2), naive_stretch(rows, n2)
                assert got.shape == (R, n2)
                sr.assert_rows_equal(got, want, f"R {R} trial {trial} n {n} n2 {n2}")
                if trial < 2:
                    assert got.tobytes() == want.tobytes()


def test_n_out_by():
    assert [sr.n_out_by(n, 2.0) for n in (0, 1, 2, 3, 34)] == [0, 1, 3, 5, 67]
    assert sr.n_out_by(11, 1.0) == 11 and sr.n_out_by(11, 1.05) == 12 and sr.n_out_by(34, 7.3) == 242


def test_first_and_last_point_are_reproduced_exactly():
    rng = np.random.default_rng(5)
    for n in (2, 3, 4, 5, 33, 257):
        rows = rng.standard_normal((4, n)) * 100.0
        for n2 in targets(n) + [64 * n]:
            y = sr.stretch_rows(rows, n2)
            assert y[:, 0].tobytes() == rows[:, 0].tobytes() and y[:, -1].tobytes() == rows[:, -1].tobytes(), (n, n2)
    # source points that fall on new points are reproduced too: n2 - 1 a multiple of n - 1, f = 0 there
    rows = rng.standard_normal((2, 9))
    y = sr.stretch_rows(rows, 8 * 4 + 1)
    assert y[:, ::4].tobytes() == rows.tobytes()


def test_a_linear_row_is_reproduced_to_a_few_ulp():
    n = 33
    x = 0.37 + 0.013 * np.arange(n)
    for n2 in targets(n) + [64 * n]:
        y = sr.stretch_rows(x[None, :], n2)[0]
        want = 0.37 + 0.013 * (np.arange(n2) * ((n - 1) / (n2 - 1)))
        # |x| < 1: one ulp is at most 2^-53 of 1; the cubic's coefficients cancel to rounding and u itself carries an ulp of 32
        assert np.abs(y - want).max() <= 8 * 32 * 2.0 ** -53, (n2, np.abs(y - want).max())


def test_a_quadratic_row_is_reproduced_on_the_inner_cells():
    """central differences are the exact tangents of a parabola, so the cubic IS the parabola on the cells 1 <= j <= n-3"""
    n = 33
    t = np.arange(n, dtype=np.float64)
    x = 0.25 * t * t - 3.0 * t + 1.0          # exact in binary64
    for n2 in targets(n) + [64 * n]:
        y = sr.stretch_rows(x[None, :], n2)[0]
        u = np.arange(n2 - 1) * ((n - 1) / (n2 - 1))
        j = np.minimum(u.astype(np.int64), n - 2)
        inner = (j >= 1) & (j <= n - 3)
        want = 0.25 * u * u - 3.0 * u + 1.0
        scale = np.abs(x).max()                # 161
        assert np.abs(y[:-1][inner] - want[inner]).max() <= 16 * scale * 2.0 ** -53, n2
        if n2 > n:
            assert np.abs(y[:-1][~inner] - want[~inner]).max() > 1e-5     # the end cells are one-sided: no parabola there


@pytest.mark.parametrize("k", [1.5, 2.0, 3.0, 7.3])
def test_the_audited_peaks_fall_as_k_and_k_squared(k):
    # whole half periods: the acceleration vanishes at both ends, where the one-sided tangents of the end cells would otherwise let the
    # cubic's second derivative reach twice the source's second difference (include/batotp_hip_stretch.h) -- the rule is about the
    # interior
    n, h = 2001, 0.004
    t = h * np.arange(n)
    amp, w = np.array([1.0, 0.5, 2.0]), np.pi * np.array([0.5, 1.0, 0.75])
    rows = amp[:, None] * np.sin(w[:, None] * t[None, :])
    prob = capi.make_problem(3, 0, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON, jnt_vel_max=[1.0] * 3, jnt_acc_max=[1.0] * 3)
    before = audit_path(rows, h, 3, 0, 0, prob, 0.0)
    n2 = sr.n_out_by(n, k)
    kk = (n2 - 1) / (n - 1)
    after = audit_path(sr.stretch_rows(rows, n2), h, 3, 0, 0, prob, 0.0)
    v0, a0 = (float(before["fam"][f]["peak"]) for f in (capi.AUDIT_JNT_VEL, capi.AUDIT_JNT_ACC))
    v1, a1 = (float(after["fam"][f]["peak"]) for f in (capi.AUDIT_JNT_VEL, capi.AUDIT_JNT_ACC))
    assert abs(v0 - (amp * w).max()) < 1e-3 * v0 and abs(a0 - (amp * w * w).max()) < 1e-3 * a0
    # second-order error of the differences and of the tangents: (w h)^2 / 6 and / 12 are below 2.7e-5 for w <= pi; the peak of a
    # sampled sine misses the true one by at most (w h / 2)^2 / 2 = 2e-5 -- 1e-3 leaves room for all of them together
    assert abs(v1 * kk - v0) <= 1e-3 * v0, (v0, v1, kk)
    assert abs(a1 * kk * kk - a0) <= 1e-3 * a0, (a0, a1, kk)


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of batotp_path_stretch as the system compiler lays it out = capi.PathStretch and capi.STRETCH_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "batotp_hip_stretch.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %zu %zu %d %lld %d %d %d\\n", sizeof(batotp_path_stretch), offsetof(batotp_path_stretch, n_in),\n'
        "         offsetof(batotp_path_stretch, n_out), offsetof(batotp_path_stretch, factor), offsetof(batotp_path_stretch, rounds),\n"
        "         offsetof(batotp_path_stretch, status), BATOTP_STRETCH_BLOCK_POINTS, (long long)BATOTP_STRETCH_MAX_POINTS,\n"
        "         BATOTP_STRETCH_PASSES, BATOTP_STRETCH_ROUNDS, BATOTP_STRETCH_CAPPED);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    PS = capi.PathStretch
    want = [C.sizeof(PS), PS.n_in.offset, PS.n_out.offset, PS.factor.offset, PS.rounds.offset, PS.status.offset, capi.STRETCH_BLOCK_POINTS,
            capi.STRETCH_MAX_POINTS, capi.STRETCH_PASSES, capi.STRETCH_ROUNDS, capi.STRETCH_CAPPED]
    assert got == want
    assert got[:6] == [32, 0, 8, 16, 24, 28]
    d = capi.STRETCH_DTYPE
    assert d.itemsize == 32 and [d.fields[f][1] for f in ("n_in", "n_out", "factor", "rounds", "status")] == got[1:6]


STRETCH_SYMBOLS = ["batotp_hip_output_stretch_to", "batotp_hip_output_stretch_by", "batotp_hip_output_stretch_audit",
                   "batotp_hip_output_stretch_ms", "batotp_hip_output_stretch_ranges"]


def test_product_library_exports_the_stretch(hip_lib):
    assert hip_lib.has_stretch
    assert hip_lib.stretch_symbols == sorted(STRETCH_SYMBOLS)
    for name in STRETCH_SYMBOLS:
        assert hasattr(hip_lib.lib, name), name
        assert name not in hip_lib.symbols      # `symbols` stays the table of include/batotp_hip.h
    new = open(os.path.join(ROOT, "include", "batotp_hip_stretch.h")).read()
    assert '#include "batotp_hip_audit.h"' in new
    for name in STRETCH_SYMBOLS:
        assert f"int {name}(" in new


def test_checker_has_no_stretch_and_says_so(oracle_lib, oracle_ctx):
    assert oracle_lib.has_stretch is False
    for name in STRETCH_SYMBOLS:
        assert not hasattr(oracle_lib.lib, name)
    case = helpers.Case("synth_gen7dof_s0")
    out, b = helpers.run_to_output(oracle_ctx, [case])
    for call in (lambda: out.stretch_to(out.n_pts), lambda: out.stretch_by(2.0), lambda: out.stretch_audit(case.problem), out.stretch_ms,
                 out.stretch_ranges):
        with pytest.raises(capi.BatotpError, match="stretch entry points"):
            call()
    out.close(); b.close()


def golden_rows(name):
    """(case, rows[n_theta + n_cart][n] promoted from the reference binary's float32 traj_out.dat, sres, n_cart)"""
    case = helpers.Case(name)
    nJ = case.problem.n_joints
    n_cart_file = 6 if case.problem.n_cart == 7 else case.problem.n_cart
    sres, n, theta, cart, trq = helpers.read_traj_out(os.path.join(case.dir, "ref_traj_out.dat"), nJ, n_cart_file)
    rows = theta.astype(np.float64) if cart is None else np.concatenate([theta.astype(np.float64), cart.astype(np.float64)])
    return case, np.ascontiguousarray(rows), float(sres), 0 if cart is None else n_cart_file


@pytest.mark.parametrize("name", ["GEN7DOF", "KUKA-LWR-IV", "UR5"])
def test_the_audit_mode_passes_on_the_reference_trajectories(name):
    case, rows, sres, n_cart = golden_rows(name)
    nJ = case.problem.n_joints
    before = audit_path(rows, sres, nJ, n_cart, 0, case.problem, 0.0)
    out, report, final = sr.stretch_audit([rows], sres, nJ, n_cart, case.problem, target=1.0, max_rounds=8, max_factor=16.0)
    r = report[0]
    print(f"STRETCH reference {name}: {int(r['n_in'])} -> {int(r['n_out'])} points, factor {float(r['factor']):.4f}, rounds {int(r['rounds'])}, "
          f"peaks before " + " ".join(f"{float(before['fam'][f]['peak']):.4f}" for f in range(4)) +
          " after " + " ".join(f"{float(final[0]['fam'][f]['peak']):.4f}" for f in range(4)))
    assert int(r["status"]) == capi.STRETCH_PASSES and 1 <= int(r["rounds"]) <= 8
    assert int(final[0]["n_over"]) == 0 and int(final[0]["n_nonfinite"]) == 0
    assert all(float(final[0]["fam"][f]["peak"]) <= 1.0 for f in range(4))
    assert out[0].shape == (rows.shape[0], int(r["n_out"])) and float(r["factor"]) > 1.0
    # the report's record is the audit of the rows it returns
    again = audit_path(out[0], sres, nJ, n_cart, 0, case.problem, 0.0)
    assert again.tobytes() == final[0].tobytes()


def test_audit_mode_cap_and_rounds():
    """a path that needs a factor of 4: capped at 2 it is stretched once, to the bound; one round leaves it over the target"""
    n, h = 101, 0.01
    t = h * np.arange(n)
    rows = np.sin(2.0 * t)[None, :] * 2.0             # |v| up to 4, |a| up to 8
    prob = capi.make_problem(1, 0, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON, jnt_vel_max=[1.0], jnt_acc_max=[100.0])
    out, report, final = sr.stretch_audit([rows], h, 1, 0, prob, 1.0, 8, 2.0)
    assert (int(report[0]["n_out"]), int(report[0]["rounds"]), int(report[0]["status"])) == (201, 1, capi.STRETCH_CAPPED)
    assert float(report[0]["factor"]) == 2.0 and float(final[0]["fam"][0]["peak"]) > 1.9
    out, report, final = sr.stretch_audit([rows], h, 1, 0, prob, 1.0, 8, 1.0)        # no room at all: capped where it stands
    assert (int(report[0]["n_out"]), int(report[0]["rounds"]), int(report[0]["status"])) == (101, 0, capi.STRETCH_CAPPED)
    assert out[0].tobytes() == rows.tobytes()
    out, report, final = sr.stretch_audit([rows], h, 1, 0, prob, 1.0, 8, 16.0)
    assert int(report[0]["status"]) == capi.STRETCH_PASSES and 4.0 <= float(report[0]["factor"]) < 4.1
    # a jump: the first round cannot know the factor the cubic's overshoot asks for
    step = np.concatenate([np.zeros(40), [0.02], np.full(40, 0.05)])[None, :]
    prob = capi.make_problem(1, 0, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON, jnt_vel_max=[100.0], jnt_acc_max=[100.0])
    out1, rep1, fin1 = sr.stretch_audit([step], h, 1, 0, prob, 1.0, 1, 64.0)
    outN, repN, finN = sr.stretch_audit([step], h, 1, 0, prob, 1.0, 16, 64.0)
    assert int(repN[0]["status"]) == capi.STRETCH_PASSES and int(fin1[0]["n_pts"]) == int(rep1[0]["n_out"])
    assert int(rep1[0]["rounds"]) == 1 and int(rep1[0]["status"]) in (capi.STRETCH_PASSES, capi.STRETCH_ROUNDS)
    # paths that pass, and paths too short to audit, come back as they are
    quiet = [np.zeros((1, 0)), np.ones((1, 1)), np.array([[0.0, 9.0]]), 1e-3 * np.sin(t)[None, :]]
    out, report, final = sr.stretch_audit(quiet, h, 1, 0, prob, 0.5, 4, 8.0)
    assert [int(v) for v in report["n_out"]] == [0, 1, 2, n] and not report["rounds"].any() and not report["status"].any()
    assert [float(v) for v in report["factor"]] == [1.0] * 4
