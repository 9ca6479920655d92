"""CPU (-m "not gpu"): the audit of finished trajectories (include/batotp_hip_audit.h) as far as it goes without a device --
the numpy reference of its definition against a naive per-point loop, the struct layout, the exported symbols, and that the
C-ABI of include/batotp_hip.h and the checker behind it are untouched."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from audit_reference import audit_reference, audit_path, assert_audit_equal, audited_families
from batotp_amd import capi

ROOT = helpers.ROOT
ALL_ON = capi.F_JNT_ACC_ON | capi.F_TRQ_ON | capi.F_CART_VEL_ON | capi.F_CART_ACC_ON | capi.F_PARALLEL
# include/batotp_hip.h at the commit before the audit: the audit has a header of its own and must not touch this one
BATOTP_HIP_H_SHA256 = "3644ea2b7838670d13a1ba947917c008f07ef305461101c3883367c4b77f4533"


def problem(n_theta=7, n_cart=3, flags=ALL_ON):
    return capi.make_problem(n_theta, n_cart, capi.ROBOT_CSPR3DOF, flags,
                             jnt_vel_max=[2.0, 1.5, 4.0, 1.0, 3.0, 2.5, 0.5, 1.0][:max(n_theta, 1)],
                             jnt_acc_max=[8.0, 16.0, 4.0, 2.0, 32.0, 1.0, 64.0, 2.0][:max(n_theta, 1)],
                             jnt_trq_max=[10.0, 7.0, 3.0, 1.0, 1.0, 1.0, 1.0, 1.0], jnt_trq_min=[-6.0, 1.0, -3.0, -1.0, -1.0, -1.0, -1.0, -1.0],
                             cart_vel_max=1.25, cart_acc_max=6.0)


def naive_audit(rows, h, nT, nC, nQ, prob, tol):
    """the definition point by point, in Python floats (binary64): (peaks[5] as (u, at, row), n_over, n_nonfinite)"""
    R, n = rows.shape
    on = audited_families(prob, nT, nC, nQ)
    best = [(-1.0, -1, -1)] * 5
    x = [[float(v) for v in rows[r]] for r in range(R)]

    def offer(f, u, i, r):
        if not math.isfinite(u):
            return False
        bu, bi, br = best[f]
        if u > bu or (u == bu and (i < bi or (i == bi and r < br))):
            best[f] = (u, i, r)
        return u > 1.0 + tol

    n_over = 0
    nonfinite = sum(1 for r in range(R) for v in x[r] if not math.isfinite(v))
    if n >= 3:
        c1, c2 = 1.0 / (2.0 * h), 1.0 / (h * h)
    for i in range(n):
        over = False
        if 1 <= i <= n - 2:
            vel = lambda r: (x[r][i + 1] - x[r][i - 1]) * c1
            acc = lambda r: ((x[r][i + 1] - x[r][i]) - (x[r][i] - x[r][i - 1])) * c2
            for j in range(nT):
                if on[0]:
                    over |= offer(0, math.fabs(vel(j)) * (1.0 / prob.jnt_vel_max[j]), i, j)
                if on[1]:
                    over |= offer(1, math.fabs(acc(j)) * (1.0 / prob.jnt_acc_max[j]), i, j)
            for f, d, limit in ((2, vel, prob.cart_vel_max), (3, acc, prob.cart_acc_max)):
                if on[f]:
                    s = None
                    for k in range(min(3, nC)):
                        t = d(nT + k)
                        s = t * t if s is None else s + t * t
                    root = math.sqrt(s) if s >= 0.0 else float("nan")   # (NaN stays NaN; math.sqrt would raise on it)
                    over |= offer(f, root * (1.0 / limit), i, 0)
        if on[4]:
            for r in range(nQ):
                mid = (prob.jnt_trq_max[r] + prob.jnt_trq_min[r]) * 0.5
                half = (prob.jnt_trq_max[r] - prob.jnt_trq_min[r]) * 0.5
                over |= offer(4, math.fabs(x[nT + nC + r][i] - mid) * (1.0 / half), i, r)
        n_over += bool(over)
    return best, n_over, nonfinite


@pytest.mark.parametrize("shape", [(7, 3, 3), (3, 0, 0), (2, 6, 2), (3, 1, 3), (1, 2, 0)])
def test_numpy_reference_equals_a_naive_loop(shape):
    nT, nC, nQ = shape
    rng = np.random.default_rng(1234 + 100 * nT + 10 * nC + nQ)
    prob = problem(nT, nC)
    R = nT + nC + nQ
    lengths = [0, 1, 2, 3, 4, 7, 33, 150]
    for trial in range(6):
        flags = ALL_ON if trial < 3 else int(rng.integers(0, 16)) | capi.F_PARALLEL
        prob.flags = flags
        tol = [0.0, 0.05, 0.5][trial % 3]
        for n in lengths:
            rows = rng.standard_normal((R, n)) * 0.1
            if trial % 2 == 0 and n >= 3:
                rows = np.round(rows * 40.0) / 8.0      # few distinct values: ties of the peak at several points and rows
            if trial >= 1 and n >= 4:
                for bad in (np.nan, np.inf, -np.inf):
                    rows[int(rng.integers(0, R)), int(rng.integers(0, n))] = bad
                rows[0, 0] = np.nan
                rows[R - 1, n - 1] = np.inf
            h = [0.5, 0.01, 0.008][trial % 3]
            got = audit_path(rows, h, nT, nC, nQ, prob, tol)
            best, n_over, nonfinite = naive_audit(rows, h, nT, nC, nQ, prob, tol)
            what = f"shape {shape} trial {trial} n {n}"
            for f in range(5):
                g = got["fam"][f]
                assert (float(g["peak"]), int(g["at"]), int(g["row"])) == best[f], (what, capi.AUDIT_FAMILIES[f])
                assert np.float64(best[f][0]).tobytes() == g["peak"].tobytes(), what
            assert (int(got["n_pts"]), int(got["n_over"]), int(got["n_nonfinite"])) == (n, n_over, nonfinite), what


def test_reference_tie_rule_and_empty_families():
    """the lowest point wins, then the lowest row; a family without a point, or without a finite utilisation, is -1"""
    prob = problem(2, 0, capi.F_JNT_ACC_ON)
    prob.jnt_vel_max[0] = prob.jnt_vel_max[1] = 1.0
    rows = np.zeros((2, 8))
    rows[1, 2] = 1.0      # row 1: |v| = 1 at points 1 and 3
    rows[0, 4] = 1.0      # row 0: |v| = 1 at points 3 and 5
    a = audit_path(rows, 0.5, 2, 0, 0, prob, 0.0)
    assert (float(a["fam"][0]["peak"]), int(a["fam"][0]["at"]), int(a["fam"][0]["row"])) == (1.0, 1, 1)
    a = audit_path(rows[::-1], 0.5, 2, 0, 0, prob, 0.0)
    assert (float(a["fam"][0]["peak"]), int(a["fam"][0]["at"]), int(a["fam"][0]["row"])) == (1.0, 1, 0)
    both = np.zeros((2, 8)); both[:, 4] = 1.0   # the same peak in both rows at point 3: the lowest row
    a = audit_path(both, 0.5, 2, 0, 0, prob, 0.0)
    assert (int(a["fam"][0]["at"]), int(a["fam"][0]["row"])) == (3, 0)
    for n in (0, 1, 2):
        a = audit_path(np.ones((2, n)), 0.5, 2, 0, 0, prob, 0.0)
        assert all(float(a["fam"][f]["peak"]) == -1.0 and int(a["fam"][f]["at"]) == -1 and int(a["fam"][f]["row"]) == -1 for f in range(5))
        assert int(a["n_pts"]) == n and int(a["n_over"]) == 0
    a = audit_path(np.full((2, 5), np.nan), 0.5, 2, 0, 0, prob, 0.0)
    assert float(a["fam"][0]["peak"]) == -1.0 and int(a["n_nonfinite"]) == 10 and int(a["n_over"]) == 0


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of batotp_path_audit as the system compiler lays it out = capi.PathAudit and capi.AUDIT_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "batotp_hip_audit.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(batotp_path_audit), sizeof(batotp_audit_peak),\n'
        "         offsetof(batotp_audit_peak, peak), offsetof(batotp_audit_peak, at), offsetof(batotp_audit_peak, row),\n"
        "         offsetof(batotp_path_audit, fam), offsetof(batotp_path_audit, n_pts), offsetof(batotp_path_audit, n_over),\n"
        "         offsetof(batotp_path_audit, n_nonfinite), BATOTP_AUDIT_BLOCK_POINTS, BATOTP_AUDIT_FAMILIES);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    PA, PK = capi.PathAudit, capi.AuditPeak
    want = [C.sizeof(PA), C.sizeof(PK), PK.peak.offset, PK.at.offset, PK.row.offset, PA.fam.offset, PA.n_pts.offset, PA.n_over.offset,
            PA.n_nonfinite.offset, capi.AUDIT_BLOCK_POINTS, len(capi.AUDIT_FAMILIES)]
    assert got == want
    assert got[:2] == [144, 24]
    d = capi.AUDIT_DTYPE
    assert d.itemsize == 144 and d.fields["n_pts"][1] == PA.n_pts.offset and d.fields["n_over"][1] == PA.n_over.offset
    assert d.fields["n_nonfinite"][1] == PA.n_nonfinite.offset and d.fields["fam"][0].base.itemsize == 24
    assert [capi.AUDIT_JNT_VEL, capi.AUDIT_JNT_ACC, capi.AUDIT_CART_VEL, capi.AUDIT_CART_ACC, capi.AUDIT_TRQ] == [0, 1, 2, 3, 4]


AUDIT_SYMBOLS = ["batotp_hip_output_audit", "batotp_hip_output_audit_device", "batotp_hip_output_audit_ms", "batotp_hip_output_from_rows"]


def test_product_library_exports_the_audit(hip_lib):
    assert hip_lib.has_audit
    assert hip_lib.audit_symbols == sorted(AUDIT_SYMBOLS)
    for name in AUDIT_SYMBOLS:
        assert hasattr(hip_lib.lib, name), name
        assert name not in hip_lib.symbols      # `symbols` stays the table of include/batotp_hip.h


def test_checker_still_loads_and_has_no_audit(oracle_lib, oracle_ctx):
    assert oracle_lib.has_audit is False
    assert "batotp_hip_output" in oracle_lib.symbols
    for name in AUDIT_SYMBOLS:
        assert not hasattr(oracle_lib.lib, name)
    # a call that needs the entry points says so instead of crashing
    case = helpers.Case("synth_gen7dof_s0")
    out, b = helpers.run_to_output(oracle_ctx, [case])
    with pytest.raises(capi.BatotpError, match="audit entry points"):
        out.audit(case.problem)
    with pytest.raises(capi.BatotpError, match="audit entry points"):
        out.audit_ms()
    with pytest.raises(capi.BatotpError, match="audit entry points"):
        capi.output_from_rows(oracle_ctx, [np.zeros((7, 4))], 0.01, 7, 0, 0)
    out.close(); b.close()


def test_public_header_is_unchanged():
    raw = open(os.path.join(ROOT, "include", "batotp_hip.h"), "rb").read()
    assert hashlib.sha256(raw).hexdigest() == BATOTP_HIP_H_SHA256
    assert b"audit" not in raw
    new = open(os.path.join(ROOT, "include", "batotp_hip_audit.h")).read()
    assert '#include "batotp_hip.h"' in new
    for name in AUDIT_SYMBOLS:
        assert f"int {name}(" in new
