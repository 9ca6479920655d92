"""CPU (-m "not gpu"): torque rows for finished trajectories (include/batotp_hip_invdyn.h) as far as they go without a device --
the restated definition (tests/invdyn_reference.py) against a naive per-point loop in Python floats, its second-order convergence
to the analytic inverse dynamics on a smooth trajectory, the symbol tables, and that a program using BA::setOutputTorques
compiles and links against the host library."""
import math
import os
import subprocess

import numpy as np
import pytest

import helpers
import invdyn_reference as ir
from batotp_amd import capi

ROOT = helpers.ROOT
HOST = os.path.join(ROOT, "batotp_amd", "host")
CSRC = os.path.join(ROOT, "batotp_amd", "csrc")
INVDYN_SYMBOLS = ["batotp_hip_output_torques", "batotp_hip_output_torques_ms", "batotp_hip_output_torques_ranges"]


def naive_rows(oracle_lib, model, x, h):
    """the definition point by point, every operation on Python floats"""
    nl, n = len(x), len(x[0])
    unit = ir.DEG2RAD if model.degrees else 1.0
    c1, c2 = 1.0 / (2.0 * h), 1.0 / (h * h)
    out = np.empty((nl, n))
    for i in range(n):
        q, qd, qdd = [], [], []
        for j in range(nl):
            v = a = 0.0
            if n >= 3:
                ic = min(max(i, 1), n - 2)
                xm, x0, xp = float(x[j][ic - 1]), float(x[j][ic]), float(x[j][ic + 1])
                v = (xp - xm) * c1
                a = ((xp - x0) - (x0 - xm)) * c2
            q.append(unit * float(x[j][i])); qd.append(unit * v); qdd.append(unit * a)
        out[:, i] = ir.torque_point(oracle_lib, model, q, qd, qdd)
    return out


@pytest.mark.parametrize("robot", [capi.ROBOT_KUKA, capi.ROBOT_RR])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 9])
def test_reference_equals_the_naive_loop(oracle_lib, robot, n):
    model = oracle_lib.builtin_serial_model(robot)
    rng = np.random.default_rng(100 * robot + n)
    x = rng.uniform(-90.0, 90.0, (model.n_links, n))
    h = 0.008
    want = naive_rows(oracle_lib, model, x, h)
    got = ir.torque_rows(oracle_lib, model, x, h)
    ir.assert_rows_bit_equal(got, want, f"robot {robot}, n {n}")
    assert got.shape == (model.n_links, n) and np.isfinite(got).all()
    v, a = ir.differences(x, h)
    if n < 3:
        # no differences: +0.0 everywhere (the torques are those of the arm at rest: gravity alone)
        assert v.view(np.uint64).sum() == 0 and a.view(np.uint64).sum() == 0
    else:
        # the end points take the differences of their interior neighbour
        assert v[:, 0].tobytes() == v[:, 1].tobytes() and v[:, -1].tobytes() == v[:, -2].tobytes()
        assert a[:, 0].tobytes() == a[:, 1].tobytes() and a[:, -1].tobytes() == a[:, -2].tobytes()
        assert np.abs(v).max() > 0 and np.abs(a).max() > 0


def test_interior_torques_converge_at_second_order(oracle_lib):
    """sums of sines on the 7-link arm: the error against bo_rnea with the analytic rates falls by ~4 when h is halved.  The steps are
    large enough that rounding is not yet visible: the second difference carries a rounding error of about 4 ulp(max |x|) / h^2,
    whose effect on the torques is measured here and has to stay below a thousandth of the truncation error at the smallest h."""
    model = oracle_lib.builtin_serial_model(capi.ROBOT_KUKA)
    nl = model.n_links
    assert nl == 7 and model.degrees == 1
    rng = np.random.default_rng(7)
    A, B = rng.uniform(20.0, 60.0, nl), rng.uniform(5.0, 15.0, nl)               # degrees
    w1, w2 = rng.uniform(0.5, 2.0, nl), rng.uniform(2.0, 4.0, nl)                # rad / s
    p1, p2 = rng.uniform(0, 6, nl), rng.uniform(0, 6, nl)

    def x_of(t):
        return A[:, None] * np.sin(w1[:, None] * t + p1[:, None]) + B[:, None] * np.sin(w2[:, None] * t + p2[:, None])

    def v_of(t):
        return A[:, None] * w1[:, None] * np.cos(w1[:, None] * t + p1[:, None]) + B[:, None] * w2[:, None] * np.cos(w2[:, None] * t + p2[:, None])

    def a_of(t):
        return -A[:, None] * w1[:, None] ** 2 * np.sin(w1[:, None] * t + p1[:, None]) - B[:, None] * w2[:, None] ** 2 * np.sin(w2[:, None] * t + p2[:, None])

    T = 2.0
    errs, scale = [], None
    steps = [0.04, 0.02, 0.01]
    for h in steps:
        n = int(round(T / h)) + 1
        t = h * np.arange(n)
        x = x_of(t)
        got = ir.torque_rows(oracle_lib, model, x, h)
        q, qd, qdd = ir.DEG2RAD * x, ir.DEG2RAD * v_of(t), ir.DEG2RAD * a_of(t)
        exact = np.stack([ir.torque_point(oracle_lib, model, q[:, i], qd[:, i], qdd[:, i]) for i in range(n)], axis=1)
        errs.append(float(np.abs(got[:, 1:-1] - exact[:, 1:-1]).max()))
        scale = float(np.abs(exact).max())
    print(f"INVDYN convergence: max |tau| {scale:.3f} Nm, errors {errs} at h {steps}")
    for coarse, fine in zip(errs, errs[1:]):
        assert 3.0 <= coarse / fine <= 5.0, errs
    # the chosen steps: rounding of the second difference, pushed through the recursion at one configuration
    h = steps[-1]
    da = 4.0 * np.spacing(float(np.abs(x).max())) / (h * h)
    i = n // 2
    bumped = ir.torque_point(oracle_lib, model, q[:, i], qd[:, i], qdd[:, i] + ir.DEG2RAD * da)
    rounding = float(np.abs(bumped - exact[:, i]).max())
    assert rounding < 1e-3 * errs[-1], (rounding, errs)


def test_library_exports_the_torque_rows_and_the_checker_does_not(hip_lib, oracle_lib):
    assert hip_lib.has_invdyn and hip_lib.invdyn_symbols == sorted(INVDYN_SYMBOLS)
    for name in INVDYN_SYMBOLS:
        assert hasattr(hip_lib.lib, name), name
        assert name not in hip_lib.symbols and name not in hip_lib.audit_symbols and name not in hip_lib.kin_symbols
        assert not hasattr(oracle_lib.lib, name)
    assert oracle_lib.has_invdyn is False
    new = open(os.path.join(ROOT, "include", "batotp_hip_invdyn.h")).read()
    assert '#include "batotp_hip.h"' in new
    for name in INVDYN_SYMBOLS:
        assert f"int {name}(" in new
    assert f"#define BATOTP_INVDYN_BLOCK_POINTS {capi.INVDYN_BLOCK_POINTS}\n" in new


def test_a_program_using_set_output_torques_links_against_the_host_library(tmp_path):
    exe = tmp_path / "invdyn_batch"
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", f"-I{HOST}", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "drivers", "invdyn_batch_main.cpp"),
           os.path.join(HOST, "_build", "libbatotp.a"), f"-L{CSRC}", "-lbatotp_hip", f"-Wl,-rpath,{CSRC}", "-pthread", "-lm", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert exe.exists()
    # the seam: only ba_invdyn.o of the host library refers to the new entry points
    nm = subprocess.run(["nm", "-A", os.path.join(HOST, "_build", "libbatotp.a")], capture_output=True, text=True)
    assert nm.returncode == 0
    users = {ln.split(":")[1] for ln in nm.stdout.splitlines() if "batotp_hip_output_torques" in ln}
    assert users == {"ba_invdyn.o"}, users
