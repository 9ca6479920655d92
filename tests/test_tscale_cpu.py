"""CPU (-m "not gpu"): the torque scale of finished trajectories (include/batotp_hip_tscale.h) as far as it goes without a device -- the
numpy reference of its definition against a naive per-point loop, the root rule against numpy.roots, the three addends against the
pinned torque rows, where one stretch by the predicted factor lands, the struct layout and the exported symbols."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import helpers
import invdyn_reference as ir
import stretch_reference as sr
import tscale_reference as tr
from audit_reference import audit_path
from batotp_amd import capi
from test_gpu_invdyn import model_named

ROOT = helpers.ROOT


def naive_record(A, B, G, hi, lo):
    """the definition point by point, in Python floats (binary64)"""
    nl, n = G.shape
    best, n_static = (math.inf, -1, -1, 0), 0
    for i in range(n):
        g = [float(G[j, i]) for j in range(nl)]
        if any(not (g[j] - float(hi[j]) < 0.0 and float(lo[j]) - g[j] < 0.0) for j in range(nl)):
            n_static += 1
            continue
        for j in range(nl):
            a0, b0 = float(A[j, i]), float(B[j, i])
            for side, (a, b, c) in ((1, (a0, b0, g[j] - float(hi[j]))), (-1, (-a0, -b0, float(lo[j]) - g[j]))):
                disc = b * b - (4.0 * a) * c
                if not disc >= 0.0:
                    continue
                q = b + math.sqrt(disc)
                if not (q > 0.0 and math.isfinite(q)):
                    continue
                x = (2.0 * (-c)) / q
                if math.isfinite(x) and x < best[0]:        # strictly: the first in the order point, joint, upper side wins a tie
                    best = (x, i, j, side)
    return best + (n_static,)


@pytest.mark.parametrize("name", ["kuka", "one"])
def test_numpy_reference_equals_a_naive_loop(oracle_lib, name):
    model = model_named(oracle_lib, name)
    nl = model.n_links
    rows = tr.synth_rows(model, [0, 1, 2, 3, 40, 131], [1.0, 1.0, 1.0, 2.0, 3.0, 2.5])
    sres = tr.synth_steps(len(rows))
    P = [tr.pieces(oracle_lib, model, r, sres[k]) for k, r in enumerate(rows)]
    gmax = np.max([np.abs(G).max(axis=1) for A, B, G in P if G.shape[1]], axis=0)
    seen_static = seen_root = seen_none = False
    for scale in (0.9, 1.2, 40.0):           # gravity outside the range at some points; a range that binds; one that hardly does
        prob = capi.make_problem(nl, 0, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0] * nl, jnt_trq_max=[float(v) for v in scale * gmax + 1e-3],
                                 jnt_trq_min=[float(v) for v in -0.7 * (scale * gmax + 1e-3)])
        for target in (1.0, 0.8):
            hi, lo = tr.bounds(prob, nl, target)
            for k, (A, B, G) in enumerate(P):
                rec, want = tr.scale_record(A, B, G, hi, lo), naive_record(A, B, G, hi, lo)
                got = (float(rec["s"]), int(rec["at"]), int(rec["row"]), int(rec["side"]), int(rec["n_static"]))
                assert got == want and int(rec["reserved"]) == 0, (name, scale, target, k, got, want)
                seen_static |= want[4] > 0
                seen_root |= want[1] >= 0
                seen_none |= want[1] < 0 and G.shape[1] >= 3
    assert seen_static and seen_root and (seen_none or name == "one")
    # fewer than three points: A = B = 0 and no candidate
    for k in (1, 2):
        A, B, G = P[k]
        assert not A.any() and not B.any()


def test_the_root_rule_against_numpy_roots():
    rng = np.random.default_rng(17)
    seen = dict.fromkeys(("a>0", "a=0,b>0", "a=0,b<=0", "a<0,disc<0", "a<0,b<=0", "a<0,two roots"), 0)
    for trial in range(4000):
        a, b = rng.choice([0.0, 1.0, -1.0]) * 10.0 ** rng.uniform(-3, 3), rng.choice([0.0, 1.0, -1.0]) * 10.0 ** rng.uniform(-3, 3)
        c = -10.0 ** rng.uniform(-3, 3)
        x, e = tr.roots(np.array([a]), np.array([b]), np.array([c]))
        x, e = float(x[0]), bool(e[0])
        if a == 0.0:
            pos = [-c / b] if b > 0.0 else []
            seen["a=0,b>0" if b > 0.0 else "a=0,b<=0"] += 1
        else:
            disc = b * b - 4.0 * a * c
            if abs(disc) <= 1e-9 * (b * b + abs(4.0 * a * c)):
                continue                                    # a double root within rounding: either answer is right
            r = np.roots([a, b, c])
            pos = sorted(float(v.real) for v in r if abs(v.imag) == 0.0 and v.real > 0.0) if disc > 0.0 else []
            key = "a>0" if a > 0.0 else ("a<0,disc<0" if disc < 0.0 else ("a<0,b<=0" if b <= 0.0 else "a<0,two roots"))
            seen[key] += 1
        assert e == bool(pos), (a, b, c, x, e, pos)
        if pos:
            # two sources of error, both a few ulp times a condition number.  numpy.roots goes through the eigenvalues of the
            # companion matrix: a few ulp of the LARGER root's scale, so the smaller root of a pair carries eps * (large / small).
            # The rule itself: b*b, 4ac, their difference, the root and the sum q = b + sqrt(disc) each round once, an absolute
            # error of a few eps * (|b| + sqrt(disc)) in q -- for b < 0 the sum cancels and x = 2(-c)/q carries that over q.
            eps = np.finfo(float).eps
            if a != 0.0:
                sq = math.sqrt(disc)
                tol = 64 * eps * max(1.0, max(abs(v) for v in np.roots([a, b, c])) / pos[0]) + 8 * eps * (abs(b) + sq) / (b + sq)
            else:
                tol = 4 * eps
            assert abs(x - pos[0]) <= tol * pos[0], (a, b, c, x, pos)
    assert all(v >= 20 for v in seen.values()), seen


@pytest.mark.parametrize("name", ["kuka", "rr", "random8", "one"])
def test_the_addends_sum_to_the_pinned_torque_rows(oracle_lib, name):
    model = model_named(oracle_lib, name)
    rows = tr.synth_rows(model, [0, 1, 2, 3, 50], [1.0, 1.0, 1.0, 1.0, 2.0])
    sres = tr.synth_steps(len(rows))
    for k, r in enumerate(rows):
        A, B, G = tr.pieces(oracle_lib, model, r, sres[k])
        with np.errstate(all="ignore"):
            ir.assert_rows_bit_equal((A + B) + G, ir.torque_rows(oracle_lib, model, r, sres[k]), f"{name}, path {k}")
    prob = tr.synth_problem(oracle_lib, model, tr.synth_rows(model), tr.synth_steps(len(tr.SYNTH_LENGTHS)))
    got, rec = tr.torque_scale(oracle_lib, model, rows, sres, prob)
    for g, w in zip(got, ir.with_torques(oracle_lib, model, rows, sres)):
        ir.assert_rows_bit_equal(g, w, name)


@pytest.mark.parametrize("name", ["kuka", "one"])
def test_one_stretch_by_the_predicted_factor_lands_near_the_target(oracle_lib, name):
    model = model_named(oracle_lib, name)
    nl = model.n_links
    rows, sres = tr.synth_rows(model), tr.synth_steps(len(tr.SYNTH_LENGTHS))
    prob = tr.synth_problem(oracle_lib, model, rows, sres)
    probT = tr.with_trq_on(prob)
    hi, lo = tr.bounds(prob, nl, 1.0)
    done = 0
    for k in (3, 5, 7):                                   # the smooth paths that move fast
        w, rec = tr.path_with_torques(oracle_lib, model, rows[k], sres[k], hi, lo)
        before = float(audit_path(w, sres[k], nl, 0, nl, probT, 0.0)["fam"][capi.AUDIT_TRQ]["peak"])
        s = float(rec["s"])
        if not (before > 1.0 and s < 1.0 and int(rec["n_static"]) == 0):
            continue
        m = rows[k].shape[1] - 1
        n2 = int(math.ceil(m / s)) + 1
        w2, rec2 = tr.path_with_torques(oracle_lib, model, sr.stretch_rows(rows[k], n2), sres[k], hi, lo)
        after = float(audit_path(w2, sres[k], nl, 0, nl, probT, 0.0)["fam"][capi.AUDIT_TRQ]["peak"])
        print(f"TSCALE reference {name} path {k}: s {s:.6f}, {m + 1} -> {n2} points, TRQ peak {before:.6f} -> {after:.6f} (after / target = {after:.6f}), "
              f"s of the result {float(rec2['s']):.6f}")
        assert after < before
        done += 1
    assert done >= 1


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of batotp_path_tscale as the system compiler lays it out = capi.PathTscale and capi.TSCALE_DTYPE"""
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "batotp_hip_tscale.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(batotp_path_tscale), offsetof(batotp_path_tscale, s),\n'
        "         offsetof(batotp_path_tscale, at), offsetof(batotp_path_tscale, row), offsetof(batotp_path_tscale, side),\n"
        "         offsetof(batotp_path_tscale, n_static), offsetof(batotp_path_tscale, reserved), BATOTP_TSCALE_BLOCK_POINTS,\n"
        "         BATOTP_STRETCH_STATIC, BATOTP_INVDYN_BLOCK_POINTS);\n"
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    PT = capi.PathTscale
    want = [C.sizeof(PT), PT.s.offset, PT.at.offset, PT.row.offset, PT.side.offset, PT.n_static.offset, PT.reserved.offset, capi.TSCALE_BLOCK_POINTS,
            capi.STRETCH_STATIC, capi.INVDYN_BLOCK_POINTS]
    assert got == want
    assert got[:7] == [40, 0, 8, 16, 20, 24, 32] and got[7:9] == [128, 3]
    d = capi.TSCALE_DTYPE
    assert d.itemsize == 40 and [d.fields[f][1] for f in ("s", "at", "row", "side", "n_static", "reserved")] == got[1:7]
    assert capi.STRETCH_STATIC not in (capi.STRETCH_PASSES, capi.STRETCH_ROUNDS, capi.STRETCH_CAPPED)


TSCALE_SYMBOLS = ["batotp_hip_output_torque_scale", "batotp_hip_output_stretch_torques", "batotp_hip_output_tscale_ms", "batotp_hip_output_tscale_ranges"]


def test_product_library_exports_the_torque_scale(hip_lib):
    assert hip_lib.has_tscale
    assert hip_lib.tscale_symbols == sorted(TSCALE_SYMBOLS)
    for name in TSCALE_SYMBOLS:
        assert hasattr(hip_lib.lib, name), name
        assert name not in hip_lib.symbols      # `symbols` stays the table of include/batotp_hip.h
    new = open(os.path.join(ROOT, "include", "batotp_hip_tscale.h")).read()
    assert '#include "batotp_hip_stretch.h"' in new and '#include "batotp_hip_invdyn.h"' in new
    for name in TSCALE_SYMBOLS:
        assert f"int {name}(" in new
    for other in ("batotp_hip.h", "batotp_hip_audit.h", "batotp_hip_invdyn.h", "batotp_hip_stretch.h"):
        assert "tscale" not in open(os.path.join(ROOT, "include", other)).read()


def test_checker_has_no_torque_scale_and_says_so(oracle_lib, oracle_ctx):
    assert oracle_lib.has_tscale is False
    for name in TSCALE_SYMBOLS:
        assert not hasattr(oracle_lib.lib, name)
    case = helpers.Case("synth_gen7dof_s0")
    out, b = helpers.run_to_output(oracle_ctx, [case])
    model = oracle_lib.builtin_serial_model(capi.ROBOT_KUKA)
    for call in (lambda: out.torque_scale(case.problem, model), lambda: out.stretch_torques(case.problem, model), out.tscale_ms, out.tscale_ranges):
        with pytest.raises(capi.BatotpError, match="torque-scale entry points"):
            call()
    out.close(); b.close()
