"""CPU (-m "not gpu"): the continuous torque rating of finished trajectories (include/batotp_hip_duty.h) as far as it goes without a
device -- the numpy tree against a loop that adds one by one, its distance from the exact sum, the quartic against the direct sum,
the bisection against numpy.roots, where the predicted factor lands, the struct layouts, the exported symbols, and the host rule and
the round decision as plain C++ (batotp_amd/csrc/duty_rounds.h, stretch_rounds.h) against the numpy reference."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import duty_reference as du
import helpers
import stretch_reference as sr
import tscale_reference as tr
from batotp_amd import capi
from test_gpu_invdyn import model_named

ROOT = helpers.ROOT
BP = capi.DUTY_BLOCK_POINTS
U = 2.0 ** -53          # unit roundoff of binary64
EDGES = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 3 * 128 + 5]


def naive_tree(v):
    """the additions of the definition one by one, in Python floats (binary64)"""
    v = [float(x) for x in v]
    if not v:
        return 0.0
    total = None
    for b in range(0, len(v), BP):
        waves = []
        for w in (0, 1):
            lane = [v[b + 64 * w + l] if b + 64 * w + l < len(v) else 0.0 for l in range(64)]
            for d in (32, 16, 8, 4, 2, 1):
                for l in range(d):
                    lane[l] = lane[l] + lane[l + d]
            waves.append(lane[0])
        block = waves[0] + waves[1]
        total = block if total is None else total + block
    return total


def test_block_points():
    assert BP == 128 == capi.TSCALE_BLOCK_POINTS == capi.INVDYN_BLOCK_POINTS


@pytest.mark.parametrize("n", EDGES)
def test_the_numpy_tree_equals_a_naive_loop(n):
    rng = np.random.default_rng(100 + n)
    v = rng.standard_normal((3, n)) * 10.0 ** rng.uniform(-6, 6, (3, n))
    got = du.tree_sum(v)
    assert got.shape == (3,)
    for r in range(3):
        assert got[r].tobytes() == np.float64(naive_tree(v[r])).tobytes(), (n, r)
    if n:
        minus = du.tree_sum(np.full(n, -0.0))
        # padded lanes contribute +0.0: only a path that fills its blocks keeps the sign
        assert minus == 0.0 and bool(np.signbit(minus)) == (n % BP == 0), n
    else:
        assert du.tree_sum(np.zeros(0)).tobytes() == np.float64(0.0).tobytes()


@pytest.mark.parametrize("n", [n for n in EDGES if n])
def test_the_tree_is_a_few_ulps_from_the_exact_sum(n):
    """every value passes through at most 6 additions in its wavefront, 1 in its block and nb - 1 along the path: the error is within
    (6 + nb) u of the sum of absolute values, plus the rounding of the exact sum itself"""
    rng = np.random.default_rng(200 + n)
    v = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    nb = -(-n // BP)
    err = abs(float(du.tree_sum(v)) - math.fsum(v))
    bound = (6 + nb + 1) * U * math.fsum(np.abs(v))
    print(f"DUTY tree n {n}: |tree - fsum| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


_SYNTH = {}


def synth(oracle_lib, name):
    if name not in _SYNTH:
        model = model_named(oracle_lib, name)
        rows = tr.synth_rows(model)
        sres = tr.synth_steps(len(rows))
        P = [tr.pieces(oracle_lib, model, r, sres[k]) for k, r in enumerate(rows)]
        V = [du.point_values(oracle_lib, model, r, sres[k], P[k]) for k, r in enumerate(rows)]
        S = [du.sums_record(m, p) for m, p, tau in V]
        _SYNTH[name] = (model, rows, sres, P, V, S)
    return _SYNTH[name]


@pytest.mark.parametrize("name", ["kuka", "one"])
def test_s6_is_the_quartic_at_one(oracle_lib, name):
    """S6 = sum tau^2 and P(1) = S0 + 2 S1 + S2 + 2 S3 + 2 S4 + S5 are the same sum over (A + B + G)^2 term by term.  With
    T = sum (|A| + |B| + |G|)^2: tau carries 2 u of |A| + |B| + |G|, so tau^2 about 5 u of its term; each product of P carries u;
    either sum adds (6 + nb) u; the Horner form adds 8 u: well within (2 (6 + nb) + 24) u T"""
    model, rows, sres, P, V, S = synth(oracle_lib, name)
    for k, (A, B, G) in enumerate(P):
        n = G.shape[1]
        if n == 0:
            continue
        nb = -(-n // BP)
        T = ((np.abs(A) + np.abs(B) + np.abs(G)) ** 2).sum(axis=1)
        for j in range(model.n_links):
            c = du.coefficients(S[k]["S"][j])
            p1 = float(du.quartic(c, np.float64(1.0)))
            s6 = float(S[k]["S"][j][6])
            assert abs(p1 - s6) <= (2 * (6 + nb) + 24) * U * float(T[j]), (name, k, j, p1, s6)


def test_the_bisection_against_numpy_roots():
    rng = np.random.default_rng(29)
    done = 0
    for trial in range(600):
        n = int(rng.integers(3, 200))
        A, B, G = (rng.standard_normal(n) * 10.0 ** rng.uniform(-1, 1) for _ in range(3))
        S = [float(v) for v in (np.sum(A * A), np.sum(A * B), np.sum(B * B), np.sum(A * G), np.sum(B * G), np.sum(G * G))]
        c = du.coefficients(S + [0.0])
        c0, p1 = float(c[4]), float(du.quartic(c, np.float64(1.0)))
        if not c0 < p1:
            continue
        L = np.float64(c0 + rng.uniform(0.05, 0.95) * (p1 - c0))
        assert c0 < L < p1
        lo = float(du.bisect(c, L))
        poly = [float(v) for v in c]
        poly[4] -= float(L)
        r = np.roots(poly)
        real = sorted(float(z.real) for z in r if abs(z.imag) <= 1e-9 * max(1.0, abs(z)) and 0.0 < z.real < 1.0)
        assert real, (poly, lo)
        d = np.polyder(np.poly1d(poly))
        near = min(real, key=lambda z: abs(z - lo))
        slope = abs(float(d(near)))
        scale = sum(abs(v) for v in poly)
        if slope < 1e-3 * scale:
            continue                    # a root that is nearly double: its place is not determined to rounding
        # the rule itself, sharply: 64 halvings of [0, 1] end at neighbouring numbers (above 2^-10 an ulp is no smaller than 2^-64) on
        # either side of a crossing of the COMPUTED quartic
        assert float(du.quartic(c, np.float64(lo))) <= L
        if lo > 2.0 ** -10:
            assert float(du.quartic(c, np.nextafter(np.float64(lo), np.float64(1.0)))) > L, (poly, lo)
        # against numpy.roots: the computed quartic is within 8 u * scale of the exact one, which moves the crossing by that over the
        # slope; numpy.roots goes through the eigenvalues of the companion matrix and carries some 1e3 u of its scale over the same slope
        assert abs(lo - near) <= 2.0e3 * U * scale / slope, (poly, lo, real)
        done += 1
    assert done >= 300, done


WIDE = dict(jnt_vel_max=1e9, jnt_acc_max=1e9, trq=1e12)


def wide_problem(nl):
    """limits that never bind: the RMS family alone drives the rounds"""
    return capi.make_problem(nl, 0, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON, jnt_vel_max=[WIDE["jnt_vel_max"]] * nl, jnt_acc_max=[WIDE["jnt_acc_max"]] * nl,
                             jnt_trq_max=[WIDE["trq"]] * nl, jnt_trq_min=[-WIDE["trq"]] * nl)


def ratings_for(S, nl, over=1.58):
    """ratings a path exceeds by `over` on its joints that move, and that gravity alone stays inside by a quarter on the others"""
    n = float(S["n_pts"])
    rms = np.sqrt(S["S"][:nl, 6] / n)
    grav = np.sqrt(S["S"][:nl, 5] / n)
    return np.maximum(np.maximum(rms / over, 1.25 * grav), 1e-6)


def test_one_stretch_by_the_predicted_factor_lands_near_the_target(oracle_lib):
    model, rows, sres, P, V, S = synth(oracle_lib, "kuka")
    nl = model.n_links
    prob = wide_problem(nl)
    stretched = 0
    for k in (3, 5, 7, 8):
        rated = ratings_for(S[k], nl)
        d0 = du.duty_record(S[k], nl, rated, 1.0, sres[k])
        if float(d0["util"]) > 1.0 and int(d0["n_hold"]) == 0:
            n2 = int(math.ceil((rows[k].shape[1] - 1) / float(d0["s"]))) + 1
            w, s1 = du.path_duty(oracle_lib, model, sr.stretch_rows(rows[k], n2), sres[k])
            d1 = du.duty_record(s1, nl, rated, 1.0, sres[k])
            print(f"DUTY reference kuka path {k}: util {float(d0['util']):.5f} (joint {int(d0['row'])}), s {float(d0['s']):.6f} (joint {int(d0['s_row'])}), "
                  f"{rows[k].shape[1]} -> {n2} points, landing util {float(d1['util']):.5f}")
            assert float(d1["util"]) < float(d0["util"])
            stretched += 1
        out, report, final, recs, duties = du.stretch_duty(oracle_lib, model, [rows[k]], [sres[k]], 0, prob, rated, 1.0, 8, 16.0)
        print(f"DUTY reference kuka path {k}: rounds {int(report[0]['rounds'])}, status {int(report[0]['status'])}, final util {float(duties[0]['util']):.5f}")
        assert int(report[0]["status"]) == capi.STRETCH_PASSES and int(report[0]["rounds"]) <= 3, (k, report[0])
        assert float(duties[0]["util"]) <= 1.0
    assert stretched >= 2


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two records as the system compiler lays them out = capi.PathDuty, capi.PathDutySums and the dtypes"""
    duty_f = ["rms", "util", "row", "n_hold", "s", "s_row", "reserved", "energy", "peak_power", "power_at", "n_pts"]
    sums_f = ["S", "W", "peak_power", "power_at", "n_pts"]
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "batotp_hip_duty.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %d %d", sizeof(batotp_path_duty), sizeof(batotp_path_duty_sums), BATOTP_DUTY_BLOCK_POINTS, BATOTP_MAX_LINKS);\n'
        + "".join(f'  printf(" %zu", offsetof(batotp_path_duty, {f}));\n' for f in duty_f)
        + "".join(f'  printf(" %zu", offsetof(batotp_path_duty_sums, {f}));\n' for f in sums_f)
        + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    PD, PS = capi.PathDuty, capi.PathDutySums
    want = [C.sizeof(PD), C.sizeof(PS), capi.DUTY_BLOCK_POINTS, capi.MAX_LINKS] + [getattr(PD, f).offset for f in duty_f] + [getattr(PS, f).offset for f in sums_f]
    assert got == want
    assert got[:4] == [128, 480, 128, 8]
    assert [capi.DUTY_DTYPE.fields[f][1] for f in duty_f] == got[4:4 + len(duty_f)] and capi.DUTY_DTYPE.itemsize == 128
    assert [capi.DUTY_SUMS_DTYPE.fields[f][1] for f in sums_f] == got[4 + len(duty_f):] and capi.DUTY_SUMS_DTYPE.itemsize == 480
    assert capi.DUTY_SUMS_DTYPE.fields["W"][1] == 8 * 7 * capi.MAX_LINKS      # quantity q is the q-th double of the record


DUTY_SYMBOLS = ["batotp_hip_output_duty", "batotp_hip_output_stretch_duty", "batotp_hip_output_duty_ms", "batotp_hip_output_duty_ranges"]


def test_product_library_exports_the_duty_entry_points(hip_lib):
    assert hip_lib.has_duty
    assert hip_lib.duty_symbols == sorted(DUTY_SYMBOLS)
    for name in DUTY_SYMBOLS:
        assert hasattr(hip_lib.lib, name), name
        assert name not in hip_lib.symbols      # `symbols` stays the table of include/batotp_hip.h
    new = open(os.path.join(ROOT, "include", "batotp_hip_duty.h")).read()
    assert '#include "batotp_hip_tscale.h"' in new
    for name in DUTY_SYMBOLS:
        assert f"int {name}(" in new
    for other in ("batotp_hip.h", "batotp_hip_audit.h", "batotp_hip_invdyn.h", "batotp_hip_stretch.h", "batotp_hip_tscale.h"):
        assert "duty" not in open(os.path.join(ROOT, "include", other)).read()


def test_checker_has_no_duty_and_says_so(oracle_lib, oracle_ctx):
    assert oracle_lib.has_duty is False
    for name in DUTY_SYMBOLS:
        assert not hasattr(oracle_lib.lib, name)
    case = helpers.Case("synth_gen7dof_s0")
    out, b = helpers.run_to_output(oracle_ctx, [case])
    model = oracle_lib.builtin_serial_model(capi.ROBOT_KUKA)
    rated = [1.0] * model.n_links
    for call in (lambda: out.duty(model, rated), lambda: out.stretch_duty(case.problem, model, rated), out.duty_ms, out.duty_ranges):
        with pytest.raises(capi.BatotpError, match="duty entry points"):
            call()
    out.close(); b.close()


# ---- the host rule and the decision as plain C++ ---------------------------------------------------------------------------
DRIVER = os.path.join(ROOT, "tests", "drivers", "duty_plan_main.cpp")
INCLUDES = [f"-I{ROOT}/include", f"-I{ROOT}/batotp_amd/csrc"]


def build_driver(where, extra=()):
    exe = where / "duty_plan"
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", *extra, *INCLUDES, DRIVER, "-o", str(exe)], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, r = build_driver(tmp_path_factory.mktemp("duty_plan"))
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def hexf(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else v.hex()))


def records_case(where, S_list, sres, nl, rated, target):
    case = where / f"records_{nl}_{target}.txt"
    lines = [f"{nl} {hexf(target)}", " ".join(hexf(v) for v in rated)]
    for S, h in zip(S_list, sres):
        lines.append(" ".join([hexf(h)] + [hexf(v) for v in S["S"].ravel()] + [hexf(S["W"]), hexf(S["peak_power"]), str(int(S["power_at"])), str(int(S["n_pts"]))]))
    case.write_text("\n".join(lines) + "\n")
    return case


def check_records(exe, case, want):
    r = subprocess.run([exe, "records", str(case)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == len(want)
    got = np.zeros(len(want), dtype=capi.DUTY_DTYPE)
    for k, w in enumerate(lines):
        assert w[0] == "duty" and int(w[1]) == k
        f = w[2:]
        got[k]["rms"] = [float.fromhex(v) if v not in ("nan", "-nan") else math.nan for v in f[:8]]
        rest = f[8:]
        val = lambda v: math.nan if "nan" in v else float.fromhex(v)      # noqa: E731
        got[k]["util"], got[k]["row"], got[k]["n_hold"], got[k]["s"], got[k]["s_row"] = val(rest[0]), int(rest[1]), int(rest[2]), val(rest[3]), int(rest[4])
        got[k]["energy"], got[k]["peak_power"], got[k]["power_at"], got[k]["n_pts"] = val(rest[5]), val(rest[6]), int(rest[7]), int(rest[8])
    du.assert_duty_equal(got, want, str(case))


@pytest.mark.parametrize("name", ["kuka", "one"])
def test_the_host_rule_in_cpp_is_the_numpy_rule(driver, oracle_lib, tmp_path, name):
    model, rows, sres, P, V, S = synth(oracle_lib, name)
    nl = model.n_links
    base = ratings_for(S[3], nl)
    seen_hold = seen_s = seen_pass = False
    for scale, target in ((1.0, 1.0), (1.0, 0.6), (0.3, 1.0), (50.0, 1.0)):
        rated = base * scale
        want = np.zeros(len(S), dtype=capi.DUTY_DTYPE)
        for k in range(len(S)):
            want[k] = du.duty_record(S[k], nl, rated, target, sres[k])
        check_records(driver, records_case(tmp_path, S, sres, nl, rated, target), want)
        seen_hold |= bool(want["n_hold"].any())
        seen_s |= bool(np.isfinite(want["s"]).any())
        seen_pass |= bool(((want["util"] >= 0) & (want["util"] <= target)).any())
    assert seen_hold and seen_pass and (seen_s or nl == 1)      # the single link carries its weight: gravity outweighs its motion on every path
    # values that are not finite: a NaN moment gives a NaN rms that takes no part in util, an Inf likewise
    bad = np.array([S[3], S[3], S[0]])
    bad[0]["S"][0] = np.nan
    bad[1]["S"][nl - 1, 6] = np.inf
    bad[2]["W"] = np.nan
    want = np.zeros(3, dtype=capi.DUTY_DTYPE)
    for k in range(3):
        want[k] = du.duty_record(bad[k], nl, base, 1.0, sres[k])
    assert np.isnan(want[0]["rms"][0]) and (nl == 1) == (int(want[0]["row"]) == -1) and np.isnan(want[2]["energy"])
    check_records(driver, records_case(tmp_path, bad, sres[:3], nl, base, 0.5), np.array([du.duty_record(bad[k], nl, base, 0.5, sres[k]) for k in range(3)]))


def rounds_case_and_report(oracle_lib, args, hold):
    """the shared synthetic batch with ratings from its own sums: paths over their rating, paths inside it and, with hold, one joint
    of the KUKA whose gravity torque alone reaches its rating"""
    model, rows, sres, P, V, S = synth(oracle_lib, "kuka")
    nl = model.n_links
    rated = ratings_for(S[3], nl, 1.3)
    if hold:
        rated[1] = 0.5 * math.sqrt(float(S[8]["S"][1, 5]) / float(S[8]["n_pts"]))
    prob = tr.synth_problem(oracle_lib, model, rows, sres)
    trace = []
    report = du.stretch_duty(oracle_lib, model, rows, sres, 0, prob, rated, *args, trace=trace)[1]
    return rows, trace, report


@pytest.mark.parametrize("hold", [False, True], ids=["plain", "hold"])
@pytest.mark.parametrize("args", [(1.0, 8, 16.0), (0.8, 8, 1.75), (1.0, 1, 16.0)], ids=["plain", "cap", "one_round"])
def test_the_round_decision_in_cpp_is_the_numpy_rounds(driver, oracle_lib, tmp_path, args, hold):
    rows, trace, report = rounds_case_and_report(oracle_lib, args, hold)
    K = len(rows)
    if hold:
        assert capi.STRETCH_STATIC in [int(v) for v in report["status"]] or args != (1.0, 8, 16.0)
    lines = [f"{hexf(args[0])} {args[1]} {hexf(args[2])} {K}", " ".join(str(r.shape[1]) for r in rows)]
    for aud, scale, duty, n2, rounds, status in trace:
        for k in range(K):
            lines.append(" ".join([hexf(aud[k]["fam"][f]["peak"]) for f in range(5)] + [hexf(scale[k]["s"]), str(int(scale[k]["n_static"])),
                                  hexf(duty[k]["util"]), str(int(duty[k]["n_hold"])), hexf(duty[k]["s"])]))
    case = tmp_path / "rounds.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "rounds", str(case)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln.split() for ln in r.stdout.splitlines()]
    at = 0
    for rnd, (aud, scale, duty, n2, rounds, status) in enumerate(trace):
        assert out[at][0] == "round" and (out[at][1] == "1") == (rnd + 1 < len(trace)), rnd
        at += 1
        for k in range(K):
            w = out[at + k]
            assert (w[0], int(w[1]), int(w[2]), int(w[3]), int(w[4])) == ("path", k, n2[k], rounds[k], status[k]), (rnd, k, w)
        at += K
    for k in range(K):
        w = out[at + k]
        assert w[0] == "report" and [int(w[1]), int(w[2]), int(w[3]), int(w[5]), int(w[6])] == [k, int(report[k]["n_in"]), int(report[k]["n_out"]),
                                                                                                 int(report[k]["rounds"]), int(report[k]["status"])]
        assert np.float64(float.fromhex(w[4])).tobytes() == report[k]["factor"].tobytes()
    assert at + K == len(out)


def test_the_driver_under_the_host_sanitizers(oracle_lib, tmp_path):
    """the stand-alone program alone, where the toolchain has the runtime: nothing that is loaded into Python runs under a sanitizer"""
    exe, r = build_driver(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr[-2000:]
        print("DUTY: no sanitizer runtime in this toolchain; the plain build is what the other tests ran")
        return
    model, rows, sres, P, V, S = synth(oracle_lib, "kuka")
    nl = model.n_links
    rated = ratings_for(S[3], nl)
    want = np.array([du.duty_record(S[k], nl, rated, 1.0, sres[k]) for k in range(len(S))])
    check_records(str(exe), records_case(tmp_path, S, sres, nl, rated, 1.0), want)
