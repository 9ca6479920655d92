"""The host-side plan of the output stage (batotp_amd/csrc/output_plan.h) without a GPU: tests/drivers/output_plan_main.cpp
includes that header alone, reads result rows, steps and parameters from a file and prints the plan and, per chunk and route,
the layout of the launch sequences.

a. against the CPU checker, which computes point counts and sres on its own (oracle/batotp_oracle_output.c): ==
b. rows made up here: paths without a trajectory keep their place, the short curve's time step is t_total / 3
c. invariants of the chunk cuts and of the layout of every route, for three budgets
d. the same cases through a build of the driver with the address and undefined-behaviour sanitizers"""
import math
import os
import subprocess

import numpy as np
import pytest

import helpers
from helpers import output_params
from batotp_amd import capi
from test_gpu_output_steps import CORE_FACTORS, Expected, core_inputs, reinterpolated, swept_batch

DRIVER = os.path.join(helpers.ROOT, "tests", "drivers", "output_plan_main.cpp")
INCLUDES = [f"-I{helpers.ROOT}/batotp_amd/csrc", f"-I{helpers.ROOT}/include"]
SANITIZE = "-fsanitize=address,undefined"
HUGE = float(1 << 40)
# (out_res / h, smoothing factor): the settings of tests/test_gpu_output_steps.py on its core batch
CORE_GRID = ((1.1, 1.0), (1.1, 5.0), (1.1, 1.6), (1.1, 9.0), (3.0, 1.0), (3.0, 5.0), (0.3, 1.0), (0.3, 5.0))


def compile_driver(exe, extra=()):
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", *extra, *INCLUDES, DRIVER, "-o", str(exe)]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("output_plan") / "output_plan_main"
    r = compile_driver(exe)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


class PlanCase:
    """one input of the driver.  rows: (n_fwd, t_total, status_rev, status_fwd) per path; R = 7, no torque step, no pose is what the
    device works with on the core batch (seven joint rows), and only the scratch estimate reads them"""

    def __init__(self, rows, steps, out_res, smooth, budget=HUGE, R=7, torque_step=False, pose=False, path0=0):
        assert len(rows) == len(steps)
        self.rows, self.steps, self.out_res, self.smooth, self.budget, self.path0 = list(rows), list(steps), out_res, smooth, budget, path0
        self.R, self.torque_step, self.pose = R, torque_step, pose

    @staticmethod
    def of_results(res, steps, *a, **kw):
        """from the result rows of a swept batch (capi.RESULT_DTYPE)"""
        rows = [(int(r["n_fwd"]), float(r["t_total"]), int(r["status_rev"]), int(r["status_fwd"])) for r in res]
        return PlanCase(rows, steps, *a, **kw)

    def text(self):
        fl = lambda v: "nan" if math.isnan(v) else float(v).hex()
        head = [len(self.rows), self.path0, fl(self.out_res), fl(self.smooth), self.R, int(self.torque_step), int(self.pose), fl(self.budget)]
        lines = [" ".join(str(v) for v in head)]
        lines += [f"{n} {fl(t)} {sr} {sf} {fl(h)}" for (n, t, sr, sf), h in zip(self.rows, self.steps)]
        return "\n".join(lines) + "\n"


ALL_CASES = []   # every case a test of this module ran, in order: the sanitizer build repeats them


def run_driver(exe, case, where):
    path = os.path.join(str(where), "case.txt")
    with open(path, "w") as f:
        f.write(case.text())
    r = subprocess.run([str(exe), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def parse(out):
    """paths: dicts per path; chunks: [(ka, kb, staged, {route: (totals, [path dicts])})]"""
    plan = {"paths": [], "chunks": []}
    for ln in out.splitlines():
        w = ln.split()
        if w[0] == "path":
            ints = [int(v) for v in w[1:4] + w[5:10] + w[12:14]]
            plan["paths"].append(dict(zip(("k", "n", "off", "nFwd", "n1", "n2", "nF", "window", "route", "need"), ints),
                                      sres=float.fromhex(w[4]), tStep=float.fromhex(w[10]), vfactT=float.fromhex(w[11])))
        elif w[0] == "plan":
            plan["totF"], plan["mixed"], plan["maxChunk"] = int(w[1]), bool(int(w[2])), int(w[3])
        elif w[0] == "cuts":
            plan["cuts"] = [int(v) for v in w[1:]]
        elif w[0] == "chunk":
            plan["chunks"].append((int(w[1]), int(w[2]), bool(int(w[3])), {}))
        elif w[0] == "route":
            plan["chunks"][-1][3][int(w[1])] = (dict(zip(("Kc", "t1", "t2", "tS", "tF"), (int(v) for v in w[2:]))), [])
            last = plan["chunks"][-1][3][int(w[1])][1]
        elif w[0] == "at":
            last.append(dict(zip(("p", "off1", "off2", "offS", "offF", "offD", "n1", "n2", "nFwd", "nF"), (int(v) for v in w[1:]))))
        else:
            raise AssertionError(ln)
    return plan


def plan_of(exe, case, where):
    ALL_CASES.append(case)
    return parse(run_driver(exe, case, where))


def routes_live(plan):
    return {p["route"] for p in plan["paths"] if p["n"]}


# ---- a: against the checker ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core(oracle_ctx):
    """the five-path core batch of tests/test_gpu_output_steps.py, swept by the checker"""
    case, h, ys, steps = core_inputs()
    ob = swept_batch(oracle_ctx, case.problem, ys, case.sres, steps, 3 * case.max_steps())
    yield Expected(ob, output_params(case.name), steps), ob.results(), h
    ob.close()


def test_counts_and_sres_equal_the_checkers(driver, core, tmp_path):
    exp, res, h = core
    assert exp.steps == [h * f for f in CORE_FACTORS]
    seen, together = set(), 0
    for f, smooth in CORE_GRID:
        out_res = f * h
        plan = plan_of(driver, PlanCase.of_results(res, exp.steps, out_res, smooth), tmp_path)
        want = exp.get(out_res, smooth)
        for k, (n, sres, rows) in enumerate(want):
            tag = f"out_res={f} h smooth={smooth} path {k}"
            assert n >= 4, tag
            assert plan["paths"][k]["n"] == n == rows.shape[1], tag
            assert plan["paths"][k]["sres"] == sres, tag
        assert plan["totF"] == sum(n for n, _, _ in want)
        live = routes_live(plan)
        # a path is re-interpolated where out_res < its step (bit 1 of the route), smoothed where the factor exceeds 1.5 (bit 0)
        assert live == {(2 if r else 0) | (1 if smooth > 1.5 else 0) for r in reinterpolated(exp.steps, out_res)}
        assert plan["mixed"] == (len(live) > 1)
        seen |= live
        together = max(together, len(live))
    # The grid takes every route.  Two are the most one range can hold: the smoothing factor of a re-interpolated path is the
    # call's times max(out_res / step, 1), and such a path has out_res < step, so smoothed or not is the same for every path
    assert seen == {0, 1, 2, 3} and together == 2


# ---- b: rows made up here -----------------------------------------------------------------------------------------------
def test_failed_paths_keep_their_place_and_the_short_curve_its_time_step(driver, tmp_path):
    h = 0.001
    good = (1000, 0.999, 0, 0)
    rows = [good,
            (3, 0.002, 0, 0),                          # n_fwd < 4
            good,
            (1000, 0.999, capi.ST_MAX_INTEG_TIME, 0),
            (1000, 0.999, 0, capi.ST_CAPACITY),
            (1000, 0.999, capi.ST_NONFINITE, 0),
            (4, 0.75, 0, capi.ST_SHORT),               # the short curve: four points over t_total
            good,                                      # ... with a NaN step
            (1000, 0.999, 0, capi.ST_BISECT_FAIL | capi.ST_SEG_ERROR),   # these two bits disqualify nobody
            good]
    steps = [h, h, 2 * h, h, h, h, 0.5 * h, float("nan"), h, 0.5 * h]
    dead = (1, 3, 4, 5, 7)
    for out_res, smooth in ((1.5 * h, 1.0), (1.5 * h, 4.0), (0.1 * h, 1.0), (5 * h, 2.5)):
        plan = plan_of(driver, PlanCase(rows, steps, out_res, smooth, path0=3), tmp_path)
        paths, at = plan["paths"], 0
        for k, p in enumerate(paths):
            assert p["off"] == at, k                   # every path keeps its place, with or without points
            assert (p["n"] == 0) == (k in dead), k
            if k in dead:
                assert (p["nFwd"], p["n1"], p["n2"], p["nF"], p["sres"]) == (0, 0, 0, 0, 0.0), k
            else:
                assert p["n"] == p["nF"] >= 4 and p["nFwd"] == rows[k][0], k
            at += p["n"]
        assert plan["totF"] == at
        assert paths[6]["tStep"] == 0.75 / 3. != steps[6]
        assert paths[8]["n"] == paths[0]["n"] and paths[0]["tStep"] == h
        # the plain route of path 0, from the formulas of ba.cpp:1683 and 1841
        n1 = max(int(smooth * math.ceil(h * 999 / out_res + 1.)), 4) if out_res >= h else None
        if n1 is not None:
            assert paths[0]["n1"] == n1 and paths[0]["n"] == (max(int((n1 - 1) / smooth) + 1, 4) if smooth > 1.5 else n1)
        # no launch sequence holds a point of a dead path, and the batch index of a path is path0 + k
        for ka, kb, staged, routes in plan["chunks"]:
            for route, (tot, members) in routes.items():
                for m in members:
                    assert (m["nF"] == 0) == (m["p"] - 3 in dead)
    assert reinterpolated(steps, 1.5 * h)[:3] == [False, False, True]


# ---- c: invariants of the cuts and the layout ---------------------------------------------------------------------------
def check_layout(plan, K, budget):
    paths, cuts = plan["paths"], plan["cuts"]
    assert cuts[0] == 0 and cuts[-1] == K and all(a < b for a, b in zip(cuts, cuts[1:]))
    assert [(ka, kb) for ka, kb, _, _ in plan["chunks"]] == list(zip(cuts, cuts[1:]))
    sizes = []
    for ka, kb, staged, routes in plan["chunks"]:
        need = sum(p["need"] for p in paths[ka:kb])
        sizes.append(need)
        assert need <= budget or kb - ka == 1, (ka, kb)
        if kb < K:   # (the cuts are greedy: the next path would not have fitted)
            assert need + paths[kb]["need"] > budget, (ka, kb)
        live = [p for p in paths[ka:kb] if p["n"]]
        assert staged == (len({p["route"] for p in live}) >= 2), (ka, kb)
        assert set(routes) == {p["route"] for p in live}
        seen = []
        for route, (tot, members) in routes.items():
            assert [m["p"] for m in members] == [p["k"] for p in paths[ka:kb] if p["route"] == route]
            at = dict(off1=0, off2=0, offS=0, offF=0)
            for m in members:
                p = paths[m["p"]]
                assert (m["n1"], m["n2"], m["nFwd"], m["nF"]) == (p["n1"], p["n2"], p["nFwd"], p["nF"])
                # dense and ascending within the route; without smoothing the down-sampled arrays are the stage-1 arrays
                assert m["off1"] == at["off1"] and m["offS"] == at["offS"] and m["offF"] == at["offF"]
                assert m["off2"] == (at["off2"] if route & 1 else at["off1"])
                assert route & 1 or m["n2"] == m["n1"]
                # the result stays in path order
                assert m["offD"] == p["off"] - paths[ka]["off"]
                at = dict(off1=at["off1"] + m["n1"], off2=at["off2"] + m["n2"], offS=at["offS"] + m["nFwd"], offF=at["offF"] + m["nF"])
            assert (tot["t1"], tot["t2"], tot["tS"], tot["tF"]) == (at["off1"], at["off2"], at["offS"], at["offF"]) and tot["Kc"] == len(members)
            seen += [m["p"] for m in members if m["nF"]]
        assert sorted(seen) == [p["k"] for p in live]          # every live path in exactly one route
        end = paths[kb]["off"] if kb < K else plan["totF"]
        assert sum(p["n"] for p in paths[ka:kb]) == end - paths[ka]["off"]   # offD ends at the chunk's share of totF
    assert plan["maxChunk"] == max(sizes)


def check_three_budgets(driver, where, make_case):
    """make_case(budget) -> PlanCase of a range that mixes routes.  A budget no path fits (a chunk per path), the largest path and
    the fourth smallest together (a few paths per chunk), and the sum (one chunk): the budget changes the cuts and nothing else"""
    one = plan_of(driver, make_case(HUGE), where)
    K, needs = len(one["paths"]), sorted(p["need"] for p in one["paths"])
    assert one["mixed"] and len(routes_live(one)) == 2 and one["cuts"] == [0, K] and one["chunks"][0][2]
    for budget, lo, hi in ((float(needs[0] - 1), K, K), (float(needs[-1] + needs[3]), 2, K - 1), (float(sum(needs)), 1, 1)):
        plan = plan_of(driver, make_case(budget), where)
        check_layout(plan, K, budget)
        assert lo <= len(plan["cuts"]) - 1 <= hi, (budget, plan["cuts"])
        assert plan["paths"] == one["paths"] and plan["totF"] == one["totF"]


def test_layout_invariants_on_the_core_batch(driver, core, tmp_path):
    exp, res, h = core
    for smooth in (1.0, 5.0):
        check_three_budgets(driver, tmp_path, lambda budget: PlanCase.of_results(res, exp.steps, 1.1 * h, smooth, budget))
    # the setting of test_poisoned_scratch_and_chunk_cuts_together (tests/test_gpu_output_steps.py): several chunks, one of them staged
    plan = plan_of(driver, PlanCase.of_results(res, exp.steps, 1.1 * h, 5.0, float(1 << 20)), tmp_path)
    check_layout(plan, len(exp.steps), float(1 << 20))
    assert len(plan["cuts"]) - 1 >= 3 and any(staged for _, _, staged, _ in plan["chunks"])


@pytest.mark.parametrize("torque_step,pose", [(False, False), (True, False), (False, True)])
def test_layout_invariants_on_made_up_rows(driver, tmp_path, torque_step, pose):
    """thirteen paths of very different sizes whose routes alternate, two of them without a trajectory"""
    h = 0.001
    rng = np.random.default_rng(5)
    rows, steps = [], []
    for k in range(13):
        n = int(rng.integers(4, 3000))
        step = h * (0.5, 1.0, 1.7)[k % 3]
        rows.append((n, step * (n - 1), 0, capi.ST_CAPACITY if k in (4, 9) else 0))
        steps.append(step)
    for smooth in (1.0, 3.0):
        check_three_budgets(driver, tmp_path, lambda budget: PlanCase(rows, steps, 1.2 * h, smooth, budget, 13, torque_step, pose))


# ---- d: the same cases under the sanitizers -----------------------------------------------------------------------------
def test_driver_under_the_address_and_undefined_behaviour_sanitizers(driver, core, tmp_path):
    """repeats what the tests above gave the driver (the core grid when it runs alone); a host program of its own, nothing preloaded"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this compiler cannot link the sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    exe = tmp_path / "output_plan_main_san"
    r = compile_driver(exe, [SANITIZE, "-fno-sanitize-recover=all", "-g"])
    assert r.returncode == 0, r.stderr[-3000:]
    exp, res, h = core
    cases = list(ALL_CASES) or [PlanCase.of_results(res, exp.steps, f * h, smooth, float(1 << 20)) for f, smooth in CORE_GRID]
    for case in cases:
        assert run_driver(exe, case, tmp_path) == run_driver(driver, case, tmp_path)
