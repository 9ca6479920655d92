"""What every output made from an output shares on the host, without a GPU: tests/drivers/range_plan_main.cpp includes
batotp_amd/csrc/output_plan.h and batotp_amd/csrc/stretch_rounds.h alone.

a. the ranges a budget cuts a ragged batch into and the block table of every range, against a transcription of the loop the three
   drivers (torque rows, torque scale, stretch) each carried before they shared one
b. the decision of a stretch round, fed the records the numpy references read (tests/stretch_reference.py, tests/tscale_reference.py)
   on their synthetic batches: n_out, rounds and status of every path after every round, and the report"""
import os
import subprocess

import numpy as np
import pytest

import helpers
import stretch_reference as sr
import tscale_reference as tr
from batotp_amd import capi
from test_gpu_invdyn import model_named
from test_gpu_stretch import audit_batch, steps

DRIVER = os.path.join(helpers.ROOT, "tests", "drivers", "range_plan_main.cpp")
INCLUDES = [f"-I{helpers.ROOT}/batotp_amd/csrc", f"-I{helpers.ROOT}/include"]
HUGE = float(1 << 40)
LENGTHS = [4, 0, 1, 2, 3, 127, 128, 129, 257]
ARGS = [(1.0, 8, 16.0), (0.8, 8, 1.75), (1.0, 1, 16.0)]      # those of tests/test_gpu_tscale.py and the first three of tests/test_gpu_stretch.py
# bytes per (path, block, point) of the scratch estimates: torque rows, torque rows with host tables of 7 links, torque scale, stretch
BYTE_MODELS = [(40, 8, 0), (40, 8, 8 * 3 * 7), (48, 8 + 32, 0), (48, 8 + 32, 8 * 3 * 7)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("range_plan") / "range_plan_main"
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", *INCLUDES, DRIVER, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    return exe


# ---- a: cuts and block tables -------------------------------------------------------------------------------------------
def loop_of_the_drivers(lengths, bp, budget, need):
    """the cut loop as invdyn_api.inc, tscale_api.inc and stretch_api.inc each had it"""
    cuts, nbytes, largest = [0], 0, 0
    for k, n in enumerate(lengths):
        if k > cuts[-1] and float(nbytes + need(n)) > budget:
            cuts.append(k)
            nbytes = 0
        nbytes += need(n)
        largest = max(largest, nbytes)
    cuts.append(len(lengths))
    return cuts, largest


@pytest.mark.parametrize("bp", [128, 256])
def test_cuts_and_block_tables(driver, bp):
    counts = set()
    for per_path, per_block, per_point in BYTE_MODELS:
        need = lambda n: per_path + per_block * ((n + bp - 1) // bp) + per_point * n
        for budget in (HUGE, 1.0, float(need(bp))):         # no budget; every path a range of its own; room for one block-sized path
            r = subprocess.run([str(driver), "cuts", str(bp), budget.hex(), str(per_path), str(per_block), str(per_point), *map(str, LENGTHS)],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            lines = [ln.split() for ln in r.stdout.splitlines()]
            cuts, largest = loop_of_the_drivers(LENGTHS, bp, budget, need)
            assert [int(v) for v in lines[0][1:]] == cuts and lines[0][0] == "cuts"
            assert lines[1] == ["max", str(largest)]
            want = []
            for ka, kb in zip(cuts, cuts[1:]):
                nb = [(n + bp - 1) // bp for n in LENGTHS[ka:kb]]
                want.append(["range", str(ka), str(kb), str(sum(nb))])
                want += [["path", str(ka + i), str(sum(nb[:i])), str(nb[i])] for i in range(kb - ka)]
            assert lines[2:] == want
            counts.add(len(cuts) - 1)
    assert 1 in counts and len(LENGTHS) in counts and any(1 < c < len(LENGTHS) for c in counts)


def test_a_table_past_2_31_blocks_is_refused(driver):
    for lengths in ([128 << 31], [64 << 31, 64 << 31, 128]):
        r = subprocess.run([str(driver), "cuts", "128", HUGE.hex(), "40", "8", "0", *map(str, lengths)], capture_output=True, text=True)
        assert r.returncode == 0 and f"range 0 {len(lengths)} overflow" in r.stdout, r.stdout + r.stderr


# ---- b: the rounds ------------------------------------------------------------------------------------------------------
def replay(driver, where, args, n_in, trace, with_scale):
    """the driver on the records of every round of `trace`: ([(again, [(n_out, rounds, status) per path])] per round, report lines)"""
    target, max_rounds, max_factor = args
    K = len(n_in)
    text = [f"{float(target).hex()} {max_rounds} {float(max_factor).hex()} {K} {int(with_scale)}", " ".join(str(n) for n in n_in)]
    for entry in trace:
        audits, scales = (entry[0], entry[1]) if with_scale else (entry[0], [None] * K)
        for a, s in zip(audits, scales):
            peaks = [float(a["fam"][f]["peak"]).hex() for f in range(5)]
            text.append(" ".join(peaks + ([float(s["s"]).hex(), str(int(s["n_static"]))] if with_scale else ["0x0p+0", "0"])))
    path = os.path.join(str(where), "rounds.txt")
    with open(path, "w") as f:
        f.write("\n".join(text) + "\n")
    r = subprocess.run([str(driver), "rounds", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rounds, report = [], []
    for w in (ln.split() for ln in r.stdout.splitlines()):
        if w[0] == "round":
            rounds.append((bool(int(w[1])), []))
        elif w[0] == "path":
            rounds[-1][1].append((int(w[2]), int(w[3]), int(w[4])))
        else:
            assert w[0] == "report"
            report.append((int(w[2]), int(w[3]), float.fromhex(w[4]), int(w[5]), int(w[6])))
    return rounds, report


def check_against_trace(got, trace, report, what):
    rounds, rep = got
    assert len(rounds) == len(trace) >= 1, what
    for r, ((again, paths), entry) in enumerate(zip(rounds, trace)):
        n2, nr, st = entry[-3:]
        assert paths == list(zip(n2, nr, st)), f"{what}: after round {r}"
        assert again == (r + 1 < len(trace)), f"{what}: round {r}"       # the reference leaves its loop when no path was stretched
    want = np.zeros(len(rep), dtype=capi.STRETCH_DTYPE)
    for k, row in enumerate(rep):
        want[k] = row
    sr.assert_report_equal(want, report, what)


@pytest.mark.parametrize("args", ARGS, ids=["plain", "cap", "one_round"])
def test_rounds_of_the_audit_mode(driver, tmp_path, args):
    rows, prob = audit_batch()
    trace = []
    report = sr.stretch_audit(rows, steps(rows), 3, 3, prob, *args, trace=trace)[1]
    check_against_trace(replay(driver, tmp_path, args, [r.shape[1] for r in rows], trace, False), trace, report, f"audit mode {args}")
    if args == ARGS[0]:
        assert len(trace) >= 3
    if args == ARGS[1]:
        assert capi.STRETCH_CAPPED in trace[-1][-1]
    if args == ARGS[2]:
        assert capi.STRETCH_ROUNDS in trace[-1][-1] and len(trace) == 2


_CASE = {}


@pytest.mark.parametrize("args", ARGS, ids=["plain", "cap", "one_round"])
def test_rounds_of_the_torque_mode(driver, oracle_lib, tmp_path, args):
    if not _CASE:
        model = model_named(oracle_lib, "rr")
        rows = tr.synth_rows(model)
        sres = tr.synth_steps(len(rows))
        _CASE.update(model=model, rows=rows, sres=sres, prob=tr.synth_problem(oracle_lib, model, rows, sres), caches={})
    c = _CASE
    trace = []
    report = tr.stretch_torques(oracle_lib, c["model"], c["rows"], c["sres"], 0, c["prob"], *args, cache=c["caches"].setdefault(args[0], {}), trace=trace)[1]
    check_against_trace(replay(driver, tmp_path, args, [r.shape[1] for r in c["rows"]], trace, True), trace, report, f"torque mode {args}")
    # the scale records take part: without them the same audit records give another answer
    if args == ARGS[0]:
        blind = replay(driver, tmp_path, args, [r.shape[1] for r in c["rows"]], [(e[0], e[2], e[3], e[4]) for e in trace], False)
        assert [p for _, p in blind[0]] != [list(zip(*e[-3:])) for e in trace]


def test_static_and_the_minus_one_peak(driver, tmp_path):
    """a record by hand: gravity alone leaves the range on a path whose kinematic families pass -- STATIC, not stretched; a TRQ peak of
    -1 passes; the same path with a velocity peak over the target is stretched by that peak and never by 1 / s"""
    def rec(vel, trq):
        a = np.zeros((), dtype=capi.AUDIT_DTYPE)
        for f in range(5):
            a["fam"][f]["peak"] = -1.0
        a["fam"][capi.AUDIT_JNT_VEL]["peak"], a["fam"][capi.AUDIT_TRQ]["peak"] = vel, trq
        return a

    def scale(s, n_static):
        t = np.zeros((), dtype=capi.TSCALE_DTYPE)
        t["s"], t["n_static"] = s, n_static
        return t

    audits = [rec(0.5, 1.5), rec(0.5, -1.0), rec(2.0, 1.5), rec(0.5, 1.5)]
    scales = [scale(0.25, 3), scale(0.25, 0), scale(0.25, 3), scale(0.25, 0)]
    rounds, report = replay(driver, tmp_path, (1.0, 8, 16.0), [101] * 4, [(audits, scales)], True)
    assert rounds == [(True, [(101, 0, capi.STRETCH_STATIC), (101, 0, capi.STRETCH_PASSES), (201, 1, capi.STRETCH_PASSES), (401, 1, capi.STRETCH_PASSES)])]
    assert [r[2] for r in report] == [1.0, 1.0, 2.0, 4.0]
