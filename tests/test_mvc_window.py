"""The reverse-curve cursor of the forward batch kernels (batotp_amd/csrc/mvc_window.h, driven by sweep8_mvcwalk.inc) without a GPU.

tests/drivers/mvc_window_main.cpp is compiled with g++ -ffp-contract=off against that header alone and replays two walks side by
side: the literal comparison walk over the whole array (what the fragment was before it kept a window), and the window walk, eight
cursors in one wavefront-uniform loop, fed by a fake loader that hands out array elements only when asked -- at once, or one query
late.  Curves of 2, 3, 4, 5 and 1000 points with strictly increasing s, repeated values and runs of three equal values; queries on
points and one ulp to either side, NaN and +-inf, jumps of 0, +-1, +-2, +-5 segments (and of hundreds, from one random point to the
next), and the up / down / up pattern of predictor and stages of a forward step.  After every query the driver compares segM, the
segment's four values and the status bits, and checks that the window never asked for an index outside its curve and never moved
onto a point it had not been given."""
import os
import re
import subprocess

import helpers

DRIVER = os.path.join(helpers.ROOT, "tests", "drivers", "mvc_window_main.cpp")
INCLUDES = [f"-I{helpers.ROOT}/batotp_amd/csrc", f"-I{helpers.ROOT}/include"]


def test_window_walk_equals_the_literal_walk(tmp_path):
    exe = tmp_path / "mvc_window_main"
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", *INCLUDES, DRIVER, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.fullmatch(r"ok queries=(\d+) waits0=(\d+) waits1=(\d+) moves=(\d+) passes=(\d+)\s*", r.stdout)
    assert m, r.stdout[-3000:]
    queries, waits0, waits1, moves, passes = (int(v) for v in m.groups())
    print(r.stdout.strip())
    assert queries >= 10**6
    assert moves > queries // 4, "the queries are meant to move the cursors"
    assert waits0 == 0, "a loader that answers at once never makes a move wait"
    # one query late: only a second pass of the same walk waits, so fewer waits than passes -- and some, or the mode tested nothing
    assert 0 < waits1 < passes
