"""The knot window of the batch sweep kernels (batotp_amd/csrc/knot_window.h, the segment change of k_sweep8 and k_sweep8_lock) without a GPU.

tests/drivers/knot_window_main.cpp is compiled with g++ against that header alone and replays the segment-change block of a wavefront of
eight cursors against a plain array lookup: forward and reverse; paths of 4, 5, 6, 7 knots (the smallest the library accepts and 1, 2, 3
more) up to 1000; moves of 0, 1 and 2 or more segments per query, moves against the direction of the sweep, random jumps, and both ends of
the path (the prefetch index clamped).  The loads are handed out at once, or only at the head of the wavefront's next block -- where the
kernels wait for them -- and hold a poison value until then.  At every change the window reports a hit exactly when it holds the two knots
of the segment, and then holds them bit for bit; otherwise it reports a miss (the literal route)."""
import os
import re
import subprocess

import helpers

DRIVER = os.path.join(helpers.ROOT, "tests", "drivers", "knot_window_main.cpp")
INCLUDES = [f"-I{helpers.ROOT}/batotp_amd/csrc", f"-I{helpers.ROOT}/include"]


def test_window_equals_the_array_lookup(tmp_path):
    exe = tmp_path / "knot_window_main"
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", *INCLUDES, DRIVER, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.fullmatch(r"ok queries=(\d+) blocks=(\d+) changes=(\d+) hits=(\d+) misses=(\d+) far=(\d+) against=(\d+) first=(\d+) reloads=(\d+) "
                     r"clampedLoads=(\d+)\s*", r.stdout)
    assert m, r.stdout[-3000:]
    queries, blocks, changes, hits, misses, far, against, first, reloads, clamped = (int(v) for v in m.groups())
    print(r.stdout.strip())
    assert queries >= 10**6 and blocks > queries // 16
    assert hits + misses == changes and far + against + first == misses
    # every kind of change and of load is there in numbers, or the replay tested nothing
    assert hits > changes // 10 and far > changes // 10 and against > 1000
    assert first >= 8 * 2 * 2 * 40 * 3 // 4, "nearly every lane of every round changes at least once"
    assert reloads > blocks, "lanes that did not change reload what they hold"
    assert clamped > 1000, "loads at the ends of a path are clamped"
