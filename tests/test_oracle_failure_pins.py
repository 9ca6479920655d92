"""CPU: the oracle against the failure pins -- what the reference binary printed and wrote on paths whose bisections fail
(ba.cpp:1307-1319: -1, sddot untouched, ba.cpp:1091 integrates on) and on paths that run into maxIntegTime (ba.cpp:1117-1122).

The fixtures are tests/golden/pin_* (oracle/make_golden.py: PIN_CASES): config.dat, the input path, pin.json with the knot
count, the step counts and duration of the sweeps that finished, the number of failure messages in the log, which sweep gave
up, and the sha256 of the float32 files where the reference wrote them."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
from helpers import pin_case, run_pin_batch, assert_matches_pin


@pytest.mark.parametrize("name", helpers.PIN_CASES)
def test_oracle_reproduces_the_reference_on_failing_and_late_paths(oracle_ctx, name):
    case = pin_case(name)
    e = case.expected
    assert case.n == e["n_knots"] and float(case.sres).hex() == e["sres_hex"]
    assert hashlib.sha256(np.ascontiguousarray(case.y).tobytes()).hexdigest() == e["sha256_knots"]
    out = run_pin_batch(oracle_ctx, [case])[0]
    assert_matches_pin(case, out)


@pytest.mark.parametrize("name", helpers.PIN_CASES)
def test_batest_end_to_end_on_failing_and_late_paths(tmp_path, oracle_lib, name):
    """the host library with the oracle behind it: the reference's traj_out.dat for a path that finishes; for one that does not,
    the reference's message, its return code and no trajectory file"""
    case = pin_case(name)
    e = case.expected
    for f in e["inputs"]:
        shutil.copy(os.path.join(case.dir, f), tmp_path / f)
    r = subprocess.run([os.path.join(helpers.BUILD, "batest_oracle"), "config.dat"], cwd=tmp_path, capture_output=True, text=True)
    late = r.stdout.count("Error in sweep(): maxIntegTime")
    if case.aborted is None:
        assert r.returncode == 0 and late == 0, r.stdout[-3000:]
        assert hashlib.sha256(open(tmp_path / "traj_out.dat", "rb").read()).hexdigest() == e["sha256_traj_out"]
        assert open(tmp_path / "s-sdot.dat", "rb").read() == open(os.path.join(case.dir, "ref_s-sdot.dat"), "rb").read()
    else:
        assert r.returncode != 0 and late == 1, r.stdout[-3000:]
        assert ("rev. integ.:" in r.stdout) == (case.aborted == "fwd"), r.stdout[-3000:]   # which sweep gave up
        assert "fwd. integ.:" not in r.stdout
        assert not os.path.exists(tmp_path / "traj_out.dat") and not os.path.exists(tmp_path / "s-sdot.dat")


@pytest.mark.parametrize("family", ["A", "B", "C"])
def test_oracle_families_as_ragged_batches(oracle_ctx, family):
    """the paths of a family that share a config.dat as ONE batch of the checker library: every path as pinned"""
    batches = helpers.pin_batches(family)
    assert max(len(b) for b in batches) >= 3
    for cases in batches:
        for case, out in zip(cases, run_pin_batch(oracle_ctx, cases)):
            assert_matches_pin(case, out)
