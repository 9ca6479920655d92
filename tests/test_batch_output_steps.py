"""BA::optimizeBatch on paths that integrate with different steps: with the automatic integration resolution on (the class
default) the rule of reference ba.cpp:522-536 derives a step per path.  A library that samples every path of a range with
its own step (BATOTP_OUT_STEP_PER_PATH) serves the batch in ONE batotp_hip_output call; the CPU checker refuses that value,
and the host library then falls back, silently, on one call per run of equal step.  Either way every path's files are those
of the same path optimised alone.

The inputs are six variants of the golden UR5 taught path whose tool translation is shrunk about its first point: the less
the tool point travels, the more the orientation movement dominates and the finer the step the rule leaves."""
import filecmp
import os
import shutil
import subprocess

import pytest

import helpers

HOST = os.path.join(helpers.ROOT, "batotp_amd", "host")
DRIVER = os.path.join(helpers.ROOT, "tests", "drivers", "batch_steps_main.cpp")
HOST_LIB = os.path.join(HOST, "_build", "libbatotp.a")
# translation factors, chosen with the checker build so that the rule leaves more than three distinct steps, with two equal
# neighbours (a run of two) among them
FACTORS = (1.0, 1.0, 0.19, 0.174, 0.158, 0.19)
FILES = ("traj_out.dat", "s-sdot.dat")
# an output resolution between the steps, so that some paths are re-interpolated and others are not
OUT_RES = (".008  // outRes", "0.006 // outRes")


def write_variants(work):
    """config_<p>.dat + taught_<p>.csv for every factor; returns the configuration names"""
    src = os.path.join(helpers.GOLD, "UR5")
    lines = open(os.path.join(src, "trajUR.csv")).read().splitlines()
    header, rows = lines[0], [[float(v) for v in ln.split(",")] for ln in lines[1:] if ln.strip()]
    config = open(os.path.join(src, "config.dat")).read()
    assert "trajUR.csv" in config and OUT_RES[0] in config
    config = config.replace(*OUT_RES)
    names = []
    for p, f in enumerate(FACTORS):
        x0 = rows[0][7:10]
        with open(os.path.join(work, f"taught_{p}.csv"), "w") as out:
            out.write(header + "\n")
            for r in rows:
                r = list(r)
                for c in range(3):
                    r[7 + c] = x0[c] + f * (r[7 + c] - x0[c])
                out.write(", ".join(repr(v) for v in r) + "\n")
        with open(os.path.join(work, f"config_{p}.dat"), "w") as out:
            out.write(config.replace("trajUR.csv", f"taught_{p}.csv"))
        names.append(f"config_{p}.dat")
    return names


def compile_driver(exe, link):
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", f"-I{HOST}", f"-I{helpers.ROOT}/include", DRIVER, *link, "-pthread", "-lm", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def run_driver(exe, work, names):
    r = subprocess.run([str(exe), *names], cwd=work, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    steps, calls = {}, None
    for ln in r.stdout.splitlines():
        w = ln.split()
        if len(w) == 3 and w[0] == "step":
            steps[int(w[1])] = float(w[2])
        if len(w) == 2 and w[0] == "output_calls":
            calls = int(w[1])
    steps = [steps[p] for p in range(len(names))]
    assert len(set(steps)) >= 3, steps          # the batch the test is about: at least three distinct steps
    return steps, calls


def runs_of_equal_step(steps):
    return 1 + sum(1 for a, b in zip(steps, steps[1:]) if a != b)


def cpu_run(work):
    """the driver linked with the host library and the CPU checker"""
    names = write_variants(work)
    exe = os.path.join(work, "batch_steps_cpu")
    compile_driver(exe, [HOST_LIB, f"-L{helpers.BUILD}", "-lbatotp_oracle_abi", f"-Wl,-rpath,{helpers.BUILD}", "-fopenmp"])
    return names, run_driver(exe, work, names)


def test_checker_build_falls_back_to_one_call_per_run_of_equal_step(tmp_path, oracle_lib):
    names, (steps, calls) = cpu_run(str(tmp_path))
    assert 1 < runs_of_equal_step(steps) < len(steps), steps      # a run of two paths among the runs
    assert calls == runs_of_equal_step(steps), (calls, steps)
    # every path alone through BA::optimize's call sequence (the checker's batest), the rule switched on
    batest = os.path.join(helpers.BUILD, "batest_oracle")
    for p, name in enumerate(names):
        alone = tmp_path / f"alone_{p}"
        alone.mkdir()
        shutil.copy(tmp_path / name, alone / "config.dat")
        shutil.copy(tmp_path / f"taught_{p}.csv", alone / f"taught_{p}.csv")
        r = subprocess.run([batest, "config.dat", "--auto-integ-res"], cwd=alone, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        for f in FILES:
            assert filecmp.cmp(tmp_path / f"out_{p}" / f, alone / f, shallow=False), (p, f, steps[p])


@pytest.mark.gpu
def test_device_build_serves_the_batch_in_one_output_call(tmp_path, hip_ctx, oracle_lib):
    cpu = tmp_path / "cpu"
    gpu = tmp_path / "gpu"
    cpu.mkdir(); gpu.mkdir()
    _, (steps_cpu, _) = cpu_run(str(cpu))
    names = write_variants(str(gpu))
    exe = gpu / "batch_steps_gpu"
    csrc = os.path.join(helpers.ROOT, "batotp_amd", "csrc")
    compile_driver(exe, [HOST_LIB, f"-L{csrc}", "-lbatotp_hip", f"-Wl,-rpath,{csrc}"])
    steps, calls = run_driver(exe, str(gpu), names)
    assert steps == steps_cpu
    assert calls == 1, (calls, steps)
    for p in range(len(names)):
        for f in FILES:
            assert filecmp.cmp(gpu / f"out_{p}" / f, cpu / f"out_{p}" / f, shallow=False), (p, f, steps[p])
