#!/usr/bin/env python3
"""Generate tests/golden/* -- runs ONLY in the build container (needs /root/reference).

For every case this script
  1. assembles a work directory: a config.dat plus its trajectory file (either the reference's own
     shipped example data, input/<robot>/*, or a synthetic input written by batotp_amd.pathgen);
  2. runs THE REFERENCE ITSELF on it -- the prebuilt /root/reference/bin/batest (real Eigen, GCC
     5.3.1; started through the dynamic loader because the mount is read-only / not executable) --
     and keeps its outputs s-sdot.dat (both integrated curves, float32) and traj_out.dat;
  3. runs oracle/_build/dump_knots (host resampling of this repo, no device) to record the fp64
     knot values and the problem description that feed the hot path.
The fixtures are DATA (inputs and expected outputs).  No reference source is copied.
The failure pins (PIN_CASES below: failed bisections, the time limit) are a second table: pinned by the reference's log, read as a
stream, and its float32 files; oracle/README.md has the list.

Usage:  python oracle/make_golden.py [case ...]
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from batotp_amd import pathgen  # noqa: E402

REF = "/root/reference"
REF_BIN = os.path.join(REF, "bin", "batest")
LOADER = "/lib64/ld-linux-x86-64.so.2"
DUMP = os.path.join(ROOT, "oracle", "_build", "dump_knots")
GOLD = os.path.join(ROOT, "tests", "golden")


def edit_config(src: str, dst: str, subs: dict):
    """copy a config.dat replacing the value of the lines whose trailing comment names a key"""
    out = []
    for line in open(src):
        for key, val in subs.items():
            if re.search(r"//\s*" + re.escape(key) + r"\b", line):
                line = f"{val} // {key} (edited)\n"
        out.append(line)
    open(dst, "w").write("".join(out))


def shipped(robot_dir: str, subs=None):
    def build(work):
        src = os.path.join(REF, "input", robot_dir)
        for f in os.listdir(src):
            if f.endswith(".m") or f.startswith("trajKuka"):
                continue  # generators / raw logs are not inputs of batest
            shutil.copy(os.path.join(src, f), os.path.join(work, f))
            os.chmod(os.path.join(work, f), 0o644)
        if subs:
            edit_config(os.path.join(src, "config.dat"), os.path.join(work, "config.dat"), subs)
    return build


def shipped_ur5_positions_only():
    """the shipped UR5 example (joints and tool poses taught together, path type BOTH) with the three position columns only:
    nCart = 3, no orientations -- the reference then skips aa2qVect / q2aaVect and resamples both channel sets as taught
    (ba.cpp:184-192, 245-262, 1726-1736, 1922)"""
    def build(work):
        src = os.path.join(REF, "input", "UR5")
        rows = [", ".join(x.strip() for x in line.split(",")[:10]) for line in open(os.path.join(src, "trajUR.csv")).read().splitlines()]
        open(os.path.join(work, "trajUR.csv"), "w").write("\n".join(rows) + "\n")      # timestamp, j1..j6, x, y, z
        edit_config(os.path.join(src, "config.dat"), os.path.join(work, "config.dat"), {"nCart": 3})
    return build


def with_repeats(x, every):
    """repeat every `every`-th taught point and the last one (remClosePts has to drop them again; the repeated last
    point takes its tail rule)"""
    cols = []
    for i in range(x.shape[1]):
        cols.append(i)
        if i % every == every - 1:
            cols.append(i)
    cols.append(x.shape[1] - 1)
    return np.ascontiguousarray(x[:, cols])


def synth_gen7dof(seed, n_coarse, repeat_every=0, **cfg):
    def build(work):
        th = pathgen.gen7dof_fine(seed, n_coarse)
        if repeat_every:
            th = with_repeats(th, repeat_every)
        pathgen.write_traj_bin(os.path.join(work, "path.dat"), 0.01, th, None)
        kw = dict(robot="GENJNT", is_parallel=0, n_joints=7, n_cart=3, traj_file="path.dat", is_bin=1, path_type="JOINT",
                  degrees=0, jnt_vel=[5] * 7, jnt_acc_on=1, jnt_acc=[10] * 7, integ_res=0.01, max_integ_time=200000.0,
                  theta_res=0.1, theta_res2=0.1, out_res=0.008, out_smooth=5)
        kw.update(cfg)
        pathgen.write_config(os.path.join(work, "config.dat"), **kw)
    return build


def synth_ur(seed, n_coarse, **cfg):
    def build(work):
        th = pathgen.ur_like_fine(seed, n_coarse)
        pathgen.write_traj_bin(os.path.join(work, "path.dat"), 0.01, th, None)
        kw = dict(robot="GENJNT", is_parallel=0, n_joints=6, n_cart=3, traj_file="path.dat", is_bin=1, path_type="JOINT",
                  degrees=1, jnt_vel=[160] * 6, jnt_acc_on=1, jnt_acc=[573, 573, 573, 1146, 1146, 1146], integ_res=0.008,
                  max_integ_time=200000.0, theta_res=0.3, theta_res2=0.3, out_res=0.008, out_smooth=1)
        kw.update(cfg)
        pathgen.write_config(os.path.join(work, "config.dat"), **kw)
    return build


def synth_cspr(seed, n_coarse, repeat_every=0, amp=3.0, **cfg):
    def build(work):
        ca = pathgen.cspr_fine(seed, n_coarse, amp=amp)
        if repeat_every:
            ca = with_repeats(ca, repeat_every)
        pathgen.write_traj_bin(os.path.join(work, "path.dat"), 0.005, None, ca)
        kw = dict(robot="CSPR3DOF", is_parallel=1, n_joints=3, n_cart=3, traj_file="path.dat", is_bin=1, path_type="CART",
                  degrees=0, jnt_vel=[4] * 3, jnt_acc_on=1, jnt_acc=[8] * 3, trq_on=1, trq_max=[12] * 3, trq_min=[1] * 3,
                  cart_vel_on=1, cart_vel=4.0, cart_acc_on=0, cart_acc=100.0, integ_res=0.01, max_integ_time=200000.0,
                  s_weights=(0, 0, 1), scale_type=2, theta_res=0.01, theta_res2=0.01, cart_res=0.01, cart_res2=0.01,
                  out_res=0.02, out_smooth=1, par2ser=1)
        kw.update(cfg)
        pathgen.write_config(os.path.join(work, "config.dat"), **kw)
    return build


# name -> (builder, keep_full_outputs)
CASES = {
    # the reference's own five examples (BASELINE config 1 is RR)
    "RR": (shipped("RR"), True),
    "UR5": (shipped("UR5"), True),
    "GEN7DOF": (shipped("GEN7DOF"), True),
    "CSPR3DOF": (shipped("CSPR3DOF"), True),
    "KUKA-LWR-IV": (shipped("KUKA-LWR-IV"), True),
    # same data, other branches of the constraint code
    "CSPR3DOF_par": (shipped("CSPR3DOF", {"isPar2Ser": 0}), True),          # parallel-mechanism torque branch (LU solves)
    "RR_acc": (shipped("RR", {"isJntAccConOn": 1, "JntAccLims": "900 900"}), True),  # torque + joint accel
    "UR5_nocartacc": (shipped("UR5", {"isCartAccConOn": 0}), True),
    "UR5_pos3": (shipped_ur5_positions_only(), True),                        # BOTH path with nCart = 3: positions without orientations
    "KUKA_cartacc": (shipped("KUKA-LWR-IV", {"isCartAccConOn": 1, "CartAccMax": 2.0}), True),
    # solveLinSys through Eigen's Jacobi SVD (util.cpp:421-438): per-knot conversion (isPar2Ser = 1) / every constraint check (0)
    "CSPR3DOF_svd": (shipped("CSPR3DOF", {"isSVD": 1}), True),
    "CSPR3DOF_par_svd": (shipped("CSPR3DOF", {"isSVD": 1, "isPar2Ser": 0}), True),
    # synthetic inputs in the shapes of BASELINE configs 2, 4, 5 (small, kept in full)
    "synth_gen7dof_s0": (synth_gen7dof(0, 60), True),
    "synth_gen7dof_s1_vel": (synth_gen7dof(1, 40, jnt_acc_on=0), True),
    "synth_ur_s2": (synth_ur(2, 80), True),
    "synth_cspr_s3": (synth_cspr(3, 20), True),
    "synth_cspr_s5": (synth_cspr(5, 60), True),
    # taught paths with repeated points: remClosePts really removes something (also on the device resampler's path kinds)
    "synth_gen7dof_s6_dup": (synth_gen7dof(6, 30, repeat_every=7), True),
    "synth_cspr_s9_dup": (synth_cspr(9, 12, repeat_every=5), True),
    # input decimation + smoothing (ba.cpp:195-242)
    "synth_gen7dof_s10_decim": (synth_gen7dof(10, 45, decim=3, smooth=3), True),
    "synth_cspr_s11_decim": (synth_cspr(11, 14, decim=2), True),
    # wide windows (factor >= 5: the shrinking-window branches of smooth(), half width 2 and 4), also on a pose path and on
    # the robots with forward kinematics
    "synth_gen7dof_s23_decim9": (synth_gen7dof(23, 12, repeat_every=4, decim=9, smooth=2), True),
    "synth_cspr_s22_decim5": (synth_cspr(22, 14, decim=5, smooth=2), True),
    "UR5_decim5": (shipped("UR5", {"inputDecimFact": 5, "smoothWindow": 3}), True),
    "RR_decim5": (shipped("RR", {"inputDecimFact": 5, "smoothWindow": 3}), True),
    "KUKA_decim5": (shipped("KUKA-LWR-IV", {"inputDecimFact": 5, "smoothWindow": 3}), True),
    # s = teach time (sWeights 1 0 0: adjust_s returns at once, ba.cpp:416): the knots are the taught points after close-point
    # removal, input smoothing / decimation -- the branch the host library keeps (BA::keepTaughtSpacing with the filters of
    # batotp_amd/host/util.cpp); repeated points so that remClosePts really thins the path, the last one repeated too
    "synth_gen7dof_s14_teachtime": (synth_gen7dof(14, 24, repeat_every=7, decim=3, smooth=3, s_weights=(1, 0, 0), scale_type=0), True),
    "synth_gen7dof_s15_teachtime_decim2": (synth_gen7dof(15, 18, repeat_every=5, decim=2, s_weights=(1, 0, 0), scale_type=0), True),
    # BASELINE-size single paths: digest only (sha256 of the float32 curves + 1-in-64 samples)
    "synth_gen7dof_s4_50k": (synth_gen7dof(4, 871), False),
    "synth_ur_s7_100k": (synth_ur(7, 500), False),
    "synth_cspr_s8_40k": (synth_cspr(8, 200), False),
}


# ---------------------------------------------------------------------------------------------------------------------
# Failure pins: bisections that fail (ba.cpp:1307-1319, the -1 that ba.cpp:1091 ignores) and sweeps that run into maxIntegTime
# (ba.cpp:1117-1122), pinned by the reference's log and its float32 files.  A table of their own: these cases carry a pin.json
# and none of the files the other case lists of tests/helpers.py are keyed on.  Cases of one family with the same config.dat
# differ in the path only, so the device tests can run them as one ragged batch.

def _raised_cosine(n, lo, hi, height):
    """height * (1 - cos) / 2 over the fractions [lo, hi] of an n-point path, zero outside (a window may reach past an end)"""
    x = np.arange(n, dtype=np.float64) / (n - 1)
    w = np.zeros(n)
    m = (x >= lo) & (x <= hi)
    w[m] = 0.5 * height * (1.0 - np.cos(2.0 * np.pi * (x[m] - lo) / (hi - lo)))
    return w


GEN3_CFG = dict(n_joints=3, jnt_vel=[3, 2, 5], jnt_acc=[20, -1, 12], max_integ_time=30.0)


def synth_gen3_windows(seed, n_coarse, windows, hover=None, **cfg):
    """the GEN7DOF recipe with 3 joints; joint 1 -- the one with the NEGATIVE acceleration limit, for which no sddot is admissible
    wherever it moves -- stands exactly still except in the windows (lo, hi, height): raised-cosine bumps.  hover = (amplitude,
    periods): a ripple so small that |theta'| of that joint crosses jntThresh again and again"""
    def build(work):
        th = pathgen.gen7dof_fine(seed, n_coarse, n_joints=3).astype(np.float64)
        n = th.shape[1]
        j1 = np.zeros(n)
        for lo, hi, height in windows:
            j1 += _raised_cosine(n, lo, hi, height)
        if hover:
            j1 += hover[0] * np.sin(2.0 * np.pi * hover[1] * np.arange(n) / (n - 1))
        th[1] = j1
        pathgen.write_traj_bin(os.path.join(work, "path.dat"), 0.01, th.astype(np.float32), None)
        kw = dict(robot="GENJNT", is_parallel=0, n_cart=3, traj_file="path.dat", is_bin=1, path_type="JOINT", degrees=0,
                  jnt_acc_on=1, integ_res=0.01, theta_res=0.1, theta_res2=0.1, out_res=0.008, out_smooth=5)
        kw.update(GEN3_CFG)
        kw.update(cfg)
        pathgen.write_config(os.path.join(work, "config.dat"), **kw)
    return build


def synth_genjnt(seed, n_coarse, n_joints, jnt_vel, jnt_acc, scale=5.0, **cfg):
    """the GEN7DOF recipe with another joint count and one limit per joint"""
    def build(work):
        th = pathgen.gen7dof_fine(seed, n_coarse, n_joints=n_joints, scale=scale)
        pathgen.write_traj_bin(os.path.join(work, "path.dat"), 0.01, th, None)
        kw = dict(robot="GENJNT", is_parallel=0, n_joints=n_joints, n_cart=3, traj_file="path.dat", is_bin=1, path_type="JOINT",
                  degrees=0, jnt_vel=jnt_vel, jnt_acc_on=1, jnt_acc=jnt_acc, integ_res=0.01, max_integ_time=200000.0,
                  theta_res=0.1, theta_res2=0.1, out_res=0.008, out_smooth=5)
        kw.update(cfg)
        pathgen.write_config(os.path.join(work, "config.dat"), **kw)
    return build


_A = dict(jnt_thresh=1e-3, max_integ_time=300.0)                       # family A: every path finishes
_C = dict(jnt_thresh=1e-3, max_integ_time=10.0)                        # family C: 1001 steps, between the sweeps of some paths
_B = dict(max_integ_time=20.0, trq_max=[8] * 3, trq_min=[1.2] * 3)     # family B: a narrow tension band, 2001 steps
_E = {"maxIntegTime": 6, "JntTrqMin": "NAN NAN"}

# name -> (family, builder).  Cases of one family whose config.dat is the same file form one ragged batch in the device tests.
PIN_CASES = {
    # A. failures the path survives: joint 1 (acceleration limit -1) moves in windows only; jntThresh 1e-3 so that a window may
    #    begin AT an end point (theta' of that joint below the threshold there: the sweep's first stage passes, the next ones
    #    fail).  A window that has the joint moving at the end point itself fails the first stage, and such a sweep can never
    #    finish (sdot = sddot = 0 stay): those paths are in family C, pinned as aborts.
    "pin_a_window_mid": ("A", synth_gen3_windows(31, 12, [(0.40, 0.50, 0.3)], **_A)),
    "pin_a_window_first": ("A", synth_gen3_windows(35, 12, [(0.0, 0.1, 0.3)], **_A)),      # first stages of the forward sweep
    "pin_a_window_last": ("A", synth_gen3_windows(36, 12, [(0.9, 1.0, 0.3)], **_A)),       # first stages of the reverse sweep
    "pin_a_two_windows": ("A", synth_gen3_windows(37, 12, [(0.2, 0.3, 0.3), (0.6, 0.75, -0.2)], **_A)),
    "pin_a_hover": ("A", synth_gen3_windows(38, 12, [], hover=(3e-3, 7), **_A)),           # |theta'| crosses jntThresh repeatedly
    "pin_a_no_window": ("A", synth_gen3_windows(39, 12, [], **_A)),
    # B. the cable robot where the tension band does not admit the path: failures that run into the time limit
    "pin_b_ser_rev_abort": ("B", synth_cspr(37, 10, amp=2.5, **_B)),
    "pin_b_ser_fwd_abort": ("B", synth_cspr(39, 10, amp=4.0, **_B)),
    "pin_b_ser_finishes": ("B", synth_cspr(38, 10, amp=2.5, **_B)),
    "pin_b_par_rev_abort": ("B", synth_cspr(37, 10, amp=2.5, par2ser=0, **_B)),
    "pin_b_par_finishes": ("B", synth_cspr(38, 10, amp=2.5, par2ser=0, **_B)),
    "pin_b_par_svd_finishes": ("B", synth_cspr(38, 10, amp=2.5, par2ser=0, is_svd=1, **_B)),
    # C. the time limit: with and without failures before it, in either sweep, beside a path that finishes
    "pin_c_rev_late": ("C", synth_gen3_windows(36, 12, [(0.9, 1.0, 0.3)], **_C)),          # pin_a_window_last's path
    "pin_c_fwd_late": ("C", synth_gen3_windows(35, 12, [(0.0, 0.1, 0.3)], **_C)),          # pin_a_window_first's: rev 989, fwd 1048
    "pin_c_fwd_late_quiet": ("C", synth_gen3_windows(39, 12, [], **_C)),                   # pin_a_no_window's: rev 999, fwd 1066
    "pin_c_first_stage_fails_fwd": ("C", synth_gen3_windows(35, 12, [(-0.03, 0.07, 0.3)], **_C)),
    "pin_c_first_stage_fails_rev": ("C", synth_gen3_windows(36, 12, [(0.93, 1.03, 0.3)], **_C)),
    "pin_c_finishes": ("C", synth_gen3_windows(60, 8, [(0.3, 0.45, 0.3)], **_C)),
    "pin_c_gen7dof_rev_late": ("C", synth_gen7dof(0, 50, max_integ_time=20.0)),            # synth_gen7dof_s0's recipe, N < 3000
    # D. joint counts and limit spread; all finish, none fails
    "pin_d_1_joint": ("D", synth_genjnt(32, 12, 1, [5], [10])),
    "pin_d_2_joints": ("D", synth_genjnt(40, 12, 2, [5, 3], [10, 25])),
    "pin_d_8_joints": ("D", synth_genjnt(33, 12, 8, [5] * 8, [10] * 8)),
    "pin_d_5_joints_decades": ("D", synth_genjnt(34, 12, 5, [0.5, 5, 50, 500, 3], [2000, 200, 20, 2, 30])),
    # E. the shipped two-link arm with its torque limits tightened until it stalls
    "pin_e_rr_trq_12_8": ("E", shipped("RR", dict(_E, JntTrqMax="12 8"))),
    "pin_e_rr_trq_6_4": ("E", shipped("RR", dict(_E, JntTrqMax="6 4"))),
}


def run_reference_streaming(work):
    """the reference binary on work/config.dat, its stdout read line by line: the bisection-failure messages are counted, their
    continuation lines dropped, every other non-empty line kept.  (A stalled path prints millions of messages: never capture the log
    whole.)  Returns (return code, failure messages, kept lines, bytes of log, seconds)"""
    import time
    t0 = time.time()
    p = subprocess.Popen([LOADER, REF_BIN, "config.dat"], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    fails, kept, nbytes = 0, [], 0
    for raw in p.stdout:
        nbytes += len(raw)
        if b"applyAccelConstraintsBisectionPt() error" in raw:
            fails += 1
        elif raw.startswith(b"  sdot was reduced to") or raw.startswith(b"  did not respect accel") or raw.startswith(b"  sdot point not found"):
            continue
        elif raw.strip():
            kept.append(raw.decode("latin-1"))
    rc = p.wait()
    return rc, fails, "".join(kept), nbytes, time.time() - t0


PIN_CAPS = dict(seconds=10.0, log_bytes=50e6, knots=3000, steps=40000, file_bytes=150e3)


def pin_case(name, write=True):
    family, build = PIN_CASES[name]
    dst = os.path.join(GOLD, name)
    with tempfile.TemporaryDirectory() as work:
        build(work)
        inputs = sorted(os.listdir(work))
        rc, fails, log, nbytes, secs = run_reference_streaming(work)
        assert secs < PIN_CAPS["seconds"] and nbytes < PIN_CAPS["log_bytes"], (name, secs, nbytes)
        m_rev = re.search(r"rev\. integ\.:\s*(\d+) steps", log)
        m_fwd = re.search(r"fwd\. integ\.:\s*(\d+) steps.*?traj time\. ([0-9.]+) sec", log)
        n_knots = re.search(r"after splineFact: (\d+)", log)
        late = len(re.findall(r"Error in sweep\(\): maxIntegTime", log))
        assert late <= 1, (name, log[-2000:])
        aborted = None if not late else ("fwd" if m_rev else "rev")
        have_files = os.path.exists(os.path.join(work, "s-sdot.dat"))
        assert have_files == (aborted is None) and (m_fwd is not None) == (aborted is None), (name, rc, log[-2000:])
        assert (rc == 0) == (aborted is None), (name, rc)
        dk = subprocess.run([DUMP, "config.dat"], cwd=work, capture_output=True, text=True)
        if dk.returncode != 0:
            raise RuntimeError(f"{name}: dump_knots failed\n{dk.stdout[-2000:]}")
        kb = open(os.path.join(work, "knots.bin"), "rb").read()
        N, nJ, nC = (int(v) for v in np.frombuffer(kb, "<i8", 3, 0))
        sres = float(np.frombuffer(kb, "<f8", 1, 24)[0])
        y = np.frombuffer(kb, "<f8", (nJ + nC) * N, 32).reshape(nJ + nC, N)
        pin = {
            "case": name, "family": family, "n_knots": N, "n_knots_ref": int(n_knots.group(1)), "n_joints": nJ, "n_cart": nC,
            "sres_hex": float(sres).hex(),
            "n_rev": int(m_rev.group(1)) if m_rev else None, "n_fwd": int(m_fwd.group(1)) if m_fwd else None,
            "t_total_print": float(m_fwd.group(2)) if m_fwd else None,
            "ref_bisect_fail_msgs": fails, "aborted": aborted, "ref_return_code": rc, "inputs": inputs,
            "sha256_rev": None, "sha256_fwd": None, "sha256_traj_out": None,
            "sha256_knots": hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest(),
            "reference": "prebuilt /root/reference/bin/batest run in the build container",
        }
        assert pin["n_knots"] == pin["n_knots_ref"] <= PIN_CAPS["knots"], (name, pin)
        assert max(pin["n_rev"] or 0, pin["n_fwd"] or 0) <= PIN_CAPS["steps"], (name, pin)
        if aborted is None:
            curves = pathgen.read_s_sdot(os.path.join(work, "s-sdot.dat"))
            pin["sha256_rev"] = hashlib.sha256(curves[0][1].tobytes() + curves[0][2].tobytes()).hexdigest()
            pin["sha256_fwd"] = hashlib.sha256(curves[1][1].tobytes() + curves[1][2].tobytes()).hexdigest()
            pin["sha256_traj_out"] = hashlib.sha256(open(os.path.join(work, "traj_out.dat"), "rb").read()).hexdigest()
        print(f"{name}: N={N} rev={pin['n_rev']} fwd={pin['n_fwd']} T={pin['t_total_print']} fails={fails} aborted={aborted} "
              f"log={nbytes / 1e6:.1f} MB in {secs:.1f} s")
        if not write:
            return pin
        shutil.rmtree(dst, ignore_errors=True)
        os.makedirs(dst)
        for f in inputs:
            shutil.copy(os.path.join(work, f), os.path.join(dst, f))
            os.chmod(os.path.join(dst, f), 0o644)
        if aborted is None:
            shutil.copy(os.path.join(work, "s-sdot.dat"), os.path.join(dst, "ref_s-sdot.dat"))
        with open(os.path.join(dst, "pin.json"), "w") as f:
            json.dump(pin, f, indent=1)
            f.write("\n")
        for f in os.listdir(dst):
            assert os.path.getsize(os.path.join(dst, f)) <= PIN_CAPS["file_bytes"], (name, f)
    return pin


def run_case(name):
    if name in PIN_CASES:
        return pin_case(name)
    build, full = CASES[name]
    dst = os.path.join(GOLD, name)
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    with tempfile.TemporaryDirectory() as work:
        build(work)
        inputs = sorted(os.listdir(work))
        ref = subprocess.run([LOADER, REF_BIN, "config.dat"], cwd=work, capture_output=True, text=True)
        if not os.path.exists(os.path.join(work, "s-sdot.dat")):
            raise RuntimeError(f"{name}: reference produced no s-sdot.dat\n{ref.stdout[-2000:]}\n{ref.stderr[-2000:]}")
        log = ref.stdout
        m_rev = re.search(r"rev\. integ\.:\s*(\d+) steps", log)
        m_fwd = re.search(r"fwd\. integ\.:\s*(\d+) steps.*?traj time\. ([0-9.]+) sec", log)
        n_knots = re.search(r"after splineFact: (\d+)", log)
        fails = len(re.findall(r"applyAccelConstraintsBisectionPt\(\) error", log))
        dk = subprocess.run([DUMP, "config.dat"], cwd=work, capture_output=True, text=True)
        if dk.returncode != 0:
            raise RuntimeError(f"{name}: dump_knots failed\n{dk.stdout[-2000:]}")
        kb = open(os.path.join(work, "knots.bin"), "rb").read()
        N, nJ, nC = np.frombuffer(kb, "<i8", 3, 0)
        sres = float(np.frombuffer(kb, "<f8", 1, 24)[0])
        y = np.frombuffer(kb, "<f8", int((nJ + nC) * N), 32).reshape(int(nJ + nC), int(N))
        prob = np.frombuffer(open(os.path.join(work, "problem.bin"), "rb").read(), np.uint8)
        curves = pathgen.read_s_sdot(os.path.join(work, "s-sdot.dat"))
        expected = {
            "case": name, "n_knots": int(N), "n_knots_ref": int(n_knots.group(1)), "n_joints": int(nJ), "n_cart": int(nC),
            "sres": sres, "sres_hex": float(sres).hex(),
            "n_rev": int(m_rev.group(1)), "n_fwd": int(m_fwd.group(1)), "t_total_print": float(m_fwd.group(2)),
            "ref_bisect_fail_msgs": fails, "inputs": inputs,
            "sha256_rev": hashlib.sha256(curves[0][1].tobytes() + curves[0][2].tobytes()).hexdigest(),
            "sha256_fwd": hashlib.sha256(curves[1][1].tobytes() + curves[1][2].tobytes()).hexdigest(),
            "reference": "prebuilt /root/reference/bin/batest run in the build container",
        }
        assert expected["n_knots"] == expected["n_knots_ref"], (name, expected)
        for f in inputs:
            shutil.copy(os.path.join(work, f), os.path.join(dst, f))
        if full:
            np.savez_compressed(os.path.join(dst, "knots.npz"), y=y, sres=np.float64(sres), problem=prob)
            shutil.copy(os.path.join(work, "s-sdot.dat"), os.path.join(dst, "ref_s-sdot.dat"))
            shutil.copy(os.path.join(work, "traj_out.dat"), os.path.join(dst, "ref_traj_out.dat"))
        else:
            np.savez_compressed(os.path.join(dst, "ref_curves_sampled.npz"),
                                rev_s=curves[0][1][::64], rev_sd=curves[0][2][::64],
                                fwd_s=curves[1][1][::64], fwd_sd=curves[1][2][::64])
            expected["sha256_knots"] = hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()
            expected["sha256_traj_out"] = hashlib.sha256(open(os.path.join(work, "traj_out.dat"), "rb").read()).hexdigest()
            for f in inputs:  # the big synthetic input is regenerated from its seed by the tests
                if f.endswith(".dat") and f != "config.dat":
                    os.remove(os.path.join(dst, f))
        json.dump(expected, open(os.path.join(dst, "expected.json"), "w"), indent=1)
        print(f"{name}: N={N} rev={expected['n_rev']} fwd={expected['n_fwd']} T={expected['t_total_print']} fails={fails}")


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES) + list(PIN_CASES)
    for n in names:
        run_case(n)
    pins = [os.path.join(GOLD, n, f) for n in PIN_CASES if os.path.isdir(os.path.join(GOLD, n)) for f in os.listdir(os.path.join(GOLD, n))]
    assert sum(os.path.getsize(f) for f in pins) < 1e6, "the failure pins together must stay under 1 MB"
