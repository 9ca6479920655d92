"""Shared helpers of the test-suite: golden-case loading and the knots -> curves pipeline."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

from batotp_amd import capi, pathgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BUILD = os.path.join(ROOT, "oracle", "_build")
ORACLE_ABI_LIB_PATH = os.path.join(BUILD, "libbatotp_oracle_abi.so")


def load_oracle() -> capi.Library:
    """TEST INFRASTRUCTURE: the CPU oracle behind the product's C-ABI (the checker; never the thing under test)."""
    return capi.Library(ORACLE_ABI_LIB_PATH)

SELF = os.path.join(ROOT, "tests", "golden_self")   # fixtures the reference cannot produce (oracle/make_selfgolden.py)
SELF_CASES = sorted(d for d in os.listdir(SELF) if os.path.exists(os.path.join(SELF, d, "knots.npz"))) if os.path.isdir(SELF) else []

FULL_CASES = sorted(d for d in os.listdir(GOLD) if os.path.exists(os.path.join(GOLD, d, "knots.npz")))
DIGEST_CASES = sorted(d for d in os.listdir(GOLD) if os.path.exists(os.path.join(GOLD, d, "ref_curves_sampled.npz")))

RESAMPLE_CASES = sorted(d for d in os.listdir(GOLD) if os.path.exists(os.path.join(GOLD, d, "resample.npz")))

OUTPUT_CASES = sorted(d for d in os.listdir(GOLD) if os.path.exists(os.path.join(GOLD, d, "output.npz")))

# failure pins (oracle/make_golden.py: PIN_CASES): failed bisections and the time limit, pinned by the reference's log and float32 files
PIN_CASES = sorted(d for d in os.listdir(GOLD) if os.path.exists(os.path.join(GOLD, d, "pin.json")))

# how the digest-only inputs are regenerated (must match oracle/make_golden.py)
DIGEST_INPUTS = {
    "synth_gen7dof_s4_50k": lambda: (pathgen.gen7dof_fine(4, 871), None, 0.01),
    "synth_ur_s7_100k": lambda: (pathgen.ur_like_fine(7, 500), None, 0.01),
    "synth_cspr_s8_40k": lambda: (None, pathgen.cspr_fine(8, 200), 0.005),
}


def problem_from_bytes(raw: np.ndarray) -> capi.Problem:
    assert raw.size == C.sizeof(capi.Problem), (raw.size, C.sizeof(capi.Problem))
    return capi.Problem.from_buffer_copy(raw.tobytes())


class Case:
    def __init__(self, name, root=None):
        self.name = name
        self.dir = os.path.join(root or (SELF if name in SELF_CASES and not os.path.isdir(os.path.join(GOLD, name)) else GOLD), name)
        self.expected = json.load(open(os.path.join(self.dir, "expected.json")))
        self.full = os.path.exists(os.path.join(self.dir, "knots.npz"))
        if self.full:
            z = np.load(os.path.join(self.dir, "knots.npz"))
            self.y = np.ascontiguousarray(z["y"])
            self.sres = float(z["sres"])
            self.problem = problem_from_bytes(z["problem"])
            if self.problem.robot_type in (capi.ROBOT_KUKA, capi.ROBOT_RR) or self.problem.n_cart == 7:
                # what BA::fillProblem sets for the robots with forward kinematics and for pose paths since round 3 (the fixture's
                # bytes are older): the output stage takes the cos / sin of its forward kinematics (the atan2 of its pose
                # conversion) from the host libm
                self.problem.flags |= capi.F_HOST_TRIG
            self.ref = pathgen.read_s_sdot(os.path.join(self.dir, "ref_s-sdot.dat"))
        else:
            self._regen()

    def _regen(self):
        """digest-only case: rebuild the input from its seed, resample it with the host library"""
        theta, cart, tres = DIGEST_INPUTS[self.name]()
        with tempfile.TemporaryDirectory() as work:
            pathgen.write_traj_bin(os.path.join(work, "path.dat"), tres, theta, cart)
            with open(os.path.join(self.dir, "config.dat")) as f, open(os.path.join(work, "config.dat"), "w") as g:
                g.write(f.read())
            r = subprocess.run([os.path.join(BUILD, "dump_knots"), "config.dat"], cwd=work, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout[-2000:]
            kb = open(os.path.join(work, "knots.bin"), "rb").read()
            N, nJ, nC = (int(v) for v in np.frombuffer(kb, "<i8", 3, 0))
            self.sres = float(np.frombuffer(kb, "<f8", 1, 24)[0])
            self.y = np.frombuffer(kb, "<f8", (nJ + nC) * N, 32).reshape(nJ + nC, N).copy()
            self.problem = problem_from_bytes(np.frombuffer(open(os.path.join(work, "problem.bin"), "rb").read(), np.uint8))
        self.ref = None
        self.sampled = np.load(os.path.join(self.dir, "ref_curves_sampled.npz"))

    @property
    def n(self):
        return self.y.shape[1]

    def max_steps(self):
        return int(max(self.expected["n_rev"], self.expected["n_fwd"]) + 64)


class PinCase(Case):
    """a failure pin: config.dat and the committed input path, resampled by the host library against the oracle shim like the
    digest-only cases; pin.json holds what the reference's log and float32 files pin (expected["aborted"]: None, "rev" or "fwd")"""

    def __init__(self, name):
        self.name = name
        self.dir = os.path.join(GOLD, name)
        self.expected = json.load(open(os.path.join(self.dir, "pin.json")))
        self.full = False
        self.config = open(os.path.join(self.dir, "config.dat")).read()
        with tempfile.TemporaryDirectory() as work:
            for f in self.expected["inputs"]:
                with open(os.path.join(self.dir, f), "rb") as src, open(os.path.join(work, f), "wb") as dst:
                    dst.write(src.read())
            r = subprocess.run([os.path.join(BUILD, "dump_knots"), "config.dat"], cwd=work, capture_output=True, text=True)
            assert r.returncode == 0, r.stdout[-2000:]
            kb = open(os.path.join(work, "knots.bin"), "rb").read()
            N, nJ, nC = (int(v) for v in np.frombuffer(kb, "<i8", 3, 0))
            self.sres = float(np.frombuffer(kb, "<f8", 1, 24)[0])
            self.y = np.frombuffer(kb, "<f8", (nJ + nC) * N, 32).reshape(nJ + nC, N).copy()
            self.problem = problem_from_bytes(np.frombuffer(open(os.path.join(work, "problem.bin"), "rb").read(), np.uint8))
        if self.problem.robot_type in (capi.ROBOT_KUKA, capi.ROBOT_RR):
            self.problem.flags |= capi.F_HOST_TRIG     # as BA::fillProblem sets it (see Case)
        f = os.path.join(self.dir, "ref_s-sdot.dat")
        self.ref = pathgen.read_s_sdot(f) if os.path.exists(f) else None
        self.aborted = self.expected["aborted"]
        assert (self.ref is None) == (self.aborted is not None)

    def max_steps(self):
        """room for the sweeps that finish; for an aborted case room for the steps the time limit allows (ba.cpp:984, :1117)"""
        if self.aborted is None:
            return int(max(self.expected["n_rev"], self.expected["n_fwd"]) + 64)
        return int(np.floor(self.problem.max_integ_time / self.problem.integ_res)) + 2 + 64


_PIN_CACHE = {}


def pin_case(name):
    """PinCase(name), resampled once per session"""
    if name not in _PIN_CACHE:
        _PIN_CACHE[name] = PinCase(name)
    return _PIN_CACHE[name]


def pin_batches(family):
    """the pins of a family grouped by config.dat: the paths of one group share a problem description, i.e. can run as one batch"""
    groups = {}
    for name in PIN_CASES:
        c = pin_case(name)
        if c.expected["family"] == family:
            groups.setdefault(c.config, []).append(c)
    return list(groups.values())


ST_ABORT = capi.ST_MAX_INTEG_TIME | capi.ST_CAPACITY | capi.ST_NONFINITE


def run_pin_batch(ctx, cases, extra_flags=0):
    """knots -> precompute -> both sweeps of the cases as one batch: a list of dicts "result", "rev", "fwd" (a curve is None
    where its sweep did not finish)"""
    prob = cases[0].problem
    if extra_flags:
        prob = capi.Problem.from_buffer_copy(bytes(prob))
        prob.flags |= extra_flags
    b = capi.Batch(ctx, prob, [c.n for c in cases], max(c.max_steps() for c in cases))
    for k, c in enumerate(cases):
        b.upload_knots(k, [c.y], [c.sres])
    precompute_with_trig(ctx, b, prob, len(cases))
    b.sweep(-1); b.sweep(+1)
    res = b.results()
    out = []
    for k in range(len(cases)):
        d = {"result": res[k].copy()}
        d["rev"] = b.curve(k, -1) if not (int(res[k]["status_rev"]) & ST_ABORT) else None
        d["fwd"] = b.curve(k, +1) if not (int(res[k]["status_fwd"]) & ST_ABORT) else None
        out.append(d)
    b.close()
    return out


def assert_matches_pin(case, out):
    """what the reference binary pinned for a failure pin (its log; its float32 files where it wrote them) against one path's rows
    and curves.  An aborted run of the reference prints no step count for the sweep it gave up and runs no forward sweep after
    a reverse sweep that gave up: for those only the time-limit bit and the failure messages up to the abort are pinned"""
    e, r = case.expected, out["result"]
    st_rev, st_fwd = int(r["status_rev"]), int(r["status_fwd"])
    fails = int(r["n_bisect_fail_rev"]) + int(r["n_bisect_fail_fwd"])
    what = (case.name, {f: r[f].item() for f in r.dtype.names}, e)
    assert fails == e["ref_bisect_fail_msgs"], what
    assert bool((st_rev | st_fwd) & capi.ST_BISECT_FAIL) == (fails > 0), what
    if case.aborted is None:
        assert int(r["n_rev"]) == e["n_rev"] and int(r["n_fwd"]) == e["n_fwd"], what
        assert abs(float(r["t_total"]) - e["t_total_print"]) < 5.1e-4, what   # the log prints three decimals
        assert not ((st_rev | st_fwd) & ST_ABORT), what
        assert f32_digest(*out["rev"]) == e["sha256_rev"], case.name
        assert f32_digest(*out["fwd"]) == e["sha256_fwd"], case.name
        for which, (sres, s, sd), (ms, msd) in zip(("reverse", "forward"), case.ref, (out["rev"], out["fwd"])):
            assert_bit_equal(ms.astype(np.float32), s, f"{case.name}: {which} s against the reference's s-sdot.dat")
            assert_bit_equal(msd.astype(np.float32), sd, f"{case.name}: {which} sdot against the reference's s-sdot.dat")
    elif case.aborted == "rev":
        assert st_rev & capi.ST_MAX_INTEG_TIME and not (st_rev & (capi.ST_CAPACITY | capi.ST_NONFINITE)), what
        # the reference stops here.  The product runs no forward sweep either: no step, no point, no failure of its own (its
        # status word repeats the reverse sweep's, a convention of the product the log cannot show)
        assert int(r["n_rev"]) == 0 and int(r["n_fwd"]) == 0 and int(r["steps_fwd"]) == 0 and int(r["n_bisect_fail_fwd"]) == 0, what
    else:
        assert not (st_rev & ST_ABORT) and int(r["n_rev"]) == e["n_rev"], what
        assert st_fwd & capi.ST_MAX_INTEG_TIME and not (st_fwd & (capi.ST_CAPACITY | capi.ST_NONFINITE)), what
        assert int(r["n_fwd"]) == 0, what


class PrefixCase:
    """the first n knots of a golden case as a path of its own, under the problem description `problem` (one per batch)"""

    def __init__(self, case, n, problem):
        self.name, self.problem, self.sres = f"{case.name}[:{n}]", problem, case.sres
        self.y = np.ascontiguousarray(case.y[:, :n])
        self._max_steps = case.max_steps()

    @property
    def n(self):
        return self.y.shape[1]

    def max_steps(self):
        return self._max_steps     # (a prefix needs no more steps than the whole path)


class ResampleCase:
    """taught points + resampling parameters of a golden case; expected output = its knots.npz"""

    def __init__(self, name):
        self.name = name
        d = os.path.join(GOLD, name)
        z = np.load(os.path.join(d, "resample.npz"))
        self.params = capi.ResampleParams.from_bytes(z["params"].tobytes())
        self.sres_in = float(z["sres_in"])
        nJ, nC = self.params.n_joints, self.params.n_cart
        n = int(z["n_in"])
        if "x" in z.files:   # text input: the taught points are stored in the fixture
            self.x = np.ascontiguousarray(z["x"])
        else:
            tres, theta, cart = pathgen.read_traj_bin(os.path.join(d, str(z["traj_file"])), nJ, nC)
            assert float(tres) == self.sres_in
            self.x = np.zeros((nJ + nC, n))
            if theta is not None:
                self.x[:nJ] = theta
            if cart is not None:
                self.x[nJ:] = cart
        k = np.load(os.path.join(d, "knots.npz"))
        self.y = np.ascontiguousarray(k["y"])
        self.sres = float(k["sres"])


def read_traj_out(path, n_joints, n_cart):
    """traj_out.dat as BA::trajWriteBIN writes it: float32 sres; int32 nPts; int32 1; float32 theta[nJ][nPts];
    int32 hasCart; [float32 cart[nC][nPts]]; int32 hasTrq; [float32 trq[nJ][nPts]]"""
    raw = open(path, "rb").read()
    sres = np.frombuffer(raw, "<f4", 1, 0)[0]
    n = int(np.frombuffer(raw, "<i4", 1, 4)[0])
    assert int(np.frombuffer(raw, "<i4", 1, 8)[0]) == 1
    pos = 12
    theta = np.frombuffer(raw, "<f4", n_joints * n, pos).reshape(n_joints, n)
    pos += 4 * n_joints * n
    has_cart = int(np.frombuffer(raw, "<i4", 1, pos)[0])
    pos += 4
    cart = None
    if has_cart:
        cart = np.frombuffer(raw, "<f4", n_cart * n, pos).reshape(n_cart, n)
        pos += 4 * n_cart * n
    has_trq = int(np.frombuffer(raw, "<i4", 1, pos)[0])
    pos += 4
    trq = np.frombuffer(raw, "<f4", n_joints * n, pos).reshape(n_joints, n) if has_trq else None
    return sres, n, theta, cart, trq


def output_params(name):
    z = np.load(os.path.join(GOLD, name, "output.npz"))
    return capi.OutputParams.from_buffer_copy(z["params"].tobytes())


def run_to_output(ctx, cases, extra_flags=0):
    """knots -> hot path -> output stage on the library behind ctx; returns (Output, Batch)"""
    prob = cases[0].problem
    if extra_flags:
        prob = capi.Problem.from_buffer_copy(bytes(prob))
        prob.flags |= extra_flags
    b = capi.Batch(ctx, prob, [c.n for c in cases], max(c.max_steps() for c in cases))
    for k, c in enumerate(cases):
        b.upload_knots(k, [c.y], [c.sres])
    precompute_with_trig(ctx, b, prob, len(cases))
    b.sweep(-1); b.sweep(+1)
    return capi.Output(b, output_params(cases[0].name), 0, len(cases)), b


def precompute_with_trig(ctx, b, prob, n_paths, serial_model=None, samples_from=None):
    """both precompute stages of a batch whose knots are uploaded, with the model table and the host trig tables the
    dynamics of a serial robot need in between (what the host layer does in ba_device.cpp)"""
    b.precompute(1)
    # (a batch without a sample array -- pairs for all channels -- takes the joint samples of the host trig tables from a run of the
    #  same cases that kept them: samples_from[k]["samp"])
    samples = (lambda k, j: samples_from[k]["samp"][j]) if samples_from is not None else (lambda k, j: b.samples(k, j))
    if prob.flags & capi.F_TRQ_ON:
        if serial_model is None and needs_serial_model(prob):
            serial_model = ctx.library.builtin_serial_model(prob.robot_type)
        if serial_model is not None:
            b.set_serial_model(serial_model)
            if prob.flags & capi.F_HOST_TRIG:
                for k in range(n_paths):
                    b.upload_joint_trig(k, joint_trig(serial_model, [samples(k, j)[0] for j in range(prob.n_joints)]))
        elif prob.robot_type == capi.ROBOT_RR and (prob.flags & capi.F_HOST_TRIG):
            for k in range(n_paths):
                b.upload_rr_trig(k, rr_trig(samples(k, 0)[0], samples(k, 1)[0]))
        b.precompute(2)


def assert_output_equals_reference_file(case, out, k=0):
    """the trajectory of path k rounded to float32 = the reference binary's traj_out.dat, byte for byte"""
    n_cart_file = 6 if case.problem.n_cart == 7 else case.problem.n_cart   # poses are written as axis-angle again (q2aaVect)
    sres32, n, theta32, cart32, trq32 = read_traj_out(os.path.join(case.dir, "ref_traj_out.dat"), case.problem.n_joints, n_cart_file)
    assert int(out.n_pts[k]) == n, (case.name, int(out.n_pts[k]), n)
    assert np.float32(out.sres[k]) == sres32
    rows = out.rows(k)
    nT, nC = out.n_theta, out.n_cart
    assert rows[:nT].astype("<f4").tobytes() == theta32.tobytes(), case.name + ": theta"
    if nC:
        assert cart32 is not None and rows[nT:nT + nC].astype("<f4").tobytes() == cart32.tobytes(), case.name + ": cart"
    if out.n_trq:
        assert trq32 is not None and rows[nT + nC:].astype("<f4").tobytes() == trq32.tobytes(), case.name + ": torques"


def rr_trig(theta_samples0, theta_samples1):
    """cos/sin with the host libm, as the host layer does for RR (reference robot.cpp:401-419)"""
    d2r = 3.14159265358979323846 / 180.0
    th1, th2 = d2r * theta_samples0, d2r * theta_samples1
    return np.stack([np.cos(th1), np.cos(th2), np.cos(th1 + th2), np.sin(th2)])


def joint_trig(model, theta_samples):
    """[2*nJ][N] cosines, then sines, of the joint angles with the C library's cos / sin (math.cos is libm's, numpy's
    vectorised cos is not) -- what the host layer uploads for a serial-chain model (ba_device.cpp)"""
    import math
    unit = (3.14159265358979323846 / 180.0) if model.degrees else 1.0
    nJ = model.n_links
    out = np.empty((2 * nJ, theta_samples[0].shape[0]))
    for j in range(nJ):
        q = unit * np.asarray(theta_samples[j])
        out[j] = [math.cos(v) for v in q]
        out[nJ + j] = [math.sin(v) for v in q]
    return out


def needs_serial_model(prob):
    return bool(prob.flags & capi.F_TRQ_ON) and not (prob.flags & capi.F_PARALLEL) and prob.robot_type != capi.ROBOT_RR


def run_pipeline(ctx, cases, max_steps=None, mvc=True, details=True, extra_flags=0, serial_model=None, samples_from=None):
    """knots -> precompute -> (pointwise) -> sweeps on the library behind `ctx`, as one batch.

    All cases must share one problem description.  Returns a list of dicts, one per case."""
    prob = cases[0].problem
    if extra_flags:
        prob = capi.Problem.from_buffer_copy(bytes(prob))
        prob.flags |= extra_flags
    cap = max_steps or max(c.max_steps() for c in cases) + (16 if prob.flags & capi.F_CURVES_IN_PLACE else 0)  # in place: 72 points of margin
    if prob.flags & capi.F_MVC_IN_CURVES:
        cap = max(cap, (3 * max(c.n for c in cases) + 1) // 2)   # the pointwise values of a path must fit its curve slot
    b = capi.Batch(ctx, prob, [c.n for c in cases], cap)
    for k, c in enumerate(cases):
        b.upload_knots(k, [c.y], [c.sres])
    precompute_with_trig(ctx, b, prob, len(cases), serial_model, samples_from)
    mvc_early = None
    if mvc:
        b.pointwise_mvc()
        if prob.flags & capi.F_MVC_IN_CURVES:   # valid until a sweep starts
            mvc_early = [np.stack(b.mvc(k)) for k in range(len(cases))]
    b.sweep(-1)
    # BATOTP_F_CURVES_IN_PLACE: the forward sweep overwrites the reverse curve, so it is fetched between the sweeps
    in_place = bool(prob.flags & capi.F_CURVES_IN_PLACE)
    rev_early = [b.curve(k, -1) for k in range(len(cases))] if in_place else None
    b.sweep(+1)
    res = b.results()
    out = []
    for k, c in enumerate(cases):
        d = {"result": res[k]}
        d["rev"] = rev_early[k] if in_place else b.curve(k, -1)
        d["fwd"] = b.curve(k, +1)
        if details:
            nch = prob.n_channels
            d["coef"] = np.stack([b.coeffs(k, ch) for ch in range(nch)])
            if not (prob.flags & capi.F_NO_SAMPLES):
                d["samp"] = np.stack([b.samples(k, ch) for ch in range(prob.n_joints + prob.n_cart)])
            pairs_all = bool(prob.flags & capi.F_COMPACT_SPLINES) and (prob.dyn_dim or prob.flags & (capi.F_CART_VEL_ON | capi.F_CART_ACC_ON))
            if prob.dyn_dim and not pairs_all:   # (pairs for all channels: no dynamics array, the values are c0 of the channels' rows)
                d["dyn"] = np.stack([np.stack([b.dyn(k, kk, r) for r in range(prob.dyn_dim)]) for kk in (1, 2, 3, 4)])
        if mvc:
            d["mvc"] = mvc_early[k] if mvc_early is not None else np.stack(b.mvc(k))
        out.append(d)
    b.close()
    return out


def f32_digest(s, sd):
    return hashlib.sha256(np.asarray(s, dtype="<f4").tobytes() + np.asarray(sd, dtype="<f4").tobytes()).hexdigest()


def assert_matches_reference(case, out):
    """the curves, rounded to float32 exactly like the reference's sdotWrite (ba.cpp:2745-2748),
    must reproduce the reference binary's s-sdot.dat bit for bit; step counts and T likewise"""
    e = case.expected
    r = out["result"]
    assert int(r["n_rev"]) == e["n_rev"], (case.name, r, e)
    assert int(r["n_fwd"]) == e["n_fwd"], (case.name, r, e)
    assert abs(float(r["t_total"]) - e["t_total_print"]) < 5.1e-4  # the log prints %.3f
    assert int(r["n_bisect_fail_rev"]) + int(r["n_bisect_fail_fwd"]) == e["ref_bisect_fail_msgs"]
    assert f32_digest(*out["rev"]) == e["sha256_rev"], case.name
    assert f32_digest(*out["fwd"]) == e["sha256_fwd"], case.name
    if case.ref is not None:
        for (sres, s, sd), (ms, msd) in zip(case.ref, (out["rev"], out["fwd"])):
            assert np.array_equal(s, ms.astype(np.float32))
            assert np.array_equal(sd, msd.astype(np.float32))
    assert_matches_reference_f64(case, out)


def f64_digest(s, sd):
    return hashlib.sha256(np.ascontiguousarray(s, dtype="<f8").tobytes() + np.ascontiguousarray(sd, dtype="<f8").tobytes()).hexdigest()


def assert_matches_reference_f64(case, out):
    """fp64 bit equality with what the reference binary held in memory at the return of each BA::sweep (traj.sMVC, traj.sdot,
    traj.tTotalTraj read under the ROCm toolchain's gdb by oracle/make_golden_f64.py): every point of both curves for the small cases, their
    sha256 for the BASELINE-size ones"""
    f = os.path.join(case.dir, "expected_f64.json")
    if not os.path.exists(f):
        return      # (tests/golden_self: no reference exists for those)
    e = json.load(open(f))
    r = out["result"]
    assert float(r["t_total"]).hex() == e["t_total_hex"], (case.name, float(r["t_total"]).hex(), e["t_total_hex"])
    assert float(r["t_rev"]) == e["t_rev"], (case.name, float(r["t_rev"]), e["t_rev"])
    assert f64_digest(*out["rev"]) == e["sha256_rev_f64"], case.name
    assert f64_digest(*out["fwd"]) == e["sha256_fwd_f64"], case.name
    g = os.path.join(case.dir, "ref_curves_f64.npz")
    if os.path.exists(g):
        z = np.load(g)
        assert_bit_equal(out["rev"][0], z["rev_s"], f"{case.name}: reverse s vs the reference's fp64 memory")
        assert_bit_equal(out["rev"][1], z["rev_sd"], f"{case.name}: reverse sdot vs the reference's fp64 memory")
        assert_bit_equal(out["fwd"][0], z["fwd_s"], f"{case.name}: forward s vs the reference's fp64 memory")
        assert_bit_equal(out["fwd"][1], z["fwd_sd"], f"{case.name}: forward sdot vs the reference's fp64 memory")


def assert_bit_equal(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a.view(np.uint64) == b.view(np.uint64)) if a.dtype == np.float64 else (a == b)
    if not np.all(same):
        idx = np.argwhere(~same)[:5]
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} of {a.size} values differ, first at {idx.tolist()}: "
                             f"{[ (a[tuple(i)], b[tuple(i)]) for i in idx ]}")


def random_knots(rng, n_joints, n, scale):
    """smooth random joint paths: a few random Fourier modes per joint, plus a straight segment and a cusp now and then"""
    s = np.linspace(0.0, 1.0, n)
    y = np.zeros((n_joints, n))
    for j in range(n_joints):
        for k in range(1, 5):
            y[j] += rng.normal() / k * np.sin(2 * np.pi * k * s * rng.uniform(0.3, 2.0) + rng.uniform(0, 6.28))
    if rng.random() < 0.3:
        a = rng.integers(n // 4, n // 2)
        y[:, a:a + n // 8] = y[:, a:a + 1] + np.linspace(0, 1, n // 8)[None, :] * rng.normal(size=(n_joints, 1)) * 0.1
    if rng.random() < 0.3:
        y[rng.integers(0, n_joints)] += 0.3 * np.abs(s - rng.uniform(0.2, 0.8))
    return np.ascontiguousarray(scale * y)


def run_sweeps(ctx, prob, ys, sres, cap):
    """knots -> precompute -> pointwise values -> both sweeps of one batch: (result rows, [(reverse curve, forward curve, pointwise values)])"""
    b = capi.Batch(ctx, prob, [y.shape[1] for y in ys], cap)
    for k, y in enumerate(ys):
        b.upload_knots(k, [y], [sres[k]])
    b.precompute(1)
    b.pointwise_mvc()
    b.sweep(-1)
    b.sweep(+1)
    res = b.results()
    out = [(b.curve(k, -1), b.curve(k, +1), np.stack(b.mvc(k))) for k in range(len(ys))]
    b.close()
    return res, out


def set_layout(ctx, layout):
    """sweep-kernel layout of a context: 0 (automatic), 1, 8, 16, 32 lanes per path, or "flatK": 8 lanes per path, 8 paths
    per wavefront and the flat stage / bisection loop with hold K in both directions (batotp_hip_set_sweep_hold; only
    problems with joint velocity / acceleration limits alone use it, the others run the nested loops whatever K is);
    "flatKcH": the same with the reverse sweep's certificate phase at hold H; "64noff": 64 without the certified fast-forward of the
    bisection; "GxP": G lanes per path and P paths per wavefront, the loop form left as it is set"""
    if isinstance(layout, str) and layout.startswith("oldflat"):
        # the flat instantiation of the general kernel instead of k_sweep8 (batotp_hip_set_flat_form 0)
        k = int(layout[7:])
        ctx.set_sweep_group(8)
        ctx.set_paths_per_wave(8)
        ctx.set_sweep_hold(k, k)
        ctx.set_flat_form(0)
    elif isinstance(layout, str) and layout.startswith("flat"):
        # "flat4": hold 4; "flat4c2": ... and the certificate phase of the reverse sweep with hold 2 (batotp_hip_set_cert_hold; c0: no
        # certificate in the reverse sweep)
        k, _, c = layout[4:].partition("c")
        ctx.set_sweep_group(8)
        ctx.set_paths_per_wave(8)
        ctx.set_sweep_hold(int(k), int(k))
        if c:
            ctx.set_cert_hold(int(c))
    elif isinstance(layout, str) and layout.startswith("g"):
        # "g4flat3": 4 lanes per path (two joints per lane), every lane of the wavefront filled, flat loop with hold 3
        g, k = layout[1:].split("flat")
        ctx.set_sweep_group(int(g))
        ctx.set_paths_per_wave(64 // int(g))
        ctx.set_sweep_hold(int(k), int(k))
    elif isinstance(layout, str) and "x" in layout:
        # "8x3": 8 lanes per path, 3 paths per wavefront (the other lane groups idle); "64x2": k_sweep1 with TWO paths per wavefront
        # (one per half): the cable robot in serial form with every channel as pairs, the compact velocity / acceleration layout
        g, p = layout.split("x")
        ctx.set_sweep_group(int(g))
        ctx.set_paths_per_wave(int(p))
    elif layout == "64noff":
        # one path per wavefront (k_sweep1) with every iteration of the bisection checked (batotp_hip_set_fast_forward 0)
        ctx.set_sweep_group(64)
        ctx.set_fast_forward(False)
    else:
        ctx.set_sweep_group(int(layout))
