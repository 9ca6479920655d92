"""GPU (-m gpu): torque rows for finished trajectories (include/batotp_hip_invdyn.h) against tests/invdyn_reference.py on the same
rows.  With host trig tables the tolerance is 0: rows are compared as uint64.  Known-answer shapes enter through
capi.output_from_rows; real trajectories are swept and passed through the output stage on the device first."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import invdyn_reference as ir
from audit_reference import audit_reference, assert_audit_equal
from batotp_amd import capi

pytestmark = pytest.mark.gpu

BP = capi.INVDYN_BLOCK_POINTS
LENGTHS = [4, 0, 1, 2, 3, BP - 1, BP, BP + 1, 2 * BP + 1]     # the empty path sits in the middle of the small ones
H = 0.008
ERR_ARG = -1      # BATOTP_ERR_ARG
HOST = os.path.join(helpers.ROOT, "batotp_amd", "host")
CSRC = os.path.join(helpers.ROOT, "batotp_amd", "csrc")
# device libm against host trig tables, relative to each row's max |tau| (test_device_libm prints the measured figure; DESIGN.md 2
# records it: 4.1e-16 on the MI355X): 100 x the measured maximum, rounded up to a power of ten
DEVICE_LIBM_BOUND = 1e-13


def random_model(seed=5, n_links=8):
    """every term of the recursion in play: tilted axes, offsets, centres of mass, full inertia tensors, friction, tilted gravity"""
    rng = np.random.default_rng(seed)
    m = capi.SerialModel()
    m.n_links, m.degrees = n_links, 1
    for j, g in enumerate((1.7, -2.9, -9.1)):
        m.gravity[j] = g
    for i in range(n_links):
        L = m.link[i]
        a = rng.standard_normal(3)
        a /= np.sqrt((a * a).sum())
        B = rng.standard_normal((3, 3))
        I = B @ B.T * 0.02 + np.eye(3) * 0.01          # symmetric positive definite, off-diagonal terms present
        for j in range(3):
            L.axis[j], L.off[j], L.com[j] = float(a[j]), float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.1, 0.1))
        L.mass, L.fv = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.1, 2.0))
        for j, v in enumerate((I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2])):
            L.inertia[j] = float(v)
    return m


def one_link_model():
    m = capi.SerialModel()
    m.n_links, m.degrees = 1, 0
    m.gravity[2] = -9.81
    L = m.link[0]
    L.axis[1] = 1.0
    L.com[0], L.mass, L.fv = 0.25, 2.0, 0.5
    for j, v in enumerate((0.01, 0.02, 0.03, 0.0, 0.0, 0.0)):
        L.inertia[j] = v
    return m


def model_named(lib, name):
    return {"kuka": lambda: lib.builtin_serial_model(capi.ROBOT_KUKA), "rr": lambda: lib.builtin_serial_model(capi.ROBOT_RR),
            "random8": random_model, "one": one_link_model}[name]()


def batch_rows(model, n_cart, lengths=LENGTHS, seed=11):
    """random joint rows (degrees or radians of a few turns at most, steps of a fraction of that) and Cartesian rows"""
    rng = np.random.default_rng(seed + 100 * model.n_links + n_cart)
    span = 90.0 if model.degrees else 1.5
    return [np.ascontiguousarray(rng.uniform(-span, span, (model.n_links + n_cart, n))) for n in lengths]


def steps(rows):
    return np.array([H * (1 + 0.1 * k) for k in range(len(rows))])


_REFERENCE = {}


def known_answers(oracle_lib, name, n_cart):
    """(model, rows, sres, expected rows with torques) of the ragged batch -- computed once, shared, never modified"""
    key = (name, n_cart)
    if key not in _REFERENCE:
        model = model_named(oracle_lib, name)
        rows = batch_rows(model, n_cart)
        sres = steps(rows)
        want = ir.with_torques(oracle_lib, model, rows, sres, n_cart)
        for a in rows + want:
            a.setflags(write=False)
        _REFERENCE[key] = (model, rows, sres, want)
    return _REFERENCE[key]


def check_output(new, want, what):
    got = new.all_rows()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        ir.assert_rows_bit_equal(g, w, f"{what}, path {k} (download_all)")
        ir.assert_rows_bit_equal(new.rows(k), w, f"{what}, path {k} (download)")


# ---- 1. known answers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cart", [0, 3])
@pytest.mark.parametrize("name", ["kuka", "rr", "random8", "one"])
def test_known_answers_host_trig(hip_ctx, oracle_lib, name, n_cart):
    model, rows, sres, want = known_answers(oracle_lib, name, n_cart)
    nl = model.n_links
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, n_cart, 0)
    new = out.torques(model, host_trig=True)
    assert (new.n_theta, new.n_cart, new.n_trq, new.n_rows) == (nl, n_cart, nl, 2 * nl + n_cart)
    assert [int(n) for n in new.n_pts] == LENGTHS and new.sres.tobytes() == sres.tobytes()
    check_output(new, want, f"{name}, n_cart {n_cart}")
    for k, (g, r) in enumerate(zip(new.all_rows(), rows)):
        assert g[:nl + n_cart].tobytes() == r.tobytes(), f"joint and Cartesian rows of path {k} are copies"
    assert new.torques_ms() >= 0.0 and new.torques_ranges() == 1
    # the input is untouched, and it is not a result of the call
    assert (out.n_theta, out.n_cart, out.n_trq) == (nl, n_cart, 0)
    for k, (g, r) in enumerate(zip(out.all_rows(), rows)):
        assert g.tobytes() == r.tobytes(), k
    with pytest.raises(capi.BatotpError):
        out.torques_ms()
    # the device pointer spans the new rows
    ptr, cnt = C.c_void_p(), C.c_int64(0)
    new.L.check(new.lib.batotp_hip_output_device(new.handle, C.byref(ptr), C.byref(cnt)), "output_device")
    assert ptr.value and cnt.value == sum(LENGTHS) * (2 * nl + n_cart)
    new.close(); out.close()


# ---- 2. the same bits however it is cut ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cart", [0, 3])
def test_same_bits_however_it_is_cut(hip_lib, oracle_lib, n_cart):
    model, rows, sres, want = known_answers(oracle_lib, "kuka", n_cart)
    nl = model.n_links
    ctx = capi.Context(hip_lib, 0)          # a context of its own: the budget is a property of the context
    out = capi.output_from_rows(ctx, rows, sres, nl, n_cart, 0)
    whole = out.torques(model)
    assert whole.torques_ranges() == 1
    flat = [r.copy() for r in whole.all_rows()]
    for k in range(len(rows)):              # one call per path
        one = capi.output_from_rows(ctx, [rows[k]], [sres[k]], nl, n_cart, 0)
        new = one.torques(model)
        ir.assert_rows_bit_equal(new.rows(0), flat[k], f"path {k} alone")
        new.close(); one.close()
    # room for the tables of about one block-sized path: the small paths share a range, each of the four long ones has its own
    ctx.set_workspace_budget(0, 8 * 3 * nl * (BP + 2))
    cut = out.torques(model)
    assert cut.torques_ranges() >= 3, cut.torques_ranges()
    for k, (g, w) in enumerate(zip(cut.all_rows(), flat)):
        ir.assert_rows_bit_equal(g, w, f"path {k} under a budget")
    check_output(cut, want, "under a budget")
    ctx.set_workspace_budget(0, 1)          # every path with points a range of its own
    each = out.torques(model)
    assert each.torques_ranges() == sum(1 for n in LENGTHS if n > 0)
    check_output(each, want, "a range per path")
    ctx.set_workspace_budget(0, 0)
    for o in (whole, cut, each, out):
        o.close()


# ---- 3. device libm --------------------------------------------------------------------------------------------------------
def test_device_libm(hip_ctx, oracle_lib):
    model, rows, sres, want = known_answers(oracle_lib, "kuka", 3)
    nl = model.n_links
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 3, 0)
    dev = out.torques(model, host_trig=False)
    got = dev.all_rows()
    for g, w in zip(got, want):
        assert g[:nl + 3].tobytes() == w[:nl + 3].tobytes()
    # a row = one joint's torque channel over the whole batch (on a path of one or two points the arm is at rest and the last
    # joint's torque is rounding noise of 1e-18 Nm: no scale of its own)
    G, W = np.hstack([g[nl + 3:] for g in got]), np.hstack([w[nl + 3:] for w in want])
    scale = np.abs(W).max(axis=1, keepdims=True)
    assert (scale > 1e-3).all()
    worst = float((np.abs(G - W) / scale).max())
    print(f"INVDYN device libm against host trig tables: max |d tau| / max |tau| of the row = {worst:.3e}")
    assert worst <= DEVICE_LIBM_BOUND <= 1e-9
    dev.close(); out.close()


# ---- 4. values that are not finite -----------------------------------------------------------------------------------------
def test_a_nan_poisons_its_stencil_and_nothing_else(hip_ctx, oracle_lib):
    model = oracle_lib.builtin_serial_model(capi.ROBOT_KUKA)
    nl, n, k = model.n_links, BP + 7, BP           # the stencil of point k straddles the block edge
    assert 3 <= k <= n - 4
    rows = batch_rows(model, 0, [n], seed=23)
    clean = ir.with_torques(oracle_lib, model, rows, [H])[0]
    rows[0][2, k] = np.nan
    out = capi.output_from_rows(hip_ctx, rows, [H], nl, 0, 0)
    new = out.torques(model)
    got = new.rows(0)
    assert np.isnan(got[nl:, k - 1:k + 2]).all(), "points k-1, k, k+1: every torque row"
    keep = np.ones(n, dtype=bool)
    keep[k - 1:k + 2] = False
    ir.assert_rows_bit_equal(got[nl:, keep], clean[nl:, keep], "the other points")
    assert got[:nl].view(np.uint64).tobytes() == rows[0].view(np.uint64).tobytes()
    prob = capi.make_problem(nl, 0, capi.ROBOT_KUKA, capi.F_TRQ_ON, jnt_vel_max=[1e6] * nl, jnt_trq_max=[1e4] * nl, jnt_trq_min=[-1e4] * nl)
    a = new.audit(prob, 0.0)
    assert int(a[0]["n_nonfinite"]) == 1 + 3 * nl
    new.close(); out.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(hip_ctx, hip_lib, oracle_lib):
    model, rows, sres, want = known_answers(oracle_lib, "kuka", 0)
    nl = model.n_links
    lib = hip_lib.lib
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    with_trq = capi.output_from_rows(hip_ctx, [np.zeros((nl + 2, 5))], [H], nl, 0, 2)
    six = capi.output_from_rows(hip_ctx, [np.zeros((6, 5))], [H], 6, 0, 0)

    def copy():
        return capi.SerialModel.from_buffer_copy(bytes(model))

    def refused(o, m, flags, what):
        h = C.c_void_p(0xdead)
        rc = lib.batotp_hip_output_torques(o.handle if o is not None else None, C.byref(m) if m is not None else None, flags, C.byref(h))
        msg = lib.batotp_hip_last_error()
        assert rc == ERR_ARG and h.value is None and msg and b"output_torques" in msg, (what, rc, h.value, msg)

    refused(None, model, capi.F_HOST_TRIG, "NULL output")
    refused(out, None, capi.F_HOST_TRIG, "NULL model")
    assert lib.batotp_hip_output_torques(out.handle, C.byref(model), capi.F_HOST_TRIG, None) == ERR_ARG and lib.batotp_hip_last_error()
    for bad in (0, -1, 9):
        m = copy(); m.n_links = bad
        refused(out, m, capi.F_HOST_TRIG, f"n_links {bad}")
    refused(six, model, capi.F_HOST_TRIG, "n_links != n_theta")
    refused(with_trq, model, capi.F_HOST_TRIG, "torque rows already there")
    for field in ("axis", "off", "com", "inertia"):
        for value in (np.nan, np.inf):
            m = copy(); getattr(m.link[nl - 1], field)[1] = value
            refused(out, m, capi.F_HOST_TRIG, f"{field} {value}")
    for field in ("mass", "fv"):
        m = copy(); setattr(m.link[0], field, -np.inf)
        refused(out, m, capi.F_HOST_TRIG, field)
    m = copy(); m.gravity[0] = np.nan
    refused(out, m, capi.F_HOST_TRIG, "gravity")
    m = copy(); m.link[3].axis[0], m.link[3].axis[1], m.link[3].axis[2] = 0.0, 0.0, 1.0 + 1e-11
    refused(out, m, capi.F_HOST_TRIG, "axis not a unit vector")
    for flags in (capi.F_HOST_TRIG | capi.F_TRQ_ON, capi.F_JNT_ACC_ON, 1 << 31):
        refused(out, model, flags, f"flags {flags:#x}")
    # entries of links the model does not use are not read
    one = one_link_model()
    one.link[5].mass = np.nan
    o1 = capi.output_from_rows(hip_ctx, [np.zeros((1, 3))], [H], 1, 0, 0)
    n1 = o1.torques(one)
    assert np.isfinite(n1.rows(0)).all()
    n1.close(); o1.close()
    # the context still serves a valid call
    new = out.torques(model)
    check_output(new, want, "after the refusals")
    new.close()
    # no paths; paths without points
    empty = capi.output_from_rows(hip_ctx, [], [], nl, 3, 0)
    e = empty.torques(model)
    assert e.n_paths == 0 and (e.n_theta, e.n_cart, e.n_trq) == (nl, 3, nl) and e.all_rows() == [] and e.torques_ranges() == 0 and e.torques_ms() == 0.0
    hollow = capi.output_from_rows(hip_ctx, [np.zeros((nl, 0))] * 3, [H] * 3, nl, 0, 0)
    h = hollow.torques(model, host_trig=False)
    assert [int(n) for n in h.n_pts] == [0, 0, 0] and (h.n_theta, h.n_cart, h.n_trq) == (nl, 0, nl) and h.torques_ranges() == 0
    assert all(r.shape == (2 * nl, 0) for r in h.all_rows())
    a = h.audit(capi.make_problem(nl, 0, capi.ROBOT_KUKA, 0, jnt_vel_max=[1.0] * nl), 0.0)
    assert [int(v) for v in a["n_pts"]] == [0, 0, 0]
    for o in (e, empty, h, hollow, out, with_trq, six):
        o.close()


# ---- 6. plan fast, verify the dynamics -------------------------------------------------------------------------------------
def test_plan_fast_then_verify_the_dynamics(hip_ctx, oracle_lib):
    case = helpers.Case("synth_gen7dof_s0")
    assert not (case.problem.flags & capi.F_TRQ_ON)
    out, b = helpers.run_to_output(hip_ctx, [case])
    assert int(out.n_pts[0]) == 7402 and out.n_trq == 0
    model = hip_ctx.library.builtin_serial_model(capi.ROBOT_KUKA)
    nl = model.n_links
    new = out.torques(model, host_trig=True)
    rows = out.all_rows()
    want = ir.with_torques(oracle_lib, model, rows, out.sres, out.n_cart)
    check_output(new, want, "synth_gen7dof_s0")
    prob = capi.Problem.from_buffer_copy(bytes(case.problem))
    prob.flags |= capi.F_TRQ_ON
    for j, t in enumerate((200.0, 200.0, 100.0, 100.0, 50.0, 50.0, 20.0)):
        prob.jnt_trq_max[j], prob.jnt_trq_min[j] = t, -t
    got = new.audit(prob, 0.0)
    ref = audit_reference(new.all_rows(), new.sres, new.n_theta, new.n_cart, new.n_trq, prob, 0.0)
    assert_audit_equal(got, ref, "audit of the rows with torques")
    peak = got[0]["fam"][capi.AUDIT_TRQ]
    print(f"INVDYN synth_gen7dof_s0: {int(new.n_pts[0])} points, TRQ peak {float(peak['peak']):.6f} at point {int(peak['at'])}, row {int(peak['row'])}; "
          f"kernel {new.torques_ms():.3f} ms")
    assert float(peak["peak"]) > 0.0 and int(got[0]["n_nonfinite"]) == 0
    new.close(); out.close(); b.close()


# ---- 7. a record: the stage's own torque rows against the finite-difference ones -------------------------------------------
def test_record_against_the_stage_torque_rows(hip_ctx):
    name = "KUKA_trq"
    assert name in helpers.SELF_CASES
    case = helpers.Case(name)
    prob = case.problem
    assert prob.flags & capi.F_TRQ_ON
    prm = capi.OutputParams(prob.n_joints, capi.PATH_JOINT, prob.integ_res, 0.008, 5.0)
    b = capi.Batch(hip_ctx, prob, [case.n], case.max_steps())
    b.upload_knots(0, [case.y], [case.sres])
    helpers.precompute_with_trig(hip_ctx, b, prob, 1)
    b.sweep(-1); b.sweep(+1)
    staged = capi.Output(b, prm, 0, 1)
    nT, nC, nQ = staged.n_theta, staged.n_cart, staged.n_trq
    assert (nT, nQ) == (7, 7)
    rows = staged.rows(0)
    again = capi.output_from_rows(hip_ctx, [np.ascontiguousarray(rows[:nT + nC])], staged.sres, nT, nC, 0)
    new = again.torques(hip_ctx.library.builtin_serial_model(capi.ROBOT_KUKA))
    fd = new.rows(0)[nT + nC:]
    assert np.isfinite(fd).all() and np.isfinite(rows[nT + nC:]).all()
    half = np.array([(prob.jnt_trq_max[j] - prob.jnt_trq_min[j]) * 0.5 for j in range(nQ)])
    diff = np.abs(fd - rows[nT + nC:]).max(axis=1) / half
    print(f"INVDYN {name}: {rows.shape[1]} points; largest |stage torque - finite-difference torque| per joint, in half ranges of the limit: "
          + " ".join(f"{d:.4f}" for d in diff))
    for o in (new, again, staged):
        o.close()
    b.close()


# ---- 8. the host route -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("invdyn_driver") / "invdyn_batch"
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", f"-I{HOST}", f"-I{helpers.ROOT}/include", os.path.join(helpers.ROOT, "tests", "drivers", "invdyn_batch_main.cpp"),
           os.path.join(HOST, "_build", "libbatotp.a"), f"-L{CSRC}", "-lbatotp_hip", f"-Wl,-rpath,{CSRC}", "-pthread", "-lm", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


TRQ_LIMITS = "200 200 100 100 50 50 20"


def stage_kuka(work):
    """the reference's KUKA example under joint velocity and acceleration limits only, with a torque range for the audit"""
    src = os.path.join(helpers.GOLD, "KUKA-LWR-IV")
    shutil.copy(os.path.join(src, "KUKApath.dat"), work / "KUKApath.dat")
    config = open(os.path.join(src, "config.dat")).read()
    for old, new in (("1           // isCartVelConOn", "0           // isCartVelConOn"),
                     ("0 0 0 0 0 0 0 // JntTrqMax", TRQ_LIMITS + " // JntTrqMax"),
                     ("0 0 0 0 0 0 0 // JntTrqMin", " ".join("-" + v for v in TRQ_LIMITS.split()) + " // JntTrqMin")):
        assert old in config, old
        config = config.replace(old, new)
    (work / "config.dat").write_text(config)


def stage_gen7dof(work):
    src = os.path.join(helpers.GOLD, "synth_gen7dof_s0")
    for f in ("config.dat", "path.dat"):
        shutil.copy(os.path.join(src, f), work / f)


def read_dump(path):
    raw = open(path, "rb").read()
    at, out = 0, []
    while at < len(raw):
        n, nT, nC, nQ = (int(v) for v in np.frombuffer(raw, "<i8", 4, at))
        sres = float(np.frombuffer(raw, "<f8", 1, at + 32)[0])
        at += 40
        rows = np.frombuffer(raw, "<f8", (nT + nC + nQ) * n, at).reshape(nT + nC + nQ, n)
        at += 8 * rows.size
        out.append((nT, nC, nQ, sres, rows))
    return out


@pytest.mark.parametrize("which", ["kuka", "gen7dof_with_a_model"])
def test_host_route(hip_ctx, driver, tmp_path, which):
    extra = []
    if which == "kuka":
        stage_kuka(tmp_path)
    else:
        stage_gen7dof(tmp_path)
        extra = ["--kuka-model"]
    n = 3
    r = subprocess.run([driver, "config.dat", str(n), "on"] + extra, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    on = read_dump(tmp_path / "dump.bin")
    model = hip_ctx.library.builtin_serial_model(capi.ROBOT_KUKA)
    assert len(on) == n
    rows = [np.ascontiguousarray(p[4][:p[0] + p[1]]) for p in on]
    nT, nC, nQ = on[0][:3]
    # (a robot type without kinematics keeps its zero Cartesian rows only where their length happens to equal the joints')
    assert (nT, nQ) == (7, 7) and (nC == 3 if which == "kuka" else nC in (0, 3)) and rows[0].shape[1] > 100
    capi_out = capi.output_from_rows(hip_ctx, rows, [p[3] for p in on], nT, nC, 0)
    new = capi_out.torques(model, host_trig=True)
    for k, g in enumerate(new.all_rows()):
        ir.assert_rows_bit_equal(on[k][4], g, f"Traj rows of path {k} against the C-ABI route")
    peaks = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("trq_peak ")]
    assert len(peaks) == n
    if which == "kuka":
        prob = capi.make_problem(7, 3, capi.ROBOT_KUKA, capi.F_TRQ_ON, jnt_vel_max=[1.0] * 7, jnt_trq_max=[float(v) for v in TRQ_LIMITS.split()],
                                 jnt_trq_min=[-float(v) for v in TRQ_LIMITS.split()])
        want = new.audit(prob, 0.05)
    for w in peaks:
        p = int(w[1])
        peak = np.array([int(w[2], 16)], dtype=np.uint64).view(np.float64)[0]
        assert int(w[6]) == 1 and int(w[8]) == rows[p].shape[1] and int(w[10]) == 7
        if which == "kuka":
            got = want[p]["fam"][capi.AUDIT_TRQ]
            assert peak >= 0.0 and peak.tobytes() == got["peak"].tobytes() and (int(w[3]), int(w[4])) == (int(got["at"]), int(got["row"]))
        else:
            assert peak == -1.0          # the configuration has no torque range: the family stays off
    new.close(); capi_out.close()
    # off: the joint and Cartesian rows are the same, and there are no torque rows
    r = subprocess.run([driver, "config.dat", str(n), "off"] + extra, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    off = read_dump(tmp_path / "dump.bin")
    for k in range(n):
        assert off[k][:3] == (nT, nC, 0) and off[k][3] == on[k][3]
        assert off[k][4].tobytes() == on[k][4][:nT + nC].tobytes()
    assert all(ln.split()[10] == "0" and ln.split()[2] == "bff0000000000000" for ln in r.stdout.splitlines() if ln.startswith("trq_peak "))


def test_batch_driver_prints_the_torque_peaks(tmp_path):
    exe = os.path.join(HOST, "_build", "batest_batch")
    assert os.path.exists(exe), "build() must produce batest_batch"
    stage_kuka(tmp_path)
    r = subprocess.run([exe, "config.dat", "3", "--torques", "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("torques: path ")]
    assert len(lines) == 3 and all(" trq 0." in ln or " trq 1." in ln for ln in lines), r.stdout[-2000:]
    assert any(ln.startswith("audit (tol 0):") and (" trq 0." in ln or " trq 1." in ln) for ln in r.stdout.splitlines())
    r = subprocess.run([exe, "config.dat", "2", "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0 and "torques:" not in r.stdout and " trq -" in r.stdout
    # a robot type without a dynamics model
    stage_gen7dof(tmp_path)
    r = subprocess.run([exe, "config.dat", "2", "--torques"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "no dynamics model" in r.stdout, r.stdout[-2000:]
