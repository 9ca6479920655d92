"""GPU (-m gpu): the tool point of a kinematic chain (include/batotp_hip_kin.h) on the device -- the known-answer entry against
the plain-Python restatement (tests/kin_reference.py) bit for bit, the argument refusals, the resampler and the whole pipeline
on a UR joint path with a Cartesian speed limit (a configuration that was refused before), the chain against the KUKA closed
form in the output stage, and the C++ route through BA::optimizeBatch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import kin_reference as kr
from batotp_amd import capi

pytestmark = pytest.mark.gpu

HOST = os.path.join(helpers.ROOT, "batotp_amd", "host")
CSRC = os.path.join(helpers.ROOT, "batotp_amd", "csrc")
ERR_ARG = "code -1"


def to_capi(ch: kr.Chain) -> capi.KinChain:
    return capi.make_kin_chain(ch.axis, ch.off, ch.tool, ch.degrees)


# ---- 1. the known-answer entry ------------------------------------------------------------------------------------------------
RAGGED = (1, 5, 257, 64)     # 257 crosses the 256-lane block, and the boundary to the next path lies inside a block


@pytest.mark.parametrize("n_links", [1, 2, 6, 7, 8])
@pytest.mark.parametrize("degrees", [True, False])
def test_fwdkin_chain_equals_the_restatement(hip_ctx, n_links, degrees):
    """one ragged call of 4 paths; angles over +-400 degrees with exact 0 and +-90 among them.  Host trig: bit for bit.  Device
    libm: within 1e-12 m, the bound tests/test_gpu_output.py::test_forward_kinematics_with_the_device_libm_is_close uses for the
    tool point"""
    rng = np.random.default_rng(1000 + 10 * n_links + int(degrees))
    ch = kr.random_chain(rng, n_links, degrees)
    thetas = [kr.edge_angles(rng, n_links, n, degrees) for n in RAGGED]
    want = [kr.tool_points(ch, th) for th in thetas]
    got = capi.fwdkin_chain(hip_ctx, to_capi(ch), thetas, host_trig=True)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (n_links, degrees, p, np.abs(g - w).max())
    got = capi.fwdkin_chain(hip_ctx, to_capi(ch), thetas, host_trig=False)
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
    print(f"fwdkin_chain, device libm, {n_links} links, degrees={degrees}: max |difference| {err:.3e} m")
    assert err < 1e-12


def test_fwdkin_chain_builtin_chains(hip_ctx, hip_lib):
    rng = np.random.default_rng(5)
    for name, rid in (("KUKA", capi.ROBOT_KUKA), ("RR", capi.ROBOT_RR), ("UR", capi.ROBOT_UR)):
        ch = hip_lib.builtin_kin_chain(rid)
        ref = kr.builtin(name)
        th = kr.edge_angles(rng, ref.n_links, 300, True)
        got = capi.fwdkin_chain(hip_ctx, ch, [th, th[:, :0], th[:, :3]])      # an empty point list in the middle
        want = kr.tool_points(ref, th)
        assert got[0].tobytes() == want.tobytes() and got[1].shape == (3, 0) and got[2].tobytes() == want[:, :3].tobytes(), name


# ---- 2. argument refusals -----------------------------------------------------------------------------------------------------
def ur_params(flags=capi.F_CART_VEL_ON | capi.F_HOST_TRIG):
    """the golden UR5 configuration as a JOINT path with three Cartesian channels"""
    prm = capi.ResampleParams.from_buffer_copy(bytes(helpers.ResampleCase("UR5").params))
    prm.path_type, prm.n_cart, prm.robot_type, prm.flags = capi.PATH_JOINT, 3, capi.ROBOT_UR, flags
    return prm


def test_argument_refusals(hip_ctx, hip_lib):
    ur = kr.builtin("UR")
    th = [np.zeros((6, 4))]
    x = [np.zeros((9, 8))]
    x[0][:6] = np.linspace(0.0, 30.0, 8)

    def refused(fn, match):
        with pytest.raises(capi.BatotpError, match=ERR_ARG) as e:
            fn()
        assert match in str(e.value), str(e.value)

    def broken(edit):
        c = to_capi(ur)
        edit(c)
        return c

    bad = {"unit vector": broken(lambda c: c.axis[2].__setitem__(1, -1.0 - 1e-9)),
           "not finite": broken(lambda c: c.off[4].__setitem__(0, float("nan"))),
           "1 to 8 links, not 0": broken(lambda c: setattr(c, "n_links", 0)),
           "1 to 8 links, not 9": broken(lambda c: setattr(c, "n_links", 9))}
    b3 = capi.Batch(hip_ctx, capi.make_problem(6, 3, capi.ROBOT_UR, capi.F_CART_VEL_ON, [160] * 6, [573] * 6, cart_vel_max=0.2), [8], 64)
    for match, c in bad.items():
        refused(lambda: capi.fwdkin_chain(hip_ctx, c, [np.zeros((c.n_links, 4))]), match)
        refused(lambda: capi.Resampled(hip_ctx, ur_params(), x, [0.2], chain=c), match)
        refused(lambda: b3.set_kin_chain(c), match)
    # an axis off by less than the tolerance of the check is a unit vector
    capi.fwdkin_chain(hip_ctx, broken(lambda c: c.axis[2].__setitem__(1, -1.0 - 1e-13)), th)
    good = to_capi(ur)
    prm = ur_params(); prm.n_cart = 6
    refused(lambda: capi.Resampled(hip_ctx, prm, [np.zeros((12, 8))], [0.2], chain=good), "3 Cartesian rows")
    prm = ur_params(); prm.path_type = capi.PATH_CART
    refused(lambda: capi.Resampled(hip_ctx, prm, x, [0.2], chain=good), "JOINT paths")
    prm = ur_params(); prm.path_type = capi.PATH_BOTH
    refused(lambda: capi.Resampled(hip_ctx, prm, x, [0.2], chain=good), "JOINT paths")
    refused(lambda: capi.Resampled(hip_ctx, ur_params(), x, [0.2], chain=to_capi(kr.builtin("KUKA"))), "7 links")
    b0 = capi.Batch(hip_ctx, capi.make_problem(6, 0, capi.ROBOT_GENJNT, 0, [160] * 6, [573] * 6), [8], 64)
    refused(lambda: b0.set_kin_chain(good), "Cartesian channels")
    refused(lambda: b3.set_kin_chain(to_capi(kr.builtin("RR"))), "2 links")
    b3.set_kin_chain(good)
    b0.close(); b3.close()


# ---- 3. / 4. a UR arm taught in joint space, with a tool-speed limit ----------------------------------------------------------------
def ur_taught():
    """the 185 taught joint rows of the golden UR5 path and two variants (joint excursion about the first point x 0.5, x 1.5)"""
    d = np.loadtxt(os.path.join(helpers.GOLD, "UR5", "trajUR.csv"), delimiter=",", skiprows=1)
    th = d[:, 1:7].T
    xs = []
    for f in (1.0, 0.5, 1.5):
        x = np.zeros((9, th.shape[1]))
        x[:6] = th[:, :1] + f * (th - th[:, :1])
        xs.append(x)
    return xs


@pytest.fixture(scope="module")
def ur_knots(hip_ctx, hip_lib):
    """the resampled knots of the three paths, computed once for the tests below: (knots, sres, checksums of the call)"""
    chain = hip_lib.builtin_kin_chain(capi.ROBOT_UR)
    xs = ur_taught()
    sres_in = helpers.ResampleCase("UR5").sres_in
    rs = capi.Resampled(hip_ctx, ur_params(), xs, [sres_in] * 3, chain=chain)
    out = {"status": rs.status.copy(), "n": rs.n_knots.copy(), "sres": rs.sres.copy(), "sums": rs.checksums(),
           "y": [rs.knots(p) for p in range(3)], "xs": xs, "sres_in": sres_in, "chain": chain}
    rs.close()
    return out


def test_resampler_ur_joint_path_with_a_cartesian_limit(hip_ctx, ur_knots):
    k = ur_knots
    print("UR joint paths: knots", list(k["n"]), "status", list(k["status"]), "sres", list(k["sres"]))
    assert not k["status"].any() and (k["n"] >= 4).all()
    assert len(set(int(n) for n in k["n"])) > 1          # a ragged batch
    ref = kr.builtin("UR")
    for p, y in enumerate(k["y"]):
        assert y.shape == (9, int(k["n"][p])) and np.isfinite(y).all()
        want = kr.tool_points(ref, y[:6])          # the kinematics runs after the last pass (reference ba.cpp:626-628)
        assert y[6:9].tobytes() == want.tobytes(), (p, np.abs(y[6:9] - want).max())
    again = capi.Resampled(hip_ctx, ur_params(), k["xs"], [k["sres_in"]] * 3, chain=k["chain"])
    assert np.array_equal(again.checksums(), k["sums"]) and k["sums"].all()
    assert np.array_equal(again.n_knots, k["n"])
    again.close()
    # without a chain the configuration is refused, as before
    with pytest.raises(capi.BatotpError, match=ERR_ARG):
        capi.Resampled(hip_ctx, ur_params(), k["xs"], [k["sres_in"]] * 3)


def test_resampler_device_libm_is_close(hip_ctx, ur_knots):
    """without BATOTP_F_HOST_TRIG: the documented tolerance mode (same bound as the KUKA closed form's test: knots within 1e-9)"""
    k = ur_knots
    rs = capi.Resampled(hip_ctx, ur_params(capi.F_CART_VEL_ON), k["xs"], [k["sres_in"]] * 3, chain=k["chain"])
    assert not rs.status.any() and np.array_equal(rs.n_knots, k["n"])
    for p in range(3):
        assert np.max(np.abs(rs.knots(p) - k["y"][p])) < 1e-9
    rs.close()


def ur_problem():
    prob = capi.Problem.from_buffer_copy(bytes(helpers.Case("UR5").problem))
    assert prob.cart_vel_max == 0.2 and prob.n_joints == 6           # the golden UR5 config's tool-speed limit
    prob.n_cart, prob.robot_type = 3, capi.ROBOT_UR
    prob.flags = capi.F_JNT_ACC_ON | capi.F_CART_VEL_ON | capi.F_HOST_TRIG
    return prob


def test_end_to_end_on_those_knots(hip_ctx, ur_knots):
    """precompute, both sweeps, set_kin_chain, output, audit.  The figures printed are a record, not a threshold."""
    k = ur_knots
    prob = ur_problem()
    n = [int(v) for v in k["n"]]
    b = capi.Batch(hip_ctx, prob, n, 8 * max(n) + 4096)
    b.upload_knots(0, k["y"], list(k["sres"]))
    b.precompute(0)
    b.sweep(-1); b.sweep(+1)
    res = b.results()
    prm = capi.OutputParams(6, capi.PATH_JOINT, prob.integ_res, prob.integ_res, 1.0)
    # without the chain the stage has no tool point for this robot: joint rows only
    plain = capi.Output(b, prm, 0, 3)
    assert (plain.n_theta, plain.n_cart, plain.n_trq) == (6, 0, 0)
    b.set_kin_chain(k["chain"])
    out = capi.Output(b, prm, 0, 3)
    assert (out.n_theta, out.n_cart, out.n_trq) == (6, 3, 0) and out.n_rows == 9
    audit = out.audit(prob)
    ref = kr.builtin("UR")
    for p in range(3):
        r = res[p]
        assert int(r["status_rev"]) == 0 and int(r["status_fwd"]) == 0, (p, r)
        assert np.isfinite(r["t_total"]) and r["t_total"] > 0
        rows = out.rows(p)
        assert rows.shape == (9, int(out.n_pts[p])) and int(out.n_pts[p]) >= 4
        assert np.array_equal(np.asarray(plain.n_pts), np.asarray(out.n_pts)) and rows[:6].tobytes() == plain.rows(p).tobytes()
        a = audit[p]
        assert int(a["n_nonfinite"]) == 0 and int(a["n_pts"]) == int(out.n_pts[p])
        cv, jv = float(a["fam"][capi.AUDIT_CART_VEL]["peak"]), float(a["fam"][capi.AUDIT_JNT_VEL]["peak"])
        assert np.isfinite(cv) and cv > 0 and np.isfinite(jv) and jv > 0
        print(f"UR joint path {p}: knots {n[p]}, T = {float(r['t_total']):.6f} s, steps rev/fwd {int(r['steps_rev'])}/{int(r['steps_fwd'])}, "
              f"output points {int(out.n_pts[p])}, peak CART_VEL {cv:.6f}, peak JNT_VEL {jv:.6f}, over {int(a['n_over'])}")
    # no smoothing, no re-interpolation (out_res = the step): the Cartesian rows ARE the chain's tool point of the joint rows
    rows = out.rows(0)
    assert rows[6:9].tobytes() == kr.tool_points(ref, rows[:6]).tobytes()
    plain.close(); out.close(); b.close()


# ---- 5. the chain against the closed form in the output stage ---------------------------------------------------------------------
def run_both(hip_ctx, case, prm, serial_model=None):
    """(results, Output) of the case as robot KUKA, and as robot GENJNT with the built-in KUKA chain"""
    got = []
    for chain in (False, True):
        prob = capi.Problem.from_buffer_copy(bytes(case.problem))
        if chain:
            prob.robot_type = capi.ROBOT_GENJNT
        b = capi.Batch(hip_ctx, prob, [case.n], case.max_steps())
        b.upload_knots(0, [case.y], [case.sres])
        helpers.precompute_with_trig(hip_ctx, b, prob, 1, serial_model=serial_model)
        b.sweep(-1); b.sweep(+1)
        if chain:
            b.set_kin_chain(hip_ctx.library.builtin_kin_chain(capi.ROBOT_KUKA))
        got.append((b.results(), capi.Output(b, prm, 0, 1), b))
    return got


def compare_chain_with_closed_form(got, n_trq):
    (res_a, out_a, b_a), (res_b, out_b, b_b) = got
    assert res_a.tobytes() == res_b.tobytes() and int(res_a[0]["status_fwd"]) == 0
    assert (out_b.n_theta, out_b.n_cart, out_b.n_trq) == (out_a.n_theta, out_a.n_cart, out_a.n_trq) == (7, 3, n_trq)
    assert np.array_equal(out_a.n_pts, out_b.n_pts) and int(out_a.n_pts[0]) >= 4
    ra, rb = out_a.rows(0), out_b.rows(0)
    assert ra[:7].tobytes() == rb[:7].tobytes()
    err = float(np.abs(ra[7:10] - rb[7:10]).max())
    print(f"chain vs closed form, {int(out_a.n_pts[0])} output points: Cartesian rows differ by {err:.3e} m")
    # the per-point bound of the CPU test (1e-13) through a moving average (no growth) and a cubic re-interpolation (norm < 2),
    # with a margin of about ten
    assert err <= 1e-12
    if n_trq:
        assert ra[10:].tobytes() == rb[10:].tobytes()
    for _, o, b in got:
        o.close(); b.close()


@pytest.mark.parametrize("out_res, smooth", [(0.008, 5.0), (0.002, 1.0)])
def test_chain_against_the_kuka_closed_form_in_the_output_stage(hip_ctx, out_res, smooth):
    case = helpers.Case("KUKA-LWR-IV")
    prm = capi.OutputParams(7, capi.PATH_JOINT, case.problem.integ_res, out_res, smooth)   # smoothing; re-interpolation
    compare_chain_with_closed_form(run_both(hip_ctx, case, prm), 0)


def test_chain_with_the_serial_torque_recomputation(hip_ctx, hip_lib):
    """a batch that also recomputes serial torques with a chain model: the trig tables of both share the stage's scratch"""
    case = helpers.Case("KUKA_trq")
    case.y = np.ascontiguousarray(case.y[:, :max(40, case.n // 3)])
    prm = capi.OutputParams(7, capi.PATH_JOINT, case.problem.integ_res, 0.008, 5.0)
    compare_chain_with_closed_form(run_both(hip_ctx, case, prm, serial_model=hip_lib.builtin_serial_model(capi.ROBOT_KUKA)), 7)


# ---- 6. the C++ route ---------------------------------------------------------------------------------------------------------
def test_optimize_batch_on_a_ur_joint_path(tmp_path, hip_ctx):
    """BA::optimizeBatch with setSerialModel + setToolPoint (tests/drivers/kin_batch_main.cpp, linked with the HIP library) returns
    0 and writes its files; the same program without setToolPoint is refused with the message of the device resampler"""
    exe = tmp_path / "kin_batch"
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", f"-I{HOST}", f"-I{helpers.ROOT}/include",
           os.path.join(helpers.ROOT, "tests", "drivers", "kin_batch_main.cpp"), os.path.join(HOST, "_build", "libbatotp.a"), f"-L{CSRC}",
           "-lbatotp_hip", f"-Wl,-rpath,{CSRC}", "-pthread", "-lm", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    src = os.path.join(helpers.GOLD, "UR5")
    lines = open(os.path.join(src, "trajUR.csv")).read().splitlines()
    with open(tmp_path / "ur_joint.csv", "w") as f:
        for ln in lines:
            if ln.strip():
                f.write(", ".join(c.strip() for c in ln.split(",")[:10]) + "\n")
    config = open(os.path.join(src, "config.dat")).read()
    for old, new in (("6        // nCart", "3        // nCart"), ("trajUR.csv", "ur_joint.csv"), ("BOTH     // pathType", "JOINT    // pathType")):
        assert old in config
        config = config.replace(old, new)
    (tmp_path / "config.dat").write_text(config)
    r = subprocess.run([str(exe), "config.dat", "2", "--tool"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0 and "optimizeBatch 0" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for p in range(2):
        path = tmp_path / f"out_{p}" / "traj_out.dat"
        assert path.exists()
        sres, n, theta, cart, trq = helpers.read_traj_out(str(path), 6, 3)
        assert n >= 4 and cart is not None and cart.shape == (3, n) and np.isfinite(cart).all() and np.isfinite(theta).all() and trq is None
        # the written tool point is the chain's tool point of the written joints, to the precision of the file (float32)
        want = kr.tool_points(kr.builtin("UR"), theta.astype(np.float64))
        assert np.abs(want - cart).max() < 1e-4
    # ... and the same path alone through the step-by-step calls of BA::optimize gives the same file
    assert "optimize 0" in r.stdout
    assert open(tmp_path / "out_single" / "traj_out.dat", "rb").read() == open(tmp_path / "out_0" / "traj_out.dat", "rb").read()
    r = subprocess.run([str(exe), "config.dat", "2"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 4 and "optimizeBatch -1" in r.stdout and "not covered by the device resampler" in r.stdout, r.stdout[-3000:]
