"""GPU (-m gpu): the continuous torque rating of finished trajectories (include/batotp_hip_duty.h) against tests/duty_reference.py on
the same rows.  With host trig tables the tolerance is 0: the sums the kernels write are compared bit for bit, the records with the
host rule applied to them, rows as uint64, reports as bytes.  Shapes enter through capi.output_from_rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import duty_reference as du
import dyn_reference as dr
import invdyn_reference as ir
import stretch_reference as sr
import tscale_reference as tr
from audit_reference import assert_audit_equal
from batotp_amd import capi
from test_duty_cpu import EDGES, ratings_for, synth
from test_gpu_invdyn import H, model_named

pytestmark = pytest.mark.gpu

BP = capi.DUTY_BLOCK_POINTS
ERR_ARG = -1      # BATOTP_ERR_ARG
assert EDGES == [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 3 * 128 + 5] and BP == 128
AMPS = [0, 1.0, 1.0, 1.0, 2.0, 0.5, 3.0, 0.9, 1.5, 2.5, 4.0, 1.2]
# device libm against host trig tables, relative: test_device_libm prints the measured figures (DESIGN.md 2 records them: 1.2e-16
# for the RMS torques relative to each joint's largest, 0 for the energy on the MI355X); 100 x the measured maximum, rounded up to a
# power of ten
DEVICE_LIBM_BOUND = 1e-13

MODELS = {"rr": lambda lib: model_named(lib, "rr"), "kuka": lambda lib: model_named(lib, "kuka"),
          "chain1deg": lambda lib: dr.random_chain(1, True), "chain8rad": lambda lib: dr.random_chain(8, False)}
_KNOWN = {}


def known(oracle_lib, name, n_cart=0):
    """(model, rows, sres, rows with torques, duty records at the batch's ratings, sums, ratings) of the ragged batch -- computed once,
    shared, never modified"""
    key = (name, n_cart)
    if key not in _KNOWN:
        model = MODELS[name](oracle_lib)
        nl = model.n_links
        rng = np.random.default_rng(3 + n_cart)
        rows = [np.ascontiguousarray(np.concatenate([r, rng.uniform(-1.0, 1.0, (n_cart, r.shape[1]))])) for r in tr.synth_rows(model, EDGES, AMPS)]
        sres = tr.synth_steps(len(rows))
        raw = du.duty(oracle_lib, model, rows, sres, [1.0] * nl)[2]
        rated = ratings_for(raw[-1], nl, 1.3)          # the long path is over its rating, others are inside theirs
        want, rec, raw = du.duty(oracle_lib, model, rows, sres, rated, 1.0)
        for a in rows + want:
            a.setflags(write=False)
        _KNOWN[key] = (model, rows, sres, want, rec, raw, rated)
    return _KNOWN[key]


def check_rows(new, want, what):
    got = new.all_rows()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        ir.assert_rows_bit_equal(g, w, f"{what}, path {k}")


# ---- 1. ragged batches: the wavefront and block edges of the tree -----------------------------------------------------------
@pytest.mark.parametrize("name,n_cart", [("rr", 0), ("kuka", 0), ("kuka", 3), ("chain1deg", 0), ("chain8rad", 0)])
def test_ragged_batch(hip_ctx, oracle_lib, name, n_cart):
    model, rows, sres, want, rec, raw, rated = known(oracle_lib, name, n_cart)
    nl = model.n_links
    assert float(rec["util"].max()) > 1.0 and (rec["util"][1:] > 0).all() and np.isfinite(rec["s"]).any()
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, n_cart, 0)
    new, got, sums = out.duty(model, rated, 1.0, sums=True)
    assert (new.n_theta, new.n_cart, new.n_trq, new.n_rows) == (nl, n_cart, nl, 2 * nl + n_cart)
    assert [int(n) for n in new.n_pts] == EDGES and new.sres.tobytes() == sres.tobytes()
    du.assert_sums_equal(sums, raw, f"sums {name}")
    assert sums.tobytes() == raw.tobytes()
    # the records are the host rule applied to the sums
    for k in range(len(rows)):
        du.assert_duty_equal(got[k:k + 1], np.array([du.duty_record(sums[k], nl, rated, 1.0, sres[k])]), f"host rule {name} path {k}")
    du.assert_duty_equal(got, rec, f"records {name}")
    assert got.tobytes() == rec.tobytes()
    assert (int(got[0]["n_pts"]), float(got[0]["util"]), int(got[0]["row"]), float(got[0]["peak_power"]), int(got[0]["power_at"])) == (0, -1.0, -1, -np.inf, -1)
    assert not sums[0]["S"].any() and float(sums[0]["W"]) == 0.0
    # the torque rows are those of the torque kernel, and of the reference
    trq = out.torques(model)
    for k, (g, w) in enumerate(zip(new.all_rows(), trq.all_rows())):
        assert g.tobytes() == w.tobytes(), f"path {k}"
    check_rows(new, want, name)
    assert new.duty_ms() >= 0.0 and new.duty_ranges() == 1
    # another target and no sums: the same call, the host rule alone differs
    again, got2 = out.duty(model, rated, 0.7)
    for k in range(len(rows)):
        du.assert_duty_equal(got2[k:k + 1], np.array([du.duty_record(raw[k], nl, rated, 0.7, sres[k])]), f"target 0.7 {name} path {k}")
    with pytest.raises(capi.BatotpError):
        new.tscale_ms()
    with pytest.raises(capi.BatotpError):
        out.duty_ms()
    for k, (g, r) in enumerate(zip(out.all_rows(), rows)):
        assert g.tobytes() == r.tobytes(), k
    for o in (new, again, trq, out):
        o.close()


# ---- 2. the same bits however it is cut -------------------------------------------------------------------------------------
def test_same_bits_under_a_workspace_budget(hip_lib, oracle_lib):
    model, rows, sres, want, rec, raw, rated = known(oracle_lib, "kuka", 3)
    nl = model.n_links
    ctx = capi.Context(hip_lib, 0)          # a context of its own: the budget is a property of the context
    out = capi.output_from_rows(ctx, rows, sres, nl, 3, 0)
    whole, rec0, raw0 = out.duty(model, rated, sums=True)
    assert whole.duty_ranges() == 1
    flat = [r.copy() for r in whole.all_rows()]
    ctx.set_workspace_budget(0, 8 * 3 * nl * (BP + 2))          # room for the tables of about one block-sized path
    cut, rec1, raw1 = out.duty(model, rated, sums=True)
    assert 3 <= cut.duty_ranges() < len(rows), cut.duty_ranges()
    ctx.set_workspace_budget(0, 1)          # every path a range of its own; a range of empty paths launches nothing
    each, rec2, raw2 = out.duty(model, rated, sums=True)
    assert each.duty_ranges() == sum(1 for n in EDGES if n > 0)
    for o, r, s, what in ((cut, rec1, raw1, "under a budget"), (each, rec2, raw2, "a range per path")):
        for k, (g, w) in enumerate(zip(o.all_rows(), flat)):
            assert g.tobytes() == w.tobytes(), (what, k)
        assert s.tobytes() == raw0.tobytes() == raw.tobytes() and r.tobytes() == rec0.tobytes() == rec.tobytes(), what
    ctx.set_workspace_budget(0, 0)
    for o in (whole, cut, each, out):
        o.close()


# ---- 3. values that are not finite ------------------------------------------------------------------------------------------
def test_values_that_are_not_finite(hip_ctx, oracle_lib):
    model = model_named(oracle_lib, "kuka")
    nl = model.n_links
    base = tr.synth_rows(model, [BP + 40, BP + 40, BP + 40, 70], [1.0, 1.0, 1.0, 1.0])
    rows = [r.copy() for r in base]
    rows[0][2, BP] = np.nan          # the stencil of the NaN straddles the block edge
    rows[1][4, 17] = np.inf
    sres = [H] * 4
    rated = [1e3] * nl
    want, rec, raw = du.duty(oracle_lib, model, rows, sres, rated)
    clean = du.duty(oracle_lib, model, base, sres, rated)[2]
    # at the point of the NaN every A and G is NaN (the recursion passes through joint 2), and so is every moment but B*B of the
    # other joints, whose friction torque does not know of joint 2
    assert np.isnan(raw[0]["S"][:nl][:, [0, 1, 3, 4, 5, 6]]).all() and np.isnan(raw[0]["S"][2, 2]) and np.isfinite(raw[0]["S"][0, 2])
    assert np.isnan(raw[1]["S"][:nl][:, [0, 1, 3, 4, 5, 6]]).all() and not np.isfinite(raw[1]["S"][4, 2])
    for k in (2, 3):
        assert raw[k].tobytes() == clean[k].tobytes() and np.isfinite(raw[k]["S"]).all()
    # the peak power of the poisoned path is that of the clean path's points outside the stencil
    p = du.point_values(oracle_lib, model, base[0][:nl], H)[1]
    keep = np.ones(BP + 40, dtype=bool)
    keep[BP - 1:BP + 2] = False
    assert float(raw[0]["peak_power"]) == p[keep].max() and int(raw[0]["power_at"]) == int(np.flatnonzero(keep & (p == p[keep].max()))[0])
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    new, got, sums = out.duty(model, rated, sums=True)
    du.assert_sums_equal(sums, raw, "NaN and Inf")
    du.assert_duty_equal(got, rec, "NaN and Inf")
    assert float(got[0]["util"]) == -1.0 and int(got[0]["row"]) == -1 and np.isnan(got[0]["rms"][:nl]).all()
    for k in (2, 3):
        assert sums[k].tobytes() == clean[k].tobytes()
    new.close(); out.close()
    # a path of all -0.0 under a model without gravity: every value is a zero of either sign, every sum +0.0 (lanes past the end
    # contribute +0.0; a path that fills its blocks keeps what its values give)
    still = dr.weightless(model)
    zrows = [np.full((nl, 5), -0.0), np.full((nl, BP), -0.0)]
    wz, rz, sz = du.duty(oracle_lib, still, zrows, [H, H], rated)
    assert not sz[0]["S"].any() and not np.signbit(sz[0]["S"]).any() and not np.signbit(sz[0]["W"])
    out = capi.output_from_rows(hip_ctx, zrows, [H, H], nl, 0, 0)
    new, got, sums = out.duty(still, rated, sums=True)
    assert sums.tobytes() == sz.tobytes() and got.tobytes() == rz.tobytes()
    assert float(got[0]["util"]) == 0.0 and float(got[0]["energy"]) == 0.0 and float(got[0]["peak_power"]) == 0.0 and int(got[0]["power_at"]) == 0
    new.close(); out.close()


# ---- 4. the rounds ----------------------------------------------------------------------------------------------------------
_ROUNDS = {}


def rounds_case(oracle_lib):
    """tscale_reference's synthetic batch and problem, with ratings from the batch's own sums: several paths are over them, others
    inside, and the gravity torque of joint 1 alone reaches its rating on exactly one path"""
    if not _ROUNDS:
        model, rows, sres, P, V, S = synth(oracle_lib, "kuka")
        nl = model.n_links
        grav = np.array([np.sqrt(s["S"][:nl, 5] / float(s["n_pts"])) for s in S if int(s["n_pts"]) > 0])
        rated = np.maximum(ratings_for(S[3], nl, 1.3), 1.25 * grav.max(axis=0))
        top = np.sort(grav[:, 1])
        rated[1] = 0.5 * (top[-1] + top[-2])
        prob = tr.synth_problem(oracle_lib, model, rows, sres)
        _ROUNDS["c"] = (model, rows, sres, prob, rated, {})
    return _ROUNDS["c"]


ARGS = [(1.0, 8, 16.0), (0.8, 8, 1.75), (1.0, 1, 16.0)]


@pytest.mark.parametrize("args", ARGS, ids=["plain", "cap", "one_round"])
def test_rounds_synthetic_batch(hip_ctx, oracle_lib, args):
    target, max_rounds, max_factor = args
    model, rows, sres, prob, rated, caches = rounds_case(oracle_lib)
    nl = model.n_links
    want, report, final, recs, duties = du.stretch_duty(oracle_lib, model, rows, sres, 0, prob, rated, target, max_rounds, max_factor, caches.setdefault(target, {}))
    st = [int(v) for v in report["status"]]
    if args == ARGS[0]:
        held = [k for k in range(len(rows)) if int(duties[k]["n_hold"]) > 0]
        assert len(held) == 1 and st[held[0]] == capi.STRETCH_STATIC and int(duties[held[0]]["n_hold"]) == 1
        assert set(st) == {capi.STRETCH_PASSES, capi.STRETCH_STATIC} and int(report["rounds"].max()) >= 1
        plain = tr.stretch_torques(oracle_lib, model, rows, sres, 0, prob, target, max_rounds, max_factor)[1]
        assert (report["n_out"] > plain["n_out"]).any(), "the ratings bind beyond the peak torque range"
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    new, got, rec, duty = out.stretch_duty(prob, model, rated, target, max_rounds, max_factor)
    sr.assert_report_equal(got, report, f"report {args}")
    assert [int(n) for n in new.n_pts] == [int(n) for n in report["n_out"]] and (new.n_theta, new.n_cart, new.n_trq) == (nl, 0, nl)
    check_rows(new, want, f"rounds {args}")
    tr.assert_records_equal(rec, recs, f"scale records {args}")
    du.assert_duty_equal(duty, duties, f"duty records {args}")
    assert duty.tobytes() == duties.tobytes()
    assert_audit_equal(new.audit(tr.with_trq_on(prob), 0.0), final, f"final audit {args}")
    assert new.duty_ranges() == int(report["rounds"].max()) + 1 and new.duty_ms() >= 0.0
    # *out is the torque rows of the stretched output, device against device; the duty records are those of the result's own rows
    long = out.stretch_to(report["n_out"])
    composed = long.torques(model)
    for k, (g, w) in enumerate(zip(new.all_rows(), composed.all_rows())):
        assert g.tobytes() == w.tobytes(), k
    again, duty2 = long.duty(model, rated, target)
    assert duty2.tobytes() == duty.tobytes()
    for k, (g, r) in enumerate(zip(out.all_rows(), rows)):
        assert g.tobytes() == r.tobytes(), k
    for o in (new, long, composed, again, out):
        o.close()


def test_ratings_that_never_bind_are_the_torque_stretch(hip_ctx, oracle_lib):
    model, rows, sres, prob, rated, caches = rounds_case(oracle_lib)
    nl = model.n_links
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    for args in ARGS:
        plain, rep0, rec0 = out.stretch_torques(prob, model, *args)
        new, rep, rec, duty = out.stretch_duty(prob, model, [1e300] * nl, *args)
        assert rep.tobytes() == rep0.tobytes() and rec.tobytes() == rec0.tobytes(), args
        for k, (g, w) in enumerate(zip(new.all_rows(), plain.all_rows())):
            assert g.tobytes() == w.tobytes(), (args, k)
        assert not duty["n_hold"].any() and np.isposinf(duty["s"]).all()
        plain.close(); new.close()
    assert int(rep0["rounds"].max()) >= 1
    out.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(hip_ctx, hip_lib, oracle_lib):
    model, rows, sres, prob, rated, caches = rounds_case(oracle_lib)
    nl = model.n_links
    lib = hip_lib.lib
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    with_trq = capi.output_from_rows(hip_ctx, [np.zeros((nl + 2, 5))], [H], nl, 0, 2)
    six = capi.output_from_rows(hip_ctx, [np.zeros((6, 5))], [H], 6, 0, 0)
    K = len(rows)
    rep, rec = np.zeros(K, dtype=capi.STRETCH_DTYPE), np.zeros(K, dtype=capi.TSCALE_DTYPE)
    dut, raw = np.zeros(K, dtype=capi.DUTY_DTYPE), np.zeros(K, dtype=capi.DUTY_SUMS_DTYPE)
    rp, cp, dp, sp = (a.ctypes.data_as(C.c_void_p) for a in (rep, rec, dut, raw))
    good = np.ascontiguousarray(rated, dtype=np.float64)
    D = C.POINTER(C.c_double)

    def ref(x):
        return C.byref(x) if x is not None else None

    def refused(what, word, o=out, p=prob, m=model, flags=capi.F_HOST_TRIG, r=good, target=1.0, entries=("duty", "rounds")):
        rr = r.ctypes.data_as(D) if r is not None else None
        for entry in entries:
            h = C.c_void_p(0xdead)
            if entry == "duty":
                rc = lib.batotp_hip_output_duty(o.handle if o is not None else None, ref(m), flags, rr, target, C.byref(h), dp, sp)
            else:
                rc = lib.batotp_hip_output_stretch_duty(o.handle if o is not None else None, ref(p), ref(m), flags, rr, target, 8, 16.0, C.byref(h), rp, cp, dp)
            msg = lib.batotp_hip_last_error()
            assert rc == ERR_ARG and h.value is None and msg and word in msg, (what, entry, rc, h.value, msg)

    def model_copy():
        return capi.SerialModel.from_buffer_copy(bytes(model))

    refused("NULL output", b"NULL argument", o=None)
    refused("NULL model", b"NULL argument", m=None)
    refused("NULL ratings", b"NULL argument", r=None)
    refused("NULL problem", b"NULL argument", p=None, entries=("rounds",))
    gd = good.ctypes.data_as(D)
    assert lib.batotp_hip_output_duty(out.handle, C.byref(model), capi.F_HOST_TRIG, gd, 1.0, None, dp, sp) == ERR_ARG
    h = C.c_void_p(0xdead)
    assert lib.batotp_hip_output_duty(out.handle, C.byref(model), capi.F_HOST_TRIG, gd, 1.0, C.byref(h), None, sp) == ERR_ARG and h.value is None
    assert b"NULL argument" in lib.batotp_hip_last_error()
    assert lib.batotp_hip_output_stretch_duty(out.handle, C.byref(prob), C.byref(model), capi.F_HOST_TRIG, gd, 1.0, 8, 16.0, C.byref(h), None, cp, dp) == ERR_ARG
    # what batotp_hip_output_torques refuses
    for bad in (0, -1, 9):
        m = model_copy(); m.n_links = bad
        refused(f"n_links {bad}", b"links", m=m)
    refused("n_links != n_theta", b"joint rows", o=six)
    m = model_copy(); m.link[nl - 1].inertia[1] = np.nan
    refused("inertia NaN", b"not finite", m=m)
    m = model_copy(); m.gravity[0] = np.inf
    refused("gravity", b"gravity", m=m)
    m = model_copy(); m.link[3].axis[0], m.link[3].axis[1], m.link[3].axis[2] = 0.0, 0.0, 1.0 + 1e-11
    refused("axis not a unit vector", b"unit vector", m=m)
    for flags in (capi.F_HOST_TRIG | capi.F_TRQ_ON, capi.F_JNT_ACC_ON, 1 << 31):
        refused(f"flags {flags:#x}", b"only BATOTP_F_HOST_TRIG", flags=flags)
    refused("torque rows already there", b"torque rows", o=with_trq)
    # the ratings and the target
    for j, v in ((0, 0.0), (nl - 1, -1.0), (2, np.nan), (3, np.inf)):
        r = good.copy(); r[j] = v
        refused(f"rating {v}", b"rated torque of joint %d" % j, r=r)
    for target in (0.0, -1.0, 1.0 + 1e-12, np.nan, np.inf):
        refused(f"target {target}", b"target", target=target)
    for rounds, factor, what in ((0, 16.0, "no rounds"), (17, 16.0, "17 rounds"), (8, 0.99, "max_factor < 1"), (8, np.inf, "max_factor Inf")):
        h = C.c_void_p(0xdead)
        rc = lib.batotp_hip_output_stretch_duty(out.handle, C.byref(prob), C.byref(model), capi.F_HOST_TRIG, gd, 1.0, rounds, factor, C.byref(h), rp, cp, dp)
        assert rc == ERR_ARG and h.value is None and b"output_stretch_duty" in lib.batotp_hip_last_error(), what
    # what the torque stretch refuses of the problem
    p = capi.Problem.from_buffer_copy(bytes(prob)); p.flags |= capi.F_PARALLEL
    refused("a parallel mechanism", b"parallel", p=p, entries=("rounds",))
    p = capi.Problem.from_buffer_copy(bytes(prob)); p.jnt_trq_max[2] = np.nan
    refused("torque range", b"torque range of joint 2", p=p, entries=("rounds",))
    assert not any(a.view(np.uint8).any() for a in (rep, rec, dut, raw)), "a refused call writes no record"
    # entries of joints the model does not use are not read; the optional records may be NULL
    one = model_named(oracle_lib, "one")
    o1 = capi.output_from_rows(hip_ctx, [np.zeros((1, 3))], [H], 1, 0, 0)
    r1 = np.array([10.0, np.nan])
    d1 = np.zeros(1, dtype=capi.DUTY_DTYPE)
    h = C.c_void_p()
    assert lib.batotp_hip_output_duty(o1.handle, C.byref(one), capi.F_HOST_TRIG, r1.ctypes.data_as(D), 1.0, C.byref(h), d1.ctypes.data_as(C.c_void_p), None) == 0
    assert h.value and int(d1[0]["n_pts"]) == 3 and 0.0 < float(d1[0]["util"]) < 1.0
    lib.batotp_hip_output_destroy(h)
    p1 = capi.make_problem(1, 0, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0], jnt_trq_max=[10.0], jnt_trq_min=[-10.0])
    rep1 = np.zeros(1, dtype=capi.STRETCH_DTYPE)
    h = C.c_void_p()
    assert lib.batotp_hip_output_stretch_duty(o1.handle, C.byref(p1), C.byref(one), capi.F_HOST_TRIG, r1.ctypes.data_as(D), 1.0, 8, 16.0, C.byref(h),
                                              rep1.ctypes.data_as(C.c_void_p), None, None) == 0
    assert h.value and int(rep1[0]["n_out"]) == 3 and int(rep1[0]["status"]) == capi.STRETCH_PASSES
    lib.batotp_hip_output_destroy(h)
    o1.close()
    # no paths; paths without points
    empty = capi.output_from_rows(hip_ctx, [], [], nl, 0, 0)
    e, d0 = empty.duty(model, rated)
    assert e.n_paths == 0 and (e.n_theta, e.n_cart, e.n_trq) == (nl, 0, nl) and d0.shape == (0,) and e.duty_ranges() == 0 and e.duty_ms() == 0.0
    e2, rep0, r0, d0 = empty.stretch_duty(prob, model, rated)
    assert e2.n_paths == 0 and rep0.shape == (0,) and e2.duty_ranges() == 0
    hollow = capi.output_from_rows(hip_ctx, [np.zeros((nl, 0))] * 3, [H] * 3, nl, 0, 0)
    h_, rep3, r3, d3 = hollow.stretch_duty(prob, model, rated, host_trig=False)
    assert [int(n) for n in h_.n_pts] == [0, 0, 0] and h_.duty_ranges() == 0 and not rep3["status"].any()
    assert [float(v) for v in d3["util"]] == [-1.0] * 3 and all(np.isposinf(d3["s"])) and [int(v) for v in d3["power_at"]] == [-1] * 3
    for o in (e, e2, empty, h_, hollow, out, with_trq, six):
        o.close()


# ---- 6. device libm ---------------------------------------------------------------------------------------------------------
def test_device_libm(hip_ctx, oracle_lib):
    """without BATOTP_F_HOST_TRIG the trig comes from the device libm: rms and energy stay close to the host-trig run of the same batch"""
    model, rows, sres, want, rec, raw, rated = known(oracle_lib, "kuka", 3)
    nl = model.n_links
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 3, 0)
    a, host = out.duty(model, rated, host_trig=True)
    b, dev = out.duty(model, rated, host_trig=False)
    assert host.tobytes() == rec.tobytes()
    live = host["n_pts"] > 0
    # relative to each joint's largest RMS torque over the batch (on a path of one or two points the arm is at rest and the last
    # joint's torque is rounding noise of 1e-18 Nm: no scale of its own -- the measure of test_gpu_invdyn.test_device_libm)
    rms_h, rms_d = host["rms"][live, :nl], dev["rms"][live, :nl]
    scale = rms_h.max(axis=0, keepdims=True)
    assert (scale > 1e-3).all()
    d_rms = float((np.abs(rms_d - rms_h) / scale).max())
    moving = live & (host["energy"] > 0)
    d_en = float((np.abs(dev["energy"][moving] - host["energy"][moving]) / host["energy"][moving]).max())
    print(f"DUTY device libm against host trig tables, kuka batch: largest relative difference of rms {d_rms:.3e}, of energy {d_en:.3e} "
          f"({int(moving.sum())} paths that move); power_at differs on {int((host['power_at'] != dev['power_at']).sum())} paths")
    assert d_rms <= DEVICE_LIBM_BOUND and d_en <= DEVICE_LIBM_BOUND
    assert (dev["energy"][live & ~moving] == 0.0).all() and (dev["n_pts"] == host["n_pts"]).all()
    for o in (a, b, out):
        o.close()


# ---- 7. the host route ------------------------------------------------------------------------------------------------------
def test_host_route(tmp_path):
    """BA::setStretchToRatedTorques on the reference's KUKA example, planned under joint velocity and acceleration limits only"""
    import helpers
    from test_gpu_invdyn import TRQ_LIMITS, stage_kuka
    stage_kuka(tmp_path)
    exe = os.path.join(helpers.ROOT, "batotp_amd", "host", "_build", "batest_batch")
    assert os.path.exists(exe), "build() must produce batest_batch"
    n = 3
    plain = subprocess.run([exe, "config.dat", str(n), "--stretch-torques", "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stdout[-2000:]
    f_plain = float([ln for ln in plain.stdout.splitlines() if ln.startswith("stretch-torques")][0].split("factor")[1].split()[0])
    # ratings far above the peak range change nothing; a tenth of the peak range binds beyond it
    for scale, binds in ((1e6, False), (0.1, True)):
        rated = ",".join(str(float(v) * scale) for v in TRQ_LIMITS.split())
        r = subprocess.run([exe, "config.dat", str(n), "--stretch-duty", rated, "--audit"], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("stretch-duty (target 1):")]
        assert len(lines) == 1 and "stretch-torques" not in r.stdout, r.stdout[-2000:]
        print("DUTY host route:", lines[0])
        w = lines[0].split()
        factor = float(w[w.index("factor") + 1])
        duty = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("duty: path ")]
        assert len(duty) == n, r.stdout[-2000:]
        print("DUTY host route:", " ".join(duty[0]))
        not_passing, static = int(w[w.index("not") - 1]), int(w[-4])
        for d in duty:
            util, energy, peak = float(d[4]), float(d[8]), float(d[10])
            assert util > 0.0 and energy > 0.0 and peak > 0.0
            if not_passing == 0:
                assert util <= 1.0
        if binds:
            assert factor > f_plain or static == n, lines[0]
        else:
            assert factor == f_plain and not_passing == 0, (lines[0], f_plain)
        peaks = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("torques: path ")]
        assert len(peaks) == n
    # without the option nothing changes
    r0 = subprocess.run([exe, "config.dat", str(n), "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r0.returncode == 0 and "stretch-duty" not in r0.stdout and "duty:" not in r0.stdout
