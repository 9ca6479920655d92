"""GPU (-m gpu): finished trajectories stretched until their torque limits pass (include/batotp_hip_tscale.h) against
tests/tscale_reference.py on the same rows.  With host trig tables the tolerance is 0: rows are compared as uint64, records and
reports as bytes.  Known-answer shapes enter through capi.output_from_rows; real trajectories are swept and passed through the
output stage on the device first."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dyn_reference as dr
import helpers
import invdyn_reference as ir
import stretch_reference as sr
import tscale_reference as tr
from audit_reference import audit_reference, assert_audit_equal
from batotp_amd import capi
from test_gpu_invdyn import H, LENGTHS, batch_rows, model_named, one_link_model, stage_kuka, steps  # noqa: F401

pytestmark = pytest.mark.gpu

BP = capi.TSCALE_BLOCK_POINTS
assert BP == capi.INVDYN_BLOCK_POINTS and LENGTHS == [4, 0, 1, 2, 3, BP - 1, BP, BP + 1, 2 * BP + 1]
ERR_ARG = -1      # BATOTP_ERR_ARG
HOST = os.path.join(helpers.ROOT, "batotp_amd", "host")
SMOOTH_AMPS = [1.0, 0, 1.0, 1.0, 2.0, 0.9, 2.5, 4.0, 0.5]


def check_rows(new, want, what):
    got = new.all_rows()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        ir.assert_rows_bit_equal(g, w, f"{what}, path {k}")


# ---- 1. known answers of torque_scale --------------------------------------------------------------------------------------
_KNOWN = {}


def known_pieces(oracle_lib, name, n_cart, kind):
    """(model, rows, sres, rows with torques, pieces per path) of the ragged batch -- computed once, shared, never modified"""
    key = (name, n_cart, kind)
    if key not in _KNOWN:
        model = model_named(oracle_lib, name)
        nl = model.n_links
        if kind == "random":
            rows = batch_rows(model, n_cart)
        else:
            rng = np.random.default_rng(7 + n_cart)
            rows = [np.ascontiguousarray(np.concatenate([r, rng.uniform(-1.0, 1.0, (n_cart, r.shape[1]))])) for r in tr.synth_rows(model, LENGTHS, SMOOTH_AMPS)]
        sres = steps(rows)
        P = [tr.pieces(oracle_lib, model, r[:nl], sres[k]) for k, r in enumerate(rows)]
        with np.errstate(all="ignore"):
            want = [np.concatenate([r, (A + B) + G]) for r, (A, B, G) in zip(rows, P)]
        for a in rows + want:
            a.setflags(write=False)
        _KNOWN[key] = (model, rows, sres, want, P)
    return _KNOWN[key]


def range_of(P, nl, scale):
    """a torque range from the pieces of the batch: gravity fits into it everywhere and the motion of the last path does not; with
    scale < 1, a fraction of what gravity alone asks for"""
    gmax = np.max([np.abs(G).max(axis=1) for A, B, G in P if G.shape[1]], axis=0)
    A, B, G = P[-1]
    tmax = 1.1 * gmax + 0.5 * np.abs(A + B).max(axis=1) + 1e-3 if scale == 1.0 else scale * gmax + 1e-3
    return [float(v) for v in tmax], [float(v) for v in -(0.8 * tmax + 0.3 * gmax)]


@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("n_cart", [0, 3])
@pytest.mark.parametrize("name", ["kuka", "rr", "random8", "one"])
def test_known_answers(hip_ctx, oracle_lib, name, n_cart, kind):
    model, rows, sres, want, P = known_pieces(oracle_lib, name, n_cart, kind)
    nl = model.n_links
    if kind == "random":
        for g, w in zip(want, ir.with_torques(oracle_lib, model, rows, sres, n_cart)):
            ir.assert_rows_bit_equal(g, w, "the addends sum to the pinned torque rows")
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, n_cart, 0)
    seen_static = seen_root = False
    for scale, target in ((1.0, 1.0), (1.0, 0.7), (0.5, 1.0)):      # a range that binds; a tighter target; gravity outside it somewhere
        tmax, tmin = range_of(P, nl, scale)
        prob = capi.make_problem(nl, n_cart, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0] * nl, jnt_trq_max=tmax, jnt_trq_min=tmin)
        hi, lo = tr.bounds(prob, nl, target)
        ref = np.zeros(len(rows), dtype=capi.TSCALE_DTYPE)
        for k, (A, B, G) in enumerate(P):
            ref[k] = tr.scale_record(A, B, G, hi, lo)
        new, rec = out.torque_scale(prob, model, target)
        assert (new.n_theta, new.n_cart, new.n_trq, new.n_rows) == (nl, n_cart, nl, 2 * nl + n_cart)
        assert [int(n) for n in new.n_pts] == LENGTHS and new.sres.tobytes() == sres.tobytes()
        check_rows(new, want, f"{name}, n_cart {n_cart}, {kind}")
        tr.assert_records_equal(rec, ref, f"{name}, n_cart {n_cart}, {kind}, scale {scale}, target {target}")
        assert new.tscale_ms() >= 0.0 and new.tscale_ranges() == 1
        with pytest.raises(capi.BatotpError):
            new.torques_ms()
        seen_static |= bool(ref["n_static"].any())
        seen_root |= bool((ref["at"] >= 0).any())
        assert [int(r["at"]) for r in ref[1:4]] == [-1] * 3 and all(np.isinf(ref["s"][1:4]))      # no points, or too few to move
        new.close()
    assert seen_static and seen_root
    # the input is untouched, and it is not a result of the call
    for k, (g, r) in enumerate(zip(out.all_rows(), rows)):
        assert g.tobytes() == r.tobytes(), k
    with pytest.raises(capi.BatotpError):
        out.tscale_ms()
    out.close()


@pytest.mark.parametrize("host_trig", [True, False], ids=["host_trig", "device_libm"])
def test_rows_are_those_of_the_torque_rows(hip_ctx, oracle_lib, host_trig):
    """k_tscale and k_invdyn run one body for a point: on the same output their rows are the same bytes, whichever trig they read"""
    model, rows, sres, want, P = known_pieces(oracle_lib, "kuka", 3, "smooth")
    nl = model.n_links
    tmax, tmin = range_of(P, nl, 1.0)
    prob = capi.make_problem(nl, 3, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0] * nl, jnt_trq_max=tmax, jnt_trq_min=tmin)
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 3, 0)
    new, rec = out.torque_scale(prob, model, host_trig=host_trig)
    trq = out.torques(model, host_trig=host_trig)
    got, ref = new.all_rows(), trq.all_rows()
    assert [r.shape for r in got] == [(2 * nl + 3, n) for n in LENGTHS] == [r.shape for r in ref]
    for k, (g, w) in enumerate(zip(got, ref)):
        assert g.tobytes() == w.tobytes(), f"path {k}"
    assert sum(r.size for r in got) > 0 and all(np.isfinite(r).all() for r in got)
    for o in (new, trq, out):
        o.close()


# ---- 2. steered roots ------------------------------------------------------------------------------------------------------
def steered_paths():
    """one weightless link (G = 0, tau = J qdd + fv qd): short paths whose binding candidate is known by construction"""
    i = np.arange(40, dtype=np.float64)
    up = 0.5 * 30.0 * (i * H) ** 2                       # speeding up in the positive direction: the upper bound
    ramp = i * 2.0 ** -6                                 # exact in binary64: second differences are 0, A = 0
    rest = np.full(40, 0.3)
    base = 0.8 * np.sin(2.0 * np.pi * np.arange(BP) / BP)
    return {"upper": up, "lower": -up, "linear": ramp, "none": rest, "short": np.array([0.1, 0.9]), "base": base}


def test_steered_roots(hip_ctx, oracle_lib):
    model = dr.weightless(one_link_model())
    paths = steered_paths()
    prob = capi.make_problem(1, 0, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0], jnt_trq_max=[1.5], jnt_trq_min=[-1.0])
    hi, lo = tr.bounds(prob, 1, 1.0)
    # the periodic path: one period tiled exactly, rolled so that the first of its equal minima is point BP (its stencil straddles the
    # block edge BP-1 | BP); the same candidate stands again at 2 BP
    tiled = np.tile(paths["base"], 3)[: 2 * BP + 40]
    first = int(tr.path_with_torques(oracle_lib, model, tiled[None, :], H, hi, lo)[1]["at"])
    assert 1 <= first <= BP
    periodic = np.tile(np.roll(paths["base"], BP - first), 3)[: 2 * BP + 40]
    names = ["upper", "lower", "linear", "none", "short"]
    rows = [np.ascontiguousarray(paths[n][None, :]) for n in names] + [np.ascontiguousarray(periodic[None, :])]
    sres = [H] * len(rows)
    want, ref = tr.torque_scale(oracle_lib, model, rows, sres, prob)
    # what each path is there for, from the reference
    P = [tr.pieces(oracle_lib, model, r, H) for r in rows]
    assert all(not G.any() for A, B, G in P) and not ref["n_static"].any()
    assert int(ref[0]["side"]) == 1 and int(ref[1]["side"]) == -1 and float(ref[0]["s"]) < 1.0 and float(ref[1]["s"]) < 1.0
    assert not P[2][0].any() and P[2][1].all() and (int(ref[2]["side"]), int(ref[2]["at"]), int(ref[2]["row"])) == (1, 0, 0)
    x_line = (2.0 * float(hi[0])) / (float(P[2][1][0, 0]) + np.sqrt(float(P[2][1][0, 0]) ** 2))
    assert float(ref[2]["s"]) == x_line
    for k in (3, 4):
        assert np.isposinf(ref[k]["s"]) and (int(ref[k]["at"]), int(ref[k]["row"]), int(ref[k]["side"])) == (-1, -1, 0)
    a = int(ref[5]["at"])
    assert a == BP and all(P[5][j][0, a] == P[5][j][0, a + BP] for j in (0, 1)), "two equal minima: the lowest point is reported"
    out = capi.output_from_rows(hip_ctx, rows, sres, 1, 0, 0)
    new, rec = out.torque_scale(prob, model)
    check_rows(new, want, "steered")
    tr.assert_records_equal(rec, ref, "steered")
    new.close(); out.close()


# ---- 3. the same bits however it is cut ------------------------------------------------------------------------------------
def test_same_bits_under_a_workspace_budget(hip_lib, oracle_lib):
    model, rows, sres, want, P = known_pieces(oracle_lib, "kuka", 3, "smooth")
    nl = model.n_links
    tmax, tmin = range_of(P, nl, 1.0)
    prob = capi.make_problem(nl, 3, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0] * nl, jnt_trq_max=tmax, jnt_trq_min=tmin)
    ctx = capi.Context(hip_lib, 0)          # a context of its own: the budget is a property of the context
    out = capi.output_from_rows(ctx, rows, sres, nl, 3, 0)
    whole, rec = out.torque_scale(prob, model)
    assert whole.tscale_ranges() == 1
    flat = [r.copy() for r in whole.all_rows()]
    # room for the tables of about one block-sized path: the small paths share a range, each of the four long ones has its own
    ctx.set_workspace_budget(0, 8 * 3 * nl * (BP + 2))
    cut, rec_cut = out.torque_scale(prob, model)
    assert 3 <= cut.tscale_ranges() < len(rows), cut.tscale_ranges()
    ctx.set_workspace_budget(0, 1)          # every path a range of its own; a range of empty paths launches nothing
    each, rec_each = out.torque_scale(prob, model)
    assert each.tscale_ranges() == sum(1 for n in LENGTHS if n > 0)
    for o, r, what in ((cut, rec_cut, "under a budget"), (each, rec_each, "a range per path")):
        for k, (g, w) in enumerate(zip(o.all_rows(), flat)):
            assert g.tobytes() == w.tobytes(), (what, k)
        check_rows(o, want, what)
        assert r.tobytes() == rec.tobytes(), what
    # the rounds under the budget: the same report, rows and records
    ctx.set_workspace_budget(0, 0)
    a, rep_a, rec_a = out.stretch_torques(prob, model, 1.0, 4, 8.0)
    ctx.set_workspace_budget(0, 1)
    b, rep_b, rec_b = out.stretch_torques(prob, model, 1.0, 4, 8.0)
    assert rep_a.tobytes() == rep_b.tobytes() and rec_a.tobytes() == rec_b.tobytes() and int(rep_a["rounds"].max()) >= 1
    for k, (g, w) in enumerate(zip(b.all_rows(), a.all_rows())):
        assert g.tobytes() == w.tobytes(), k
    ctx.set_workspace_budget(0, 0)
    for o in (whole, cut, each, a, b, out):
        o.close()


# ---- 4. the rounds on a synthetic ragged batch -----------------------------------------------------------------------------
_SYNTH = {}


def synth_case(oracle_lib, name):
    if name not in _SYNTH:
        model = model_named(oracle_lib, name)
        rows = tr.synth_rows(model)
        sres = tr.synth_steps(len(rows))
        for a in rows:
            a.setflags(write=False)
        _SYNTH[name] = (model, rows, sres, tr.synth_problem(oracle_lib, model, rows, sres), {})
    return _SYNTH[name]


ARGS = [(1.0, 8, 16.0), (0.8, 8, 1.75), (1.0, 1, 16.0)]


@pytest.mark.parametrize("args", ARGS, ids=["plain", "cap", "one_round"])
@pytest.mark.parametrize("name", ["kuka", "rr", "random8", "one"])
def test_rounds_synthetic_batch(hip_ctx, oracle_lib, name, args):
    target, max_rounds, max_factor = args
    model, rows, sres, prob, caches = synth_case(oracle_lib, name)
    nl = model.n_links
    want, report, final, recs = tr.stretch_torques(oracle_lib, model, rows, sres, 0, prob, target, max_rounds, max_factor, caches.setdefault(target, {}))
    st = [int(v) for v in report["status"]]
    # what each parameter set is there for
    if args == ARGS[0]:
        assert set(st) == {capi.STRETCH_PASSES} and 2 <= int(report["rounds"].max()) <= 3
    if args == ARGS[1]:
        assert capi.STRETCH_CAPPED in st and capi.STRETCH_PASSES in st
    if args == ARGS[2]:
        assert capi.STRETCH_ROUNDS in st
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    new, got, rec = out.stretch_torques(prob, model, target, max_rounds, max_factor)
    sr.assert_report_equal(got, report, f"report {name} {args}")
    assert [int(n) for n in new.n_pts] == [int(n) for n in report["n_out"]] and (new.n_theta, new.n_cart, new.n_trq) == (nl, 0, nl)
    check_rows(new, want, f"rounds {name} {args}")
    assert_audit_equal(new.audit(tr.with_trq_on(prob), 0.0), final, f"final audit {name} {args}")
    tr.assert_records_equal(rec, recs, f"records {name} {args}")
    assert new.tscale_ranges() == int(report["rounds"].max()) + 1 and new.tscale_ms() >= 0.0
    for k, (g, r) in enumerate(zip(out.all_rows(), rows)):
        assert g.tobytes() == r.tobytes(), k
    new.close(); out.close()


def test_device_libm_report(hip_ctx, oracle_lib):
    """a record: how the report of the rounds differs when the trig comes from the device libm"""
    model, rows, sres, prob, caches = synth_case(oracle_lib, "kuka")
    out = capi.output_from_rows(hip_ctx, rows, sres, model.n_links, 0, 0)
    a, rep_a, rec_a = out.stretch_torques(prob, model, 1.0, 8, 16.0, host_trig=True)
    b, rep_b, rec_b = out.stretch_torques(prob, model, 1.0, 8, 16.0, host_trig=False)
    ds = [abs(float(x) - float(y)) / float(x) for x, y in zip(rec_a["s"], rec_b["s"]) if np.isfinite(x)]
    print(f"TSCALE device libm against host trig tables, kuka batch: n_out differ on {int((rep_a['n_out'] != rep_b['n_out']).sum())} of {len(rows)} paths "
          f"(largest difference {int(np.abs(rep_a['n_out'] - rep_b['n_out']).max())} points), rounds differ on {int((rep_a['rounds'] != rep_b['rounds']).sum())}, "
          f"status on {int((rep_a['status'] != rep_b['status']).sum())}; largest relative difference of s {max(ds):.3e}")
    assert [int(v) for v in rep_b["status"]] == [capi.STRETCH_PASSES] * len(rows)
    for o in (a, b, out):
        o.close()


# ---- 5. gravity alone leaves the range -------------------------------------------------------------------------------------
def test_static(hip_ctx, oracle_lib):
    model = one_link_model()                     # G = m g com cos(q): 4.905 Nm with the link horizontal
    n = 200
    t = np.arange(n) * H
    swing = 1.2 * np.sin(4.0 * t)                # passes the horizontal, and moves faster than its limits allow
    hang = np.pi / 2 + 0.1 * np.sin(2.0 * t)     # stays near the vertical
    rows = [np.ascontiguousarray(swing[None, :]), np.ascontiguousarray(hang[None, :])]
    sres = [H, H]
    P = [tr.pieces(oracle_lib, model, r, H) for r in rows]
    gpeak = float(np.abs(P[0][2]).max())
    assert gpeak > 4.9 and float(np.abs(P[1][2]).max()) < 0.6
    prob = capi.make_problem(1, 0, capi.ROBOT_GENJNT, capi.F_JNT_ACC_ON, jnt_vel_max=[3.0], jnt_acc_max=[12.0], jnt_trq_max=[0.8 * gpeak],
                             jnt_trq_min=[-0.8 * gpeak])
    want, report, final, recs = tr.stretch_torques(oracle_lib, model, rows, sres, 0, prob, 1.0, 8, 16.0)
    kin = sr.stretch_audit(rows, sres, 1, 0, prob, 1.0, 8, 16.0)[1]
    assert [int(v) for v in report["status"]] == [capi.STRETCH_STATIC, capi.STRETCH_PASSES]
    assert int(recs[0]["n_static"]) > 0 and int(recs[1]["n_static"]) == 0
    # stretched as far as its kinematic families ask, and no further
    assert int(report[0]["n_out"]) == int(kin[0]["n_out"]) > n and int(report[0]["rounds"]) == int(kin[0]["rounds"]) >= 1
    assert float(final[0]["fam"][capi.AUDIT_TRQ]["peak"]) > 1.0
    out = capi.output_from_rows(hip_ctx, rows, sres, 1, 0, 0)
    new, got, rec = out.stretch_torques(prob, model, 1.0, 8, 16.0)
    sr.assert_report_equal(got, report, "static")
    check_rows(new, want, "static")
    tr.assert_records_equal(rec, recs, "static")
    assert_audit_equal(new.audit(tr.with_trq_on(prob), 0.0), final, "static")
    new.close(); out.close()


# ---- 6. a range that never binds -------------------------------------------------------------------------------------------
def test_a_range_that_never_binds_is_the_stretch_audit(hip_ctx, oracle_lib):
    model, rows, sres, prob, caches = synth_case(oracle_lib, "kuka")
    nl = model.n_links
    wide = capi.Problem.from_buffer_copy(bytes(prob))
    for j in range(nl):
        wide.jnt_trq_max[j], wide.jnt_trq_min[j] = 1e9, -1e9
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    plain, rep_plain = out.stretch_audit(wide, 1.0, 8, 16.0)
    new, rep, rec = out.stretch_torques(wide, model, 1.0, 8, 16.0)
    assert rep.tobytes() == rep_plain.tobytes() and int(rep["rounds"].max()) >= 1
    for k, (g, w) in enumerate(zip(new.all_rows(), plain.all_rows())):
        assert g[:nl].tobytes() == w.tobytes(), k
    assert not rec["n_static"].any()
    for o in (new, plain, out):
        o.close()


# ---- 7. composition, device against device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("host_trig", [True, False], ids=["host_trig", "device_libm"])
def test_the_result_is_the_torque_rows_of_the_stretched_output(hip_ctx, oracle_lib, host_trig):
    model, rows, sres, prob, caches = synth_case(oracle_lib, "random8")
    nl = model.n_links
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    for target, max_rounds, max_factor in ARGS:
        new, rep, rec = out.stretch_torques(prob, model, target, max_rounds, max_factor, host_trig=host_trig)
        long = out.stretch_to(rep["n_out"])
        composed = long.torques(model, host_trig=host_trig)
        for k, (g, w) in enumerate(zip(new.all_rows(), composed.all_rows())):
            ir.assert_rows_bit_equal(g, w, f"path {k}, {(target, max_rounds, max_factor)}")
        aud = new.audit(tr.with_trq_on(prob), 0.0)
        for k in range(len(rows)):
            if int(rep[k]["status"]) == capi.STRETCH_PASSES:
                assert all(float(aud[k]["fam"][f]["peak"]) <= target for f in range(5)), (k, aud[k])
                if target == 1.0:
                    assert int(aud[k]["n_over"]) == 0
        # the records are those of the result's own rows: the known-answer entry on the stretched output gives them again
        again, rec2 = long.torque_scale(prob, model, target, host_trig=host_trig)
        assert rec2.tobytes() == rec.tobytes()
        for o in (new, long, composed, again):
            o.close()
    out.close()


# ---- 8. real trajectories --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["KUKA-LWR-IV", "synth_gen7dof_s0"])
def test_real_trajectories(hip_ctx, oracle_lib, name):
    case = helpers.Case(name)
    out, b = helpers.run_to_output(hip_ctx, [case])
    model = hip_ctx.library.builtin_serial_model(capi.ROBOT_KUKA)
    nl = model.n_links
    rows = [r.copy() for r in out.all_rows()]
    A, B, G = tr.pieces(oracle_lib, model, rows[0][:nl], out.sres[0])
    limit = 1.05 * np.abs(G).max(axis=1) + 0.5 * np.abs(A + B).max(axis=1) + 1e-3
    prob = capi.Problem.from_buffer_copy(bytes(case.problem))
    for j in range(nl):
        prob.jnt_trq_max[j], prob.jnt_trq_min[j] = float(limit[j]), -float(limit[j])
    new, got, rec = out.stretch_torques(prob, model, 1.0, 8, 16.0)
    want, report, final, recs = tr.stretch_torques(oracle_lib, model, rows, out.sres, out.n_cart, prob, 1.0, 8, 16.0)
    r = got[0]
    print(f"TSCALE {name}: {int(r['n_in'])} -> {int(r['n_out'])} points, factor {float(r['factor']):.4f}, rounds {int(r['rounds'])}, status {int(r['status'])}; "
          f"TRQ peak after {float(final[0]['fam'][capi.AUDIT_TRQ]['peak']):.6f}, s of the result {float(rec[0]['s']):.6f}; kernels {new.tscale_ms():.3f} ms in "
          f"{new.tscale_ranges()} launches")
    sr.assert_report_equal(got, report, name)
    check_rows(new, want, name)
    tr.assert_records_equal(rec, recs, name)
    assert int(r["status"]) == capi.STRETCH_PASSES
    after = new.audit(tr.with_trq_on(prob), 0.0)
    assert_audit_equal(after, final, name)
    assert int(after[0]["n_over"]) == 0 and int(after[0]["n_nonfinite"]) == 0
    # the source is untouched
    for g, w in zip(out.all_rows(), rows):
        assert g.tobytes() == w.tobytes()
    new.close(); out.close(); b.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(hip_ctx, hip_lib, oracle_lib):
    model, rows, sres, prob, caches = synth_case(oracle_lib, "kuka")
    nl = model.n_links
    lib = hip_lib.lib
    out = capi.output_from_rows(hip_ctx, rows, sres, nl, 0, 0)
    with_trq = capi.output_from_rows(hip_ctx, [np.zeros((nl + 2, 5))], [H], nl, 0, 2)
    six = capi.output_from_rows(hip_ctx, [np.zeros((6, 5))], [H], 6, 0, 0)
    rep = np.zeros(len(rows), dtype=capi.STRETCH_DTYPE)
    rec = np.zeros(len(rows), dtype=capi.TSCALE_DTYPE)
    rp, cp = rep.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)

    def ref(x):
        return C.byref(x) if x is not None else None

    def refused(what, word, o=out, p=prob, m=model, flags=capi.F_HOST_TRIG, target=1.0, rounds=8, factor=16.0, report=rp, scale=cp):
        for entry in ("scale", "rounds"):
            h = C.c_void_p(0xdead)
            if entry == "scale":
                rc = lib.batotp_hip_output_torque_scale(o.handle if o is not None else None, ref(p), ref(m), flags, target, C.byref(h), scale)
            else:
                rc = lib.batotp_hip_output_stretch_torques(o.handle if o is not None else None, ref(p), ref(m), flags, target, rounds, factor, C.byref(h),
                                                           report, scale)
            msg = lib.batotp_hip_last_error()
            assert rc == ERR_ARG and h.value is None and msg and word in msg, (what, entry, rc, h.value, msg)

    def model_copy():
        return capi.SerialModel.from_buffer_copy(bytes(model))

    def prob_copy():
        return capi.Problem.from_buffer_copy(bytes(prob))

    refused("NULL output", b"NULL argument", o=None)
    refused("NULL problem", b"NULL argument", p=None)
    refused("NULL model", b"NULL argument", m=None)
    assert lib.batotp_hip_output_torque_scale(out.handle, C.byref(prob), C.byref(model), capi.F_HOST_TRIG, 1.0, None, cp) == ERR_ARG
    assert lib.batotp_hip_output_stretch_torques(out.handle, C.byref(prob), C.byref(model), capi.F_HOST_TRIG, 1.0, 8, 16.0, None, rp, cp) == ERR_ARG
    h = C.c_void_p(0xdead)
    assert lib.batotp_hip_output_torque_scale(out.handle, C.byref(prob), C.byref(model), capi.F_HOST_TRIG, 1.0, C.byref(h), None) == ERR_ARG and h.value is None
    assert lib.batotp_hip_output_stretch_torques(out.handle, C.byref(prob), C.byref(model), capi.F_HOST_TRIG, 1.0, 8, 16.0, C.byref(h), None, cp) == ERR_ARG
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
    # what the audit refuses
    seven = capi.make_problem(6, 0, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0] * 6, jnt_trq_max=[1.0] * 6, jnt_trq_min=[-1.0] * 6)
    refused("joint count", b"audit", p=seven)
    p = prob_copy(); p.jnt_acc_max[2] = 0.0
    refused("a limit of 0", b"audit", p=p)
    p = prob_copy(); p.flags |= capi.F_PARALLEL
    refused("a parallel mechanism", b"parallel", p=p)
    # the torque range
    for j, (hi, lo) in ((0, (1.0, 1.0)), (nl - 1, (-1.0, 1.0)), (2, (np.nan, -1.0)), (3, (np.inf, -1.0)), (1, (1.0, -np.inf))):
        p = prob_copy(); p.jnt_trq_max[j], p.jnt_trq_min[j] = hi, lo
        refused(f"torque range {hi} {lo}", b"torque range of joint %d" % j, p=p)
    # target, and what the stretch's audit mode refuses
    for target in (0.0, -1.0, 1.0 + 1e-12, np.nan, np.inf):
        refused(f"target {target}", b"target", target=target)
    for rounds, factor, what in ((0, 16.0, "no rounds"), (17, 16.0, "17 rounds"), (8, 0.99, "max_factor < 1"), (8, np.inf, "max_factor Inf"), (8, np.nan, "NaN")):
        h = C.c_void_p(0xdead)
        rc = lib.batotp_hip_output_stretch_torques(out.handle, C.byref(prob), C.byref(model), capi.F_HOST_TRIG, 1.0, rounds, factor, C.byref(h), rp, cp)
        assert rc == ERR_ARG and h.value is None and b"output_stretch_torques" in lib.batotp_hip_last_error(), what
    assert not rep.view(np.uint8).any() and not rec.view(np.uint8).any(), "a refused call writes no report and no record"
    # entries of joints the model does not use are not read; the scale records are optional for the rounds
    one = one_link_model()
    p1 = capi.make_problem(1, 0, capi.ROBOT_GENJNT, 0, jnt_vel_max=[1.0], jnt_trq_max=[10.0, np.nan], jnt_trq_min=[-10.0, np.nan])
    o1 = capi.output_from_rows(hip_ctx, [np.zeros((1, 3))], [H], 1, 0, 0)
    n1, r1 = o1.torque_scale(p1, one)
    assert np.isfinite(n1.rows(0)).all() and np.isposinf(r1[0]["s"]) and int(r1[0]["n_static"]) == 0
    rep1 = np.zeros(1, dtype=capi.STRETCH_DTYPE)
    h = C.c_void_p()
    assert lib.batotp_hip_output_stretch_torques(o1.handle, C.byref(p1), C.byref(one), capi.F_HOST_TRIG, 1.0, 8, 16.0, C.byref(h), rep1.ctypes.data_as(C.c_void_p), None) == 0
    assert h.value and int(rep1[0]["n_out"]) == 3 and int(rep1[0]["status"]) == capi.STRETCH_PASSES
    lib.batotp_hip_output_destroy(h)
    n1.close(); o1.close()
    # the context still serves a valid call; no paths; paths without points
    new, got, r = out.stretch_torques(prob, model, 1.0, 1, 16.0)
    assert capi.STRETCH_ROUNDS in [int(v) for v in got["status"]]
    new.close()
    empty = capi.output_from_rows(hip_ctx, [], [], nl, 0, 0)
    e, r0 = empty.torque_scale(prob, model)
    assert e.n_paths == 0 and (e.n_theta, e.n_cart, e.n_trq) == (nl, 0, nl) and e.all_rows() == [] and r0.shape == (0,) and e.tscale_ranges() == 0 and e.tscale_ms() == 0.0
    e2, rep0, r0 = empty.stretch_torques(prob, model)
    assert e2.n_paths == 0 and rep0.shape == (0,) and e2.tscale_ranges() == 0
    hollow = capi.output_from_rows(hip_ctx, [np.zeros((nl, 0))] * 3, [H] * 3, nl, 0, 0)
    h_, rep3, r3 = hollow.stretch_torques(prob, model, host_trig=False)
    assert [int(n) for n in h_.n_pts] == [0, 0, 0] and (h_.n_theta, h_.n_cart, h_.n_trq) == (nl, 0, nl) and h_.tscale_ranges() == 0
    assert not rep3["status"].any() and [float(v) for v in rep3["factor"]] == [1.0] * 3 and all(np.isposinf(r3["s"])) and [int(v) for v in r3["at"]] == [-1] * 3
    assert all(r.shape == (2 * nl, 0) for r in h_.all_rows())
    for o in (e, e2, empty, h_, hollow, out, with_trq, six):
        o.close()


# ---- 10. the host route ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    csrc = os.path.join(helpers.ROOT, "batotp_amd", "csrc")
    exe = tmp_path_factory.mktemp("tscale_driver") / "tscale_batch"
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", f"-I{HOST}", f"-I{helpers.ROOT}/include", os.path.join(helpers.ROOT, "tests", "drivers", "tscale_batch_main.cpp"),
           os.path.join(HOST, "_build", "libbatotp.a"), f"-L{csrc}", "-lbatotp_hip", f"-Wl,-rpath,{csrc}", "-pthread", "-lm", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_host_route(hip_ctx, driver, tmp_path):
    """BA::setStretchToTorqueLimits on the reference's KUKA example, planned under joint velocity and acceleration limits only"""
    from test_gpu_invdyn import TRQ_LIMITS, read_dump
    stage_kuka(tmp_path)
    exe = os.path.join(HOST, "_build", "batest_batch")
    assert os.path.exists(exe), "build() must produce batest_batch"
    n = 3
    # as the issue words it: the default target
    r = subprocess.run([exe, "config.dat", str(n), "--stretch-torques", "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("stretch-torques (target 1):")]
    assert len(lines) == 1, r.stdout[-2000:]
    peaks = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("torques: path ")]
    assert len(peaks) == n and all(0.0 <= float(p[4]) <= 1.0 for p in peaks), r.stdout[-2000:]
    print("TSCALE host route:", lines[0])
    w = lines[0].split()
    # stretch-torques (target 1): 3 of 3 paths stretched, largest factor 3.18.. (path 0), 0 not passing, 0 of them static
    assert (w[3], w[5], w[w.index("not") - 1], w[-4]) == (str(n), str(n), "0", "0") and float(w[w.index("factor") + 1]) > 1.0, lines[0]
    after = [ln for ln in r.stdout.splitlines() if ln.startswith("audit (tol 0):")]
    assert len(after) == 1 and after[0].endswith("; over: none"), r.stdout[-2000:]
    target = 1.0
    # without the option nothing changes
    r0 = subprocess.run([exe, "config.dat", str(n), "--audit"], cwd=tmp_path, capture_output=True, text=True)
    assert r0.returncode == 0 and "stretch-torques" not in r0.stdout and " trq -" in r0.stdout
    # Traj::trq, nPts and tTotalTraj against the C-ABI route on the dumped rows
    r = subprocess.run([driver, "config.dat", str(n), str(target)], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    dump = read_dump(tmp_path / "dump.bin")
    rep = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("tscale ")]
    assert len(dump) == n and len(rep) == n
    model = hip_ctx.library.builtin_serial_model(capi.ROBOT_KUKA)
    nT, nC, nQ = dump[0][:3]
    assert (nT, nC, nQ) == (7, 3, 7)
    rows = [np.ascontiguousarray(p[4][:nT + nC]) for p in dump]
    again = capi.output_from_rows(hip_ctx, rows, [p[3] for p in dump], nT, nC, 0)
    new = again.torques(model, host_trig=True)
    for k, g in enumerate(new.all_rows()):
        ir.assert_rows_bit_equal(dump[k][4], g, f"Traj rows of path {k} against the C-ABI route")
    prob = capi.make_problem(7, 3, capi.ROBOT_KUKA, capi.F_TRQ_ON, jnt_vel_max=[1.0] * 7, jnt_trq_max=[float(v) for v in TRQ_LIMITS.split()],
                             jnt_trq_min=[-float(v) for v in TRQ_LIMITS.split()])
    aud = new.audit(prob, 0.0)
    for k, w in enumerate(rep):
        f = dict(zip(w[2::2], w[3::2]))
        assert int(w[1]) == k and int(f["done"]) == 1 and int(f["status"]) == capi.STRETCH_PASSES and int(f["n_out"]) == rows[k].shape[1] >= int(f["n_in"])
        peak = np.array([int(f["trq_peak"], 16)], dtype=np.uint64).view(np.float64)[0]
        assert peak.tobytes() == aud[k]["fam"][capi.AUDIT_TRQ]["peak"].tobytes() and 0.0 <= peak <= target
    assert all(int(dict(zip(w[2::2], w[3::2]))["n_out"]) > int(dict(zip(w[2::2], w[3::2]))["n_in"]) for w in rep), "every path was stretched"
    new.close(); again.close()
