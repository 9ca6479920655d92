"""GPU (-m gpu): torque-limited planning with chain models of 1 to 8 links -- k_dyn_serial, the splines of the 4 nJ dynamics
channels, the torque branch of the pointwise evaluation and the FEAT == 2 sweep kernels -- against the oracle, bit for bit.

The oracle's a1..a4 are pinned by tests/test_dyn_chain_cpu.py (Lagrange's equations in 50-digit arithmetic); here the device has to
reproduce them, and everything planned from them, exactly (host trig tables, tolerance 0).  Models: random tilted-axis
chains of every link count in degrees and radians, and the special cases of tests/dyn_reference.py.  One ragged batch per model with
path boundaries on both sides of k_dyn_serial's 128-lane blocks; C = 5 nJ + nC runs from 5 to 43 channels, so the LDS row window of
the one-path-per-wavefront kernel holds between 76 and 8 rows.  Torque limits come from the oracle's own a1 / a4 peaks, and every
batch is checked (on the oracle) to finish and to be bounded by them."""
import zlib

import numpy as np
import pytest

import dyn_reference as dr
import helpers
from helpers import assert_bit_equal
from batotp_amd import capi

pytestmark = pytest.mark.gpu

LENGTHS = [4, 5, 127, 128, 129, 257, 300]
SPAN = 1.0          # every path runs over s in [0, SPAN]: q' of short and long paths has one scale
CAP = 8192
BASE_FLAGS = capi.F_TRQ_ON | capi.F_HOST_TRIG | capi.F_JNT_ACC_ON
PAIRS = capi.F_NO_SAMPLES | capi.F_COMPACT_SPLINES
WIDE = 1e9
# device libm (BATOTP_F_HOST_TRIG cleared) against host trig tables, a1..a4 relative to the largest |value| of the coefficient family
# on the path.  Measured on the MI355X over the three batches of test_device_libm_is_close, which prints it: 8.1e-16 (a1 5.1e-16,
# a2 8.1e-16, a3 0, a4 6.3e-16).  The bound is 100 x the measured maximum, rounded up to a power of ten.
DEVICE_LIBM_BOUND = 1e-13

# name -> (model, Cartesian channels, further problem flags).  `lib` supplies the built-in tables.
MODELS = {
    "1deg": (lambda lib: dr.random_chain(1, True), 0, 0),
    "2rad+3": (lambda lib: dr.random_chain(2, False), 3, 0),
    "3deg": (lambda lib: dr.random_chain(3, True), 0, 0),
    "4rad+3": (lambda lib: dr.random_chain(4, False), 3, 0),
    "5deg+3": (lambda lib: dr.random_chain(5, True), 3, 0),
    "6rad": (lambda lib: dr.random_chain(6, False), 0, 0),
    "7rad": (lambda lib: dr.random_chain(7, False), 0, 0),
    "8deg+3": (lambda lib: dr.random_chain(8, True), 3, 0),
    "8rad": (lambda lib: dr.random_chain(8, False), 0, 0),
    "frictionless4deg": (lambda lib: dr.frictionless(dr.random_chain(4, True, seed=71)), 0, 0),
    "weightless3rad+3": (lambda lib: dr.weightless(dr.random_chain(3, False, seed=72)), 3, 0),
    "massless5rad": (lambda lib: dr.massless_last_link(dr.random_chain(5, False, seed=73)), 0, 0),
    "aligned6deg": (lambda lib: dr.axis_aligned(6, True), 0, 0),
    "rr": (lambda lib: lib.builtin_serial_model(capi.ROBOT_RR), 0, 0),
    "cartvel3deg+3": (lambda lib: dr.random_chain(3, True, seed=74), 3, capi.F_CART_VEL_ON),
}
ROW_LAYOUTS = [0, 1, 2, 4, 8, 16, 64, "64noff", "64x2"]
PAIR_LAYOUTS = [0, 64, "64noff", "64x2"]
MANDATORY = {("rows", 0), ("rows", 1), ("rows", 8), ("rows", 64), ("pairs", 0), ("pairs", 64)}


class Path:
    def __init__(self, name, y, sres, problem):
        self.name, self.y, self.sres, self.problem = name, np.ascontiguousarray(y), float(sres), problem
        self.y.setflags(write=False)

    @property
    def n(self):
        return self.y.shape[1]

    def max_steps(self):
        return CAP


def _knots(name, model, n_cart, lengths, amplitude=1.0):
    """[(y, sres)] of the ragged batch `name`"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    nJ = model.n_links
    out = []
    for n in lengths:
        if name == "rr":
            # the lemniscate of the reference's two-link example, thinned to n knots
            rr = helpers.Case("RR")
            idx = np.round(np.linspace(0, rr.n - 1, n)).astype(int)
            out.append((rr.y[:2, idx], rr.sres * (rr.n - 1) / (n - 1)))
            continue
        if nJ == 1:
            # one joint: a full turn in one direction.  (Where its only q' changes sign, a1 = M q' passes through 0 with nothing else
            # to bound the path: the oracle -- like the reference's bisection -- fails there on every oscillating path tried.)
            s = np.linspace(0.0, 1.0, n)
            y = rng.choice([-1.0, 1.0]) * (rng.uniform(6, 9) * s + 0.5 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * s + rng.uniform(0, 6)) - rng.uniform(0, 9))
            y = np.ascontiguousarray(amplitude * dr.knot_scale(model) * y[None, :])
        else:
            y = helpers.random_knots(rng, nJ, n, amplitude * dr.knot_scale(model))
        if n_cart:
            y = np.vstack([y, helpers.random_knots(rng, n_cart, n, 0.3)])
        out.append((y, SPAN / (n - 1)))
    return out


VMAX = 1.75         # joint speed limit [rad / s] (the same in degrees for a model in degrees); acceleration limit: 5 x that per second


def _problem(model, n_cart, extra, trq_max, **kw):
    nJ = model.n_links
    vmax = VMAX * (180.0 / np.pi if model.degrees else 1.0)
    return capi.make_problem(nJ, n_cart, flags=BASE_FLAGS | extra, jnt_vel_max=[vmax] * nJ, jnt_acc_max=[5 * vmax] * nJ,
                             jnt_trq_max=list(trq_max), jnt_trq_min=[-v for v in trq_max], cart_vel_max=0.5, **kw)


def _limits_from(dyn_list):
    """symmetric torque limits a little above the gravity peak of every row: 1.1 max|a4| + 0.01 max|a1| x the acceleration limit
    + 0.02 over the given paths (the acceleration limit in rad / s^2 whatever the model's unit, so that the recipe means the same
    for both; a1 is per unit of s, all paths of a batch span the same s)"""
    a1 = np.max([np.abs(d[0]).max(axis=1) for d in dyn_list], axis=0)
    a4 = np.max([np.abs(d[3]).max(axis=1) for d in dyn_list], axis=0)
    return [float(v) for v in 1.1 * a4 + 0.01 * a1 * (5 * VMAX) + 0.02]


def plan(ctx, paths, model, flags=0, samples_from=None, mvc=True, details=False):
    """helpers.run_pipeline of one batch on `ctx`, plus the shape of both sweep launches where the library reports it"""
    prob = capi.Problem.from_buffer_copy(bytes(paths[0].problem))
    prob.flags |= flags
    b = capi.Batch(ctx, prob, [p.n for p in paths], CAP)
    for k, p in enumerate(paths):
        b.upload_knots(k, [p.y], [p.sres])
    helpers.precompute_with_trig(ctx, b, prob, len(paths), model, samples_from)
    if mvc:
        b.pointwise_mvc()
    b.sweep(-1); b.sweep(+1)
    res = b.results()
    out = []
    for k in range(len(paths)):
        d = {"result": res[k], "rev": b.curve(k, -1), "fwd": b.curve(k, +1)}
        if mvc:
            d["mvc"] = np.stack(b.mvc(k))
        if details:
            d.update(precomputed(b, prob, k))
        out.append(d)
    try:
        launch = (b.last_sweep_launch(-1), b.last_sweep_launch(+1))
    except (capi.BatotpError, AttributeError):
        launch = None       # (the oracle launches nothing)
    b.close()
    return out, launch


def precomputed(b, prob, k):
    """what the precompute stages publish for path k: coefficient rows of all C channels; samples and a1..a4 where the batch keeps them"""
    d = {"coef": np.stack([b.coeffs(k, ch) for ch in range(prob.n_channels)])}
    if not (prob.flags & capi.F_NO_SAMPLES):
        d["samp"] = np.stack([b.samples(k, ch) for ch in range(prob.n_joints + prob.n_cart)])
    if not (prob.flags & capi.F_COMPACT_SPLINES):
        d["dyn"] = np.stack([np.stack([b.dyn(k, kk, r) for r in range(prob.dyn_dim)]) for kk in (1, 2, 3, 4)])
    return d


_BATCHES = {}


def batch(oracle_ctx, name):
    """(model, paths under the derived torque limits, the oracle's plan of them with every published array) of the batch `name` --
    built once, shared, never modified.  The conditions every batch has to meet are asserted here, on the oracle."""
    if name in _BATCHES:
        return _BATCHES[name]
    make, n_cart, extra = MODELS[name]
    model = make(oracle_ctx.library)
    knots = _knots(name, model, n_cart, LENGTHS)
    wide_prob = _problem(model, n_cart, extra, [WIDE] * model.n_links)
    wide, _ = plan(oracle_ctx, [Path(f"{name}[{k}]", y, s, wide_prob) for k, (y, s) in enumerate(knots)], model, mvc=False, details=True)
    prob = _problem(model, n_cart, extra, _limits_from([w["dyn"] for w in wide]))
    paths = [Path(f"{name}[{k}]", y, s, prob) for k, (y, s) in enumerate(knots)]
    want, _ = plan(oracle_ctx, paths, model, details=True)
    bound = 0
    for k, (w, o) in enumerate(zip(wide, want)):
        r = o["result"]
        assert r["status_rev"] == 0 and r["status_fwd"] == 0 and r["n_bisect_fail_rev"] == 0 and r["n_bisect_fail_fwd"] == 0, (name, k, r)
        assert r["n_fwd"] >= 4 and np.all(np.isfinite(o["dyn"]))
        bound += int(o["fwd"][1].shape != w["fwd"][1].shape or not np.array_equal(o["fwd"][1], w["fwd"][1]))
    assert 2 * bound >= len(paths), f"{name}: the torque limits change the forward curve of {bound} of {len(paths)} paths only"
    for o in want:
        for v in o.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    _BATCHES[name] = (model, paths, want)
    return _BATCHES[name]


def compare_plans(paths, got, want, what):
    """pointwise bounds, both curves and the whole result row of every path (the fields tests/test_gpu_parity.py compares)"""
    for p, g, w in zip(paths, got, want):
        if "mvc" in g:
            assert_bit_equal(g["mvc"], w["mvc"], f"{p.name}: pointwise bounds, {what}")
        for which in ("rev", "fwd"):
            assert_bit_equal(g[which][0], w[which][0], f"{p.name}: {which}.s, {what}")
            assert_bit_equal(g[which][1], w[which][1], f"{p.name}: {which}.sdot, {what}")
        for f in g["result"].dtype.names:
            assert g["result"][f] == w["result"][f], (p.name, f, what, g["result"], w["result"])


def compare_precomputed(p, prob, g, w, what):
    """coefficient rows of all C channels; samples and a1..a4 at every knot -- with pairs for all channels a_k of row r is c0 of
    channel Cin + (k - 1) d + r (its last entry belongs to no segment)"""
    assert_bit_equal(g["coef"], w["coef"], f"{p.name}: coefficient rows, {what}")
    if "samp" in g:
        assert_bit_equal(g["samp"], w["samp"], f"{p.name}: samples, {what}")
    if "dyn" in g:
        assert_bit_equal(g["dyn"], w["dyn"], f"{p.name}: a1..a4, {what}")
    else:
        cin, d = prob.n_joints + prob.n_cart, prob.dyn_dim
        for k in range(4):
            for r in range(d):
                assert_bit_equal(g["coef"][cin + k * d + r][0][:-1], w["dyn"][k][r][:-1], f"{p.name}: a{k + 1} of row {r}, {what}")


# ---- 1. precompute alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows", "pairs"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_coefficients_at_every_knot_and_their_splines(hip_ctx, oracle_ctx, name, form):
    model, paths, want = batch(oracle_ctx, name)
    prob = capi.Problem.from_buffer_copy(bytes(paths[0].problem))
    prob.flags |= PAIRS if form == "pairs" else 0
    assert prob.n_channels == 5 * model.n_links + prob.n_cart
    b = capi.Batch(hip_ctx, prob, [p.n for p in paths], CAP)
    for k, p in enumerate(paths):
        b.upload_knots(k, [p.y], [p.sres])
    helpers.precompute_with_trig(hip_ctx, b, prob, len(paths), model, want if form == "pairs" else None)
    for k, p in enumerate(paths):
        compare_precomputed(p, prob, precomputed(b, prob, k), want[k], form)
    b.close()


def test_special_models_are_what_they_claim(oracle_ctx):
    """(on the oracle) a3 == 0 without friction, a4 == 0 without gravity, a row of a1 under the threshold of reference ba.cpp:1500 without mass"""
    for name, fam, rows in (("frictionless4deg", 2, slice(None)), ("weightless3rad+3", 3, slice(None)), ("massless5rad", 0, slice(4, 5)),
                            ("massless5rad", 1, slice(4, 5)), ("massless5rad", 3, slice(4, 5))):
        _, paths, want = batch(oracle_ctx, name)
        for w in want:
            assert not np.any(w["dyn"][fam][rows]), (name, fam)
    _, paths, want = batch(oracle_ctx, "massless5rad")
    assert all(np.any(w["dyn"][2][4]) for w in want)       # (friction still acts on the massless link's joint)
    # the Cartesian speed limit of its batch binds: without it every forward curve is another
    model, paths, want = batch(oracle_ctx, "cartvel3deg+3")
    prob = capi.Problem.from_buffer_copy(bytes(paths[0].problem))
    prob.flags &= ~capi.F_CART_VEL_ON
    free, _ = plan(oracle_ctx, [Path(p.name, p.y, p.sres, prob) for p in paths], model, mvc=False)
    assert all(not np.array_equal(f["fwd"][1], w["fwd"][1]) for f, w in zip(free, want))
    model, _, want = batch(oracle_ctx, "aligned6deg")
    assert all(sorted(abs(v) for v in model.link[i].axis) == [0, 0, 1] and not any(list(model.link[i].inertia)[3:]) for i in range(6))


# ---- 2. pointwise bounds, both curves, the result rows: every sweep kernel shape ----------------------------------------------
def _layouts():
    return [("rows", l) for l in ROW_LAYOUTS] + [("pairs", l) for l in PAIR_LAYOUTS]


@pytest.mark.parametrize("form,layout", _layouts(), ids=[f"{f}-{l}" for f, l in _layouts()])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_torque_limited_plan(hip_lib, oracle_ctx, name, form, layout):
    model, paths, want = batch(oracle_ctx, name)
    ctx = capi.Context(hip_lib, 0)
    try:
        helpers.set_layout(ctx, layout)
        got, launch = plan(ctx, paths, model, flags=PAIRS if form == "pairs" else 0, samples_from=want if form == "pairs" else None)
    except capi.BatotpError as e:
        assert (form, layout) not in MANDATORY, f"{name}: {form} x {layout} may not be refused: {e}"
        pytest.skip(f"{name}: {form} x {layout} refused by the library: {e}")
    finally:
        ctx.close()
    assert launch is not None
    compare_plans(paths, got, want, f"{form} x {layout}, launches (lanes, paths per wavefront, hold) {launch[0]} / {launch[1]}")
    if layout in (1, 2, 4, 8, 16) and form == "rows":
        assert launch[0][0] == layout and launch[1][0] == layout
    if form == "pairs" or layout in (64, "64noff", "64x2"):
        assert launch[0][0] == 64 and launch[1][0] == 64


# ---- 3. an inadmissible path in the batch -------------------------------------------------------------------------------------
_STALLED = {}


def stalled_batch(oracle_ctx):
    """the 4-link chain with limits taken from paths of a fifth of the amplitude; path 2 (129 knots) swings six times as far, into
    configurations whose gravity torque alone exceeds them.  max_integ_time and the capacity are small: the path ends quickly."""
    if not _STALLED:
        name = "4rad+3"
        make, n_cart, extra = MODELS[name]
        model = make(oracle_ctx.library)
        lengths = [127, 5, 129, 128, 300]
        knots = _knots("stalled", model, n_cart, lengths, amplitude=0.2)
        big = _knots("stalled-big", model, n_cart, [129], amplitude=1.2)[0]
        wide_prob = _problem(model, n_cart, extra, [WIDE] * 4)
        wide, _ = plan(oracle_ctx, [Path(f"stalled[{k}]", y, s, wide_prob) for k, (y, s) in enumerate(knots + [big])], model, mvc=False, details=True)
        lim = _limits_from([w["dyn"] for w in wide[:-1]])
        over = np.abs(wide[-1]["dyn"][3]) > np.array(lim)[:, None]
        assert 0 < np.count_nonzero(over.any(axis=0)) < 129, "gravity has to exceed the limits on a part of the path"
        prob = _problem(model, n_cart, extra, lim, max_integ_time=12.0)
        knots[2] = big
        paths = [Path(f"stalled[{k}]", y, s, prob) for k, (y, s) in enumerate(knots)]
        want, _ = plan(oracle_ctx, paths, model, details=True)
        alone, _ = plan(oracle_ctx, [p for k, p in enumerate(paths) if k != 2], model)
        _STALLED.update(model=model, paths=paths, want=want, alone=alone)
    return _STALLED["model"], _STALLED["paths"], _STALLED["want"], _STALLED["alone"]


@pytest.mark.parametrize("form,layout", [("rows", 0), ("rows", 1), ("rows", 8), ("rows", 16), ("rows", 64), ("rows", "64noff"), ("pairs", 0), ("pairs", "64noff")])
def test_a_path_gravity_alone_stops(hip_lib, oracle_ctx, form, layout):
    model, paths, want, alone = stalled_batch(oracle_ctx)
    r = want[2]["result"]
    assert r["n_bisect_fail_rev"] + r["n_bisect_fail_fwd"] > 0 and (r["status_rev"] | r["status_fwd"]) & capi.ST_BISECT_FAIL, r
    assert (r["status_rev"] | r["status_fwd"]) & (capi.ST_MAX_INTEG_TIME | capi.ST_CAPACITY), r
    # its neighbours: planned as if it were not there
    others = [k for k in range(len(paths)) if k != 2]
    compare_plans([paths[k] for k in others], [want[k] for k in others], alone, "oracle, with and without the inadmissible path")
    assert all(want[k]["result"]["status_fwd"] == 0 and want[k]["result"]["status_rev"] == 0 for k in others)
    ctx = capi.Context(hip_lib, 0)
    helpers.set_layout(ctx, layout)
    got, launch = plan(ctx, paths, model, flags=PAIRS if form == "pairs" else 0, samples_from=want if form == "pairs" else None)
    ctx.close()
    compare_plans(paths, got, want, f"{form} x {layout}, launches {launch}")


# ---- 4. device libm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1deg", "4rad+3", "8deg+3"])
def test_device_libm_is_close(hip_ctx, oracle_ctx, name):
    """BATOTP_F_HOST_TRIG cleared: cos / sin of the device libm -- a1..a4 agree with the host-trig result to rounding of the
    trigonometric functions (no bit equality, no step counts)"""
    model, paths, want = batch(oracle_ctx, name)
    prob = capi.Problem.from_buffer_copy(bytes(paths[0].problem))
    prob.flags &= ~capi.F_HOST_TRIG
    b = capi.Batch(hip_ctx, prob, [p.n for p in paths], CAP)
    for k, p in enumerate(paths):
        b.upload_knots(k, [p.y], [p.sres])
    b.precompute(1)
    b.set_serial_model(model)
    b.precompute(2)
    dyn = [precomputed(b, prob, k)["dyn"] for k in range(len(paths))]
    b.close()
    err = np.zeros(4)
    for d, w in zip(dyn, want):
        scale = np.abs(w["dyn"]).max(axis=(1, 2))        # per coefficient family, on the path
        err = np.maximum(err, np.abs(d - w["dyn"]).max(axis=(1, 2)) / np.where(scale > 0, scale, 1.0))
    print(f"{name}: device libm against host trig tables, |difference| / max|family|: a1 {err[0]:.2e}, a2 {err[1]:.2e}, a3 {err[2]:.2e}, a4 {err[3]:.2e}")
    assert err.max() < DEVICE_LIBM_BOUND, (name, err)
    assert err[2] == 0.0       # (a3 takes no trigonometric function)
