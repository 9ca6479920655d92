"""GPU (-m gpu): the sweep kernels in the shapes the automatic plan picks between a thousand and sixteen thousand paths.

Part A forces a shape -- G lanes per path, P paths per wavefront with P odd, or not a power of two, or not filling the
wavefront -- on small batches of every problem family, so that a failure says whether the shape or the batch size is
responsible.  Part B leaves every developer switch automatic, runs batches on both sides of every batch-size threshold of
planSweep() (batotp_amd/csrc/batotp_hip.hip), asserts what was launched against a table of literal tuples and compares every
path with the oracle.  The table is the written record of the plan: a threshold that is moved on purpose is edited here in
the same change."""
import numpy as np
import pytest

import helpers
from helpers import assert_bit_equal, random_knots, set_layout
from batotp_amd import capi

pytestmark = pytest.mark.gpu

D = 127            # distinct paths of a part B batch: a prime, coprime to every paths-per-wavefront count and to 64
N_EQUAL = 33       # knots per path of the equal-length pools
CAP = 2500         # curve capacity: a stalled path ends on it quickly, 14 337 paths keep their two curves in 1.2 GB
COMPACT = capi.F_NO_SAMPLES | capi.F_COMPACT_SPLINES


# ---------------------------------------------------------------------------------------------
# problem families: a problem (the oracle's and the HIP library's flags), a pool of distinct paths, how a batch is prepared
# ---------------------------------------------------------------------------------------------
class Pool:
    """distinct paths of one family with the oracle's rows, curves and pointwise values (computed once per module run)"""

    def __init__(self, fam, ys, sres):
        self.fam, self.ys, self.sres = fam, ys, sres
        self.n = np.array([y.shape[1] for y in ys])
        self.aux = {}          # per distinct path: what prepare() uploads besides the knots (trig tables), kept from the oracle's run
        self.rows = self.curves = self.mvc = None


class Family:
    def __init__(self, name, oracle_prob, hip_flags=0):
        self.name, self.oprob = name, oracle_prob
        self.hprob = capi.Problem.from_buffer_copy(bytes(oracle_prob))
        self.hprob.flags |= hip_flags

    def paths(self, rng, lengths):
        raise NotImplementedError

    def prepare(self, b, pool, idx):
        b.precompute(0)


def _distinct_lengths(count, avoid=()):
    """knot counts of which any 101 consecutive ones differ (37 is a unit modulo 101)"""
    out, k = [], 0
    while len(out) < count:
        n = 16 + (37 * k) % 101
        k += 1
        if n not in avoid:
            out.append(n)
    return out


class VelAcc(Family):
    """joint velocity / acceleration limits only, six joints, the populations of the flat loop's canary: ordinary paths; paths on
    which the joint with a NEGATIVE acceleration limit moves (every bisection fails, the path ends on curve capacity); paths on
    which that joint hovers around the zero-velocity threshold (a failure now and then); paths that crawl under a tiny limit"""

    def __init__(self, name, hip_flags):
        rng = np.random.default_rng(4100)
        vmax = list(rng.uniform(1.0, 6.0, 6))
        amax = list(rng.uniform(5.0, 30.0, 4)) + [1e-7, -1.0]
        super().__init__(name, capi.make_problem(6, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=vmax, jnt_acc_max=amax, integ_res=0.02,
                                                 max_integ_time=1e5), hip_flags)

    def paths(self, rng, lengths):
        ys, sres = [], []
        for k, n in enumerate(lengths):
            y = random_knots(rng, 6, n, rng.uniform(0.3, 2.0))
            kind = k % 4
            if kind != 3:
                y[4] = 0.25                             # (kind 3 crawls)
            if kind in (0, 3):
                y[5] = 0.25                             # kind 0: ordinary
            elif kind == 2:
                y[5] *= 10.0 ** rng.uniform(-6.2, -5.6)     # hovers; kind 1: fails everywhere
            ys.append(np.ascontiguousarray(y))
            sres.append(float(rng.uniform(0.02, 0.2)))
        return ys, sres


class UploadedSites(Family):
    """velocity / acceleration limits on coefficient rows with the knot sites of every path uploaded and no longer sres * k: the
    kernels that search their segment instead of computing it (k_sweep<G, F, false>)"""

    def __init__(self, name):
        rng = np.random.default_rng(4200)
        super().__init__(name, capi.make_problem(6, 0, flags=capi.F_JNT_ACC_ON, jnt_vel_max=list(rng.uniform(1.0, 6.0, 6)),
                                                 jnt_acc_max=list(rng.uniform(5.0, 30.0, 6)), integ_res=0.02, max_integ_time=1e5))

    def paths(self, rng, lengths):
        ys = [random_knots(rng, 6, n, rng.uniform(0.3, 2.0)) for n in lengths]
        return ys, [float(rng.uniform(0.02, 0.2)) for _ in lengths]

    def prepare(self, b, pool, idx):
        b.precompute(0)
        for k, i in enumerate(idx):
            n, sres = int(pool.n[i]), pool.sres[i]
            sites = sres * np.arange(n, dtype=np.float64) * (1.0 + 1e-3 * np.sin(np.arange(n) + i))
            sites[0] = 0.0
            b.upload_path_sites(k, sites, 1.0 / sres, (1.0 / sres) * (1.0 / sres), 0)


class Cartesian(Family):
    """joint limits plus Cartesian speed and acceleration limits (solveQuadratic branch); the tool point stands still on a part
    of some paths"""

    def __init__(self, name):
        rng = np.random.default_rng(4300)
        flags = capi.F_JNT_ACC_ON | capi.F_CART_VEL_ON | capi.F_CART_ACC_ON
        super().__init__(name, capi.make_problem(5, 3, flags=flags, jnt_vel_max=list(rng.uniform(1, 6, 5)), jnt_acc_max=list(rng.uniform(2, 30, 5)),
                                                 cart_vel_max=float(rng.uniform(0.3, 2.0)), cart_acc_max=float(rng.uniform(0.5, 5.0)),
                                                 integ_res=0.02, max_integ_time=1e5))

    def paths(self, rng, lengths):
        ys, sres = [], []
        for n in lengths:
            th = random_knots(rng, 5, n, rng.uniform(0.3, 2.0))
            ca = random_knots(rng, 3, n, rng.uniform(0.1, 1.0))
            if rng.random() < 0.25:
                ca[:, n // 3: n // 2] = ca[:, n // 3: n // 3 + 1]
            ys.append(np.ascontiguousarray(np.vstack([th, ca])))
            sres.append(float(rng.uniform(0.02, 0.2)))
        return ys, sres


def _stalled_two_link_population():
    """problem and paths of test_two_link_arm_paths_that_never_finish (tests/test_gpu_fuzz.py), drawn in the same order"""
    rng = np.random.default_rng(3000)
    prob = capi.Problem.from_buffer_copy(bytes(helpers.Case("RR").problem))
    prob.flags = capi.F_TRQ_ON | capi.F_HOST_TRIG
    for j in range(2):
        prob.jnt_vel_max[j] = float(rng.uniform(100, 400)); prob.jnt_acc_max[j] = float(rng.uniform(500, 2000))
        prob.jnt_trq_max[j] = float(rng.uniform(5, 40)); prob.jnt_trq_min[j] = -float(rng.uniform(5, 40))
    ys = [random_knots(rng, 2, int(rng.integers(20, 400)), rng.uniform(20, 120)) for _ in range(int(rng.integers(2, 9)))]
    ys = [np.ascontiguousarray(np.vstack([y, np.zeros((prob.n_cart, y.shape[1]))])) for y in ys]
    sres = [float(rng.uniform(0.2, 2.0)) for _ in ys]
    return prob, ys, sres


class TwoLink(Family):
    """two-link arm with torque limits (serial dynamics, uploaded trigonometric terms) under the limits of the stalled population"""

    def __init__(self, name):
        prob, self.stalled_ys, self.stalled_sres = _stalled_two_link_population()
        prob.integ_res = 0.02
        super().__init__(name, prob)

    def paths(self, rng, lengths):
        # (under these limits gravity alone is too much in most poses: paths that start with the arm hanging or upright finish, the
        #  wider their swing the more of their bisections fail, and many stall)
        ys = []
        for n in lengths:
            y = random_knots(rng, 2, n, rng.uniform(5, 40))
            y[0] += float(rng.choice([-90.0, 0.0, 90.0])) - y[0, 0]
            y[1] += float(rng.choice([0.0, 180.0])) - y[1, 0]
            ys.append(np.ascontiguousarray(np.vstack([y, np.zeros((self.oprob.n_cart, n))])))
        return ys, [float(rng.uniform(0.5, 2.0)) for _ in lengths]

    def prepare(self, b, pool, idx):
        b.precompute(1)
        for k, i in enumerate(idx):
            if i not in pool.aux:   # (the oracle's run of the pool comes first: both implementations get the same arrays)
                pool.aux[i] = helpers.rr_trig(b.samples(k, 0)[0], b.samples(k, 1)[0])
            b.upload_rr_trig(k, pool.aux[i])
        b.precompute(2)


class Cable(Family):
    """3-cable robot: tension limits, cable velocity / acceleration limits, Cartesian speed limit; as a parallel mechanism (an LU
    solve per check) or converted to serial form with every channel as pairs"""

    def __init__(self, name, serial_pairs):
        rng = np.random.default_rng(4400)
        prob = capi.Problem.from_buffer_copy(bytes(helpers.Case("synth_cspr_s3").problem))
        prob.flags = capi.F_TRQ_ON | capi.F_PARALLEL | capi.F_JNT_ACC_ON | capi.F_CART_VEL_ON | (capi.F_PAR2SER if serial_pairs else 0)
        for j in range(3):
            prob.jnt_vel_max[j] = float(rng.uniform(2, 6)); prob.jnt_acc_max[j] = float(rng.uniform(4, 12))
            prob.jnt_trq_max[j] = float(rng.uniform(10, 16)); prob.jnt_trq_min[j] = float(rng.uniform(0.5, 1.5))
        prob.cart_vel_max = float(rng.uniform(2, 5))
        prob.integ_res = 0.02
        super().__init__(name, prob, COMPACT if serial_pairs else 0)

    def paths(self, rng, lengths):
        pm = np.array(list(self.oprob.pmat)).reshape(3, 3)
        ys, sres = [], []
        for k, n in enumerate(lengths):
            t = np.linspace(0, 1, n)
            amp = 1.0 if k % 5 else 2.2      # every fifth platform path leaves the region the tension limits admit
            cart = np.stack([amp * np.sin(2 * np.pi * t * rng.uniform(0.3, 1.5) + rng.uniform(0, 6)),
                             amp * np.cos(2 * np.pi * t * rng.uniform(0.3, 1.5) + rng.uniform(0, 6)) + 0.4,
                             3.0 + 0.8 * np.sin(2 * np.pi * t * rng.uniform(0.2, 1.0) + rng.uniform(0, 6))])
            theta = np.stack([np.sqrt(((cart - pm[:, q:q + 1]) ** 2).sum(axis=0)) for q in range(3)])
            ys.append(np.ascontiguousarray(np.vstack([theta, cart])))
            sres.append(float(rng.uniform(0.03, 0.2)))
        return ys, sres


_FAMILIES = {
    "va_rows": lambda: VelAcc("va_rows", 0),               # FEAT 0
    "va_compact": lambda: VelAcc("va_compact", COMPACT),   # FEAT -1
    "cartesian": lambda: Cartesian("cartesian"),           # FEAT 1
    "two_link": lambda: TwoLink("two_link"),               # FEAT 2
    "cable_parallel": lambda: Cable("cable_parallel", False),   # FEAT 3
    "sites": lambda: UploadedSites("sites"),               # FEAT 0 on searched segments
    "cable_pairs": lambda: Cable("cable_pairs", True),     # FEAT 2 on pairs for all channels: k_sweep1 only
}
_SEED = {"va_rows": 12, "va_compact": 12, "cartesian": 12, "two_link": 15, "cable_parallel": 14, "sites": 15, "cable_pairs": 14}
_pools = {}


def run_batch(ctx, prob, pool, idx, curves_of=(), mvc=False):
    """the batch made of the pool's paths idx through the library behind ctx: (rows, {k: (reverse, forward curve)}, {k: pointwise values},
    (reverse launch, forward launch) where the library records it)"""
    fam = pool.fam
    b = capi.Batch(ctx, prob, [int(pool.n[i]) for i in idx], CAP)
    b.upload_knots(0, [pool.ys[i] for i in idx], [pool.sres[i] for i in idx])
    fam.prepare(b, pool, idx)
    if mvc:
        b.pointwise_mvc()
    b.sweep(-1); b.sweep(+1)
    rows = b.results()
    launch = (b.last_sweep_launch(-1), b.last_sweep_launch(+1)) if hasattr(ctx.library.lib, "batotp_hip_last_sweep_launch") and prob is not fam.oprob else None
    cur = {k: (b.curve(k, -1), b.curve(k, +1)) for k in curves_of}
    mv = {k: np.stack(b.mvc(k)) for k in curves_of} if mvc else {}
    b.close()
    return rows, cur, mv, launch


def pool_of(oracle_ctx, family, kind):
    """kind "distinct": every path its own knot count (part A; the two-link pool includes the stalled population);
    "equal": D paths of N_EQUAL knots; "classes": D paths in five length classes (part B)"""
    key = (family, kind)
    if key not in _pools:
        fam = _FAMILIES[family]()
        rng = np.random.default_rng(8800 + _SEED[family])
        if kind == "distinct":
            head = getattr(fam, "stalled_ys", [])
            lengths = _distinct_lengths(D - len(head), avoid={y.shape[1] for y in head})
        elif kind == "equal":
            head, lengths = [], [N_EQUAL] * D
        else:
            head, lengths = [], [(20, 27, 34, 41, 48)[k % 5] for k in range(D)]
        ys, sres = fam.paths(rng, lengths)
        for j, y in enumerate(head):      # ... at every third place from the second on, so that its paths share wavefronts with others
            ys.insert(3 * j + 1, y); sres.insert(3 * j + 1, fam.stalled_sres[j])
        pool = Pool(fam, ys, sres)
        pool.stalled_at = [3 * j + 1 for j in range(len(head))]
        every = range(len(ys))
        pool.rows, pool.curves, pool.mvc, _ = run_batch(oracle_ctx, fam.oprob, pool, list(every), curves_of=every, mvc=True)
        _pools[key] = pool
    return _pools[key]


def compare(pool, idx, rows, cur, mv, what):
    """rows of every path of the batch, curves and pointwise values of the paths that were fetched, against the oracle's"""
    idx = np.asarray(idx)
    for f in rows.dtype.names:
        want = pool.rows[f][idx]
        same = (rows[f].view(np.uint64) == want.view(np.uint64)) if rows[f].dtype == np.float64 else (rows[f] == want)
        if not np.all(same):
            bad = np.flatnonzero(~same)
            raise AssertionError(f"{what}: result field {f} differs on {bad.size} of {idx.size} paths, first {bad[:8].tolist()} "
                                 f"(distinct paths {idx[bad[:8]].tolist()}): {rows[f][bad[:4]].tolist()} against the oracle's {want[bad[:4]].tolist()}")
    for k, (rev, fwd) in cur.items():
        orev, ofwd = pool.curves[int(idx[k])]
        assert_bit_equal(rev[0], orev[0], f"{what} path {k} reverse s"); assert_bit_equal(rev[1], orev[1], f"{what} path {k} reverse sdot")
        assert_bit_equal(fwd[0], ofwd[0], f"{what} path {k} forward s"); assert_bit_equal(fwd[1], ofwd[1], f"{what} path {k} forward sdot")
    for k, m in mv.items():
        assert_bit_equal(m, pool.mvc[int(idx[k])], f"{what} path {k} pointwise values")


# ---------------------------------------------------------------------------------------------
# part A: forced shapes on small batches
# ---------------------------------------------------------------------------------------------
SHAPES = ["8x2", "8x3", "8x4", "8x5", "8x6", "8x7", "4x3", "4x7", "4x13", "2x5", "2x19", "16x2", "16x3", "16x4", "32x2"]


def _batch_size(ppw):
    """more than four wavefronts (one block), their number no multiple of 4, the last one partly filled, at least 17 paths"""
    rest = max(1, ppw // 2)
    waves = 6
    while waves % 4 == 0 or (waves - 1) * ppw + rest < 17:
        waves += 1
    assert rest < ppw
    return (waves - 1) * ppw + rest, waves


def _loop_forms(family, lanes):
    """(hold of the stage, hold of the reverse sweep's certificate phase) to run: nested loops everywhere; the flat loop, which exists for
    velocity / acceleration-only problems on 2, 4 and 8 lanes, with hold 4 / 8 and the certificate phase off, at 1 and automatic"""
    forms = [((-1, -1), -1)]
    if family in ("va_rows", "va_compact") and lanes in (2, 4, 8):
        forms += [((4, 8), 0), ((4, 8), 1), ((4, 8), -1)]
    return forms


def _forced(hip_lib, pool, shape, idx, forms, what):
    lanes, ppw = (int(v) for v in shape.split("x"))
    for hold, cert in forms:
        ctx = capi.Context(hip_lib, 0)
        set_layout(ctx, shape)
        ctx.set_sweep_hold(*hold)
        ctx.set_cert_hold(cert)
        rows, cur, mv, launch = run_batch(ctx, pool.fam.hprob, pool, idx, curves_of=range(len(idx)), mvc=True)
        ctx.close()
        # a shape that was silently clamped or replaced does not count as covered
        assert launch[0] == (lanes, ppw, hold[0]) and launch[1] == (lanes, ppw, hold[1]), (what, hold, launch)
        compare(pool, idx, rows, cur, mv, f"{what} hold {hold} certificate hold {cert}")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", ["va_rows", "va_compact", "cartesian", "two_link", "cable_parallel", "sites"])
def test_forced_paths_per_wavefront(hip_lib, oracle_ctx, family, shape):
    """G lanes per path, P paths per wavefront with the other lane groups idle from the start, a wavefront count that fills no whole
    number of blocks and a last wavefront that is partly filled: rows, both curves and pointwise values of every path equal the oracle's"""
    lanes, ppw = (int(v) for v in shape.split("x"))
    pool = pool_of(oracle_ctx, family, "distinct")
    B, waves = _batch_size(ppw)
    idx = list(range(B))
    assert waves > 4 and waves % 4 and (waves - 1) * ppw < B < waves * ppw and waves == -(-B // ppw)
    ora = pool.rows[:B]
    for w in range(waves):
        of_wave = slice(w * ppw, min(B, (w + 1) * ppw))
        if of_wave.stop - of_wave.start > 1:   # the paths that share a wavefront differ in length and in step count
            assert len(set(pool.n[of_wave].tolist())) == of_wave.stop - of_wave.start, (w, pool.n[of_wave])
            assert len(set(ora["steps_rev"][of_wave].tolist())) > 1, (w, ora["steps_rev"][of_wave])
    if family in ("va_rows", "va_compact"):
        # the canary's populations, judged by the oracle alone
        status = ora["status_rev"] | ora["status_fwd"]
        finished = int(np.count_nonzero((status & ~np.uint32(capi.ST_BISECT_FAIL)) == 0))
        on_capacity = int(np.count_nonzero(status & capi.ST_CAPACITY))
        failed = int(np.count_nonzero(ora["n_bisect_fail_rev"] + ora["n_bisect_fail_fwd"] > 0))
        assert finished >= 4 and on_capacity >= 4 and failed >= 4, (finished, on_capacity, failed)
    if family == "two_link":
        at = pool.stalled_at      # the population of test_two_link_arm_paths_that_never_finish is part of every batch
        assert at and max(at) < B and int(ora["n_bisect_fail_rev"][at].max()) > 1000 and int((ora["status_rev"][at] & capi.ST_CAPACITY != 0).sum()) >= 3
    _forced(hip_lib, pool, shape, idx, _loop_forms(family, lanes), f"{family} {shape}")


@pytest.mark.parametrize("family", ["va_rows", "va_compact", "cartesian", "two_link", "cable_parallel", "sites"])
def test_single_path_with_seven_paths_per_wavefront(hip_lib, oracle_ctx, family):
    """a batch of ONE path in a wavefront laid out for seven (velocity / acceleration-only: one path of each population)"""
    pool = pool_of(oracle_ctx, family, "distinct")
    for i in (0, 1, 2, 3) if family in ("va_rows", "va_compact") else (0,):
        _forced(hip_lib, pool, "8x7", [i], _loop_forms(family, 8), f"{family} path {i} alone in 8x7")


# ---------------------------------------------------------------------------------------------
# the software prefetch of the general kernel (batotp_hip_set_sweep_prefetch): "never changes a result"
# ---------------------------------------------------------------------------------------------
# SweepArgs::touch is read by k_sweep alone -- its nested loops (bit 0: touch_ahead, bit 1, forward sweep: touch_curve_ahead) and its
# own flat instantiation (bit 0) -- and by neither k_sweep8 nor k_sweep1, so every configuration forces a shape that k_sweep runs.
# Both touches clamp their address into the path's own arrays: [row 0, row n - 1] of the spline rows or pairs, and [point 0, point
# nMvc - 1] of the reverse curve; the forward sweep of k_sweep returns before its first touch when the reverse curve has fewer than two
# points, so nMvc - 1 >= 1 wherever touch_curve_ahead runs.
PREFETCH = [(0, 0), (1, 1), (0, 2), (1, 3), (-1, -1)]
PREFETCH_SHAPES = {
    # name: (layout of helpers.set_layout, problem flags, launch on record)
    "rows_32x1": ("32", 0, (32, 1, -1)),            # one path per wavefront: the automatic setting touches rows and curve
    "rows_16x3": ("16x3", 0, (16, 3, -1)),          # several paths per wavefront: the automatic setting never sets the forward bits
    "compact_32x1": ("32", COMPACT, (32, 1, -1)),   # the pair stream (FEAT < 0)
    "rows_flat_8x8": ("oldflat4", 0, (8, 8, 4)),    # k_sweep's own flat loop instead of k_sweep8
}
_prefetch_ref = []


def _prefetch_batch(oracle_ctx):
    """five paths of 4 knots (a reverse curve of 23 points, the shortest here) .. the full golden length, and the oracle's run of them"""
    if not _prefetch_ref:
        g, s = helpers.Case("GEN7DOF"), helpers.Case("synth_gen7dof_s0")
        cuts = [helpers.PrefixCase(c, n, g.problem) for c, n in ((g, 4), (s, 37), (g, g.n), (s, 300), (g, 120))]
        _prefetch_ref.append((cuts, helpers.run_pipeline(oracle_ctx, cuts, mvc=False, details=False)))
    return _prefetch_ref[0]


@pytest.mark.parametrize("touch", PREFETCH, ids=lambda t: f"touch{t[0]}_{t[1]}")
@pytest.mark.parametrize("shape", list(PREFETCH_SHAPES))
def test_prefetch_switch_never_changes_a_result(hip_lib, oracle_ctx, shape, touch):
    cuts, ref = _prefetch_batch(oracle_ctx)
    layout, flags, launch = PREFETCH_SHAPES[shape]
    ctx = capi.Context(hip_lib, 0)
    set_layout(ctx, layout)
    ctx.set_sweep_prefetch(*touch)
    prob = capi.Problem.from_buffer_copy(bytes(cuts[0].problem))
    prob.flags |= flags
    b = capi.Batch(ctx, prob, [c.n for c in cuts], max(c.max_steps() for c in cuts))
    for k, c in enumerate(cuts):
        b.upload_knots(k, [c.y], [c.sres])
    b.optimize()
    rows = b.results()
    assert b.last_sweep_launch(-1) == launch and b.last_sweep_launch(+1) == launch, (b.last_sweep_launch(-1), b.last_sweep_launch(+1))
    for k, o in enumerate(ref):
        what = f"{shape} prefetch {touch} path {k}"
        for f in rows.dtype.names:
            assert rows[k][f] == o["result"][f], (what, f, rows[k][f], o["result"][f])
        for which, key in ((-1, "rev"), (+1, "fwd")):
            s, sd = b.curve(k, which)
            assert_bit_equal(s, o[key][0], f"{what} {key} s"); assert_bit_equal(sd, o[key][1], f"{what} {key} sdot")
    b.close(); ctx.close()


# ---------------------------------------------------------------------------------------------
# part B: the automatic plan at its switching sizes.  (lanes per path, paths per wavefront, hold) of the reverse and of the forward
# sweep; H4 / H8: hold 4 / 8 of the flat loop where its gate is open (flat_loop_status() == 1), the nested loops (-1) otherwise
# ---------------------------------------------------------------------------------------------
H4, H8 = "H4", "H8"
_K1, _K1x2 = (64, 1, -1), (64, 2, -1)     # the one-path-per-wavefront kernel with one and with two paths
PLAN = {
    "va_compact": {
        2304: (_K1, _K1), 2305: (_K1, _K1x2), 3500: (_K1, _K1x2), 3501: (_K1x2, _K1x2), 5000: (_K1x2, _K1x2),
        5001: (_K1x2, (8, 4, H8)), 7600: (_K1x2, (8, 4, H8)), 7601: ((8, 4, H4), (8, 4, H8)), 8193: ((8, 5, H4), (8, 5, H8)),
        10241: ((8, 6, H4), (8, 6, H8)), 12289: ((8, 7, H4), (8, 7, H8)), 14336: ((8, 7, H4), (8, 7, H8)), 14337: ((8, 8, H4), (8, 8, H8)),
    },
    "va_rows": {
        3072: (_K1, _K1), 3073: (_K1, (8, 4, H8)), 4096: (_K1, (8, 4, H8)), 4097: (_K1, (8, 4, H8)), 4608: (_K1, (8, 4, H8)),
        4609: ((8, 3, H4), (8, 4, H8)), 6145: ((8, 4, H4), (8, 4, H8)), 8193: ((8, 5, H4), (8, 5, H8)), 10241: ((8, 6, H4), (8, 6, H8)),
        12289: ((8, 7, H4), (8, 7, H8)), 14337: ((8, 8, H4), (8, 8, H8)),
    },
    "cartesian": {
        3072: (_K1, _K1), 3073: (_K1, (8, 4, -1)), 4608: (_K1, (8, 4, -1)), 4609: ((8, 3, -1), (8, 4, -1)), 6145: ((8, 4, -1), (8, 4, -1)),
        8193: ((8, 5, -1), (8, 5, -1)), 10241: ((8, 6, -1), (8, 6, -1)), 12289: ((8, 7, -1), (8, 7, -1)), 14337: ((8, 8, -1), (8, 8, -1)),
    },
    "two_link": {
        3072: (_K1, _K1), 3073: (_K1, (8, 4, -1)), 4608: (_K1, (8, 4, -1)), 4609: ((8, 3, -1), (8, 4, -1)), 6145: ((8, 4, -1), (8, 4, -1)),
        8193: ((8, 5, -1), (8, 5, -1)), 10241: ((8, 6, -1), (8, 6, -1)), 12289: ((8, 7, -1), (8, 7, -1)), 14337: ((8, 8, -1), (8, 8, -1)),
    },
    "cable_parallel": {
        1024: ((32, 1, -1), (32, 1, -1)), 1025: ((32, 1, -1), (8, 2, -1)), 2048: ((32, 1, -1), (8, 2, -1)), 2049: ((8, 2, -1), (8, 3, -1)),
        3073: ((8, 2, -1), (8, 4, -1)), 4097: ((8, 3, -1), (8, 4, -1)), 6144: ((8, 3, -1), (8, 4, -1)), 6145: ((8, 4, -1), (8, 4, -1)),
        8193: ((8, 5, -1), (8, 5, -1)), 10241: ((8, 6, -1), (8, 6, -1)), 12289: ((8, 7, -1), (8, 7, -1)), 14337: ((8, 8, -1), (8, 8, -1)),
    },
    "sites": {
        1024: ((32, 1, -1), (32, 1, -1)), 1025: ((32, 1, -1), (8, 2, -1)), 2048: ((32, 1, -1), (8, 2, -1)), 2049: ((8, 2, -1), (8, 3, -1)),
        3073: ((8, 2, -1), (8, 4, -1)), 4097: ((8, 3, -1), (8, 4, -1)), 6144: ((8, 3, -1), (8, 4, -1)), 6145: ((8, 4, -1), (8, 4, -1)),
        8193: ((8, 5, -1), (8, 5, -1)), 10241: ((8, 6, -1), (8, 6, -1)), 12289: ((8, 7, -1), (8, 7, -1)), 14337: ((8, 8, -1), (8, 8, -1)),
    },
    "cable_pairs": {2304: (_K1, _K1), 2305: (_K1x2, _K1x2)},
}
# one ragged batch per family (five length classes), at a size where the two sweeps run different kernels or shapes
RAGGED = {"va_compact": 5001, "va_rows": 4609, "cartesian": 4609, "two_link": 3073, "cable_parallel": 2049, "sites": 4097, "cable_pairs": 2305}


def _expected(ctx, plan):
    gate = ctx.flat_loop_status() == 1
    hold = {H4: 4 if gate else -1, H8: 8 if gate else -1}
    return tuple((lanes, ppw, hold.get(h, h)) for lanes, ppw, h in plan)


def _automatic(hip_lib, pool, B, plan, order_mode, what):
    ctx = capi.Context(hip_lib, 0)
    ctx.set_sweep_group(0); ctx.set_paths_per_wave(0); ctx.set_sweep_hold(-2, -2); ctx.set_cert_hold(-1)
    if order_mode is not None:
        ctx.set_path_order(order_mode)
    idx = np.arange(B) % D
    # launch order: the order given, or (ragged batches, default) longest path first with the order given among equals
    order = np.arange(B) if order_mode == 0 else np.argsort(-pool.n[idx], kind="stable")
    edge = 2 * max(plan[0][1], plan[1][1])          # the first two and the last two wavefronts of either sweep
    others = np.random.default_rng(B).choice(order[edge:-edge], 256, replace=False)
    fetch = sorted(set(order[:edge].tolist()) | set(order[-edge:].tolist()) | set(others.tolist()))
    rows, cur, _, launch = run_batch(ctx, pool.fam.hprob, pool, idx.tolist(), curves_of=fetch)
    want = _expected(ctx, plan)
    ctx.close()
    assert launch == want, f"{what}: launched {launch}, the plan on record is {want}"
    compare(pool, idx, rows, cur, {}, what)


@pytest.mark.parametrize("family,B", [(f, B) for f, sizes in PLAN.items() for B in sizes])
def test_automatic_plan_at_its_switching_sizes(hip_lib, oracle_ctx, family, B):
    """B paths, path p a copy of distinct path p mod 127 (equal knot counts: launch slot = path index, so the neighbours in a wavefront
    are different paths), every switch automatic: the launch of either sweep is the one on record, the row of EVERY path and the curves of
    the first two and last two wavefronts and of 256 other paths are the oracle's"""
    pool = pool_of(oracle_ctx, family, "equal")
    _automatic(hip_lib, pool, B, PLAN[family][B], None, f"{family} B={B}")


@pytest.mark.parametrize("order_mode", [0, 1])
@pytest.mark.parametrize("family", list(RAGGED))
def test_automatic_plan_on_ragged_batches(hip_lib, oracle_ctx, family, order_mode):
    """the same with five length classes, in the order given and longest first (the default): within a class the copies keep the order
    given, so a wavefront still holds different paths"""
    pool = pool_of(oracle_ctx, family, "classes")
    B = RAGGED[family]
    _automatic(hip_lib, pool, B, PLAN[family][B], order_mode, f"{family} ragged B={B} path order {order_mode}")
