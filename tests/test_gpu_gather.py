"""GPU (-m gpu): the send side of the multi-GPU curve gather -- batotp_hip_pack_curves / k_curves_pack -- and batotp_amd.dist on
device memory.

Every comparison is bit for bit.  The packed rows are compared with Batch.curve (the per-path download) and with the oracle's
curves; the destination always has 64 guard rows on both sides, filled with a bit pattern no computation produces, and every
row the call must not write is checked for it.  The oracle shim's batotp_hip_pack_curves (oracle/abi_shim.c) is the plain
statement of the status and of *total_points on every error path.

Device memory of tests a - c comes from the HIP runtime the library itself is bound to (hipMalloc through ctypes): a process that
has loaded the library first cannot give torch a GPU any more (torch brings a HIP runtime of its own, and the second runtime of a
process finds no device), and every GPU test that runs before these has loaded the library.  The product's order -- torch first,
then the library, one runtime -- is the order of the child processes of tests d and e."""
import ctypes as C
import os
import re
import traceback

import numpy as np
import pytest

import helpers
from helpers import assert_bit_equal
from batotp_amd import capi
from test_dist_gloo import _free_port, _worker

pytestmark = pytest.mark.gpu


def _header_constant(name):
    text = open(os.path.join(helpers.ROOT, "include", "batotp_hip.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(-?\d+)", text).group(1))


ERR_ARG, ERR_STATE = _header_constant("BATOTP_ERR_ARG"), _header_constant("BATOTP_ERR_STATE")
GUARD = 64                           # rows in front of and behind the destination
SENTINEL = 0x7FF4DEADBEEF5A5A        # a signalling-NaN payload: neither a curve value nor what a fresh allocation holds by accident
COMPACT = capi.F_NO_SAMPLES | capi.F_COMPACT_SPLINES


_ref = {}


def ragged(oracle_ctx):
    """(cuts, the oracle's run of them): eight paths of 4 .. 3329 knots, every curve length different"""
    if "ragged" not in _ref:
        cuts = _cuts()
        out = helpers.run_pipeline(oracle_ctx, cuts, mvc=False, details=False)
        for w in ("n_rev", "n_fwd"):
            counts = [int(o["result"][w]) for o in out]
            assert min(counts) >= 2 and len(set(counts)) == len(counts), counts
        _ref["ragged"] = (cuts, out)
    return _ref["ragged"]


_hip = None


def hip_runtime():
    """the HIP runtime the product library runs on (already in the process: loading the library has loaded it)"""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7", mode=os.RTLD_NOLOAD | os.RTLD_NOW)
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


H2D, D2H = 1, 2     # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


class Guarded:
    """a device buffer of `points` (s, sdot) rows with GUARD sentinel rows on both sides; the library gets the pointer of row GUARD"""

    def __init__(self, points):
        self.hip, self.points = hip_runtime(), points
        self.n_rows = points + 2 * GUARD
        self.base = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.base), self.n_rows * 16) == 0
        self.ptr = self.base.value + GUARD * 16
        self.fill()

    def fill(self):
        h = np.full((self.n_rows, 2), SENTINEL, dtype=np.uint64)
        assert self.hip.hipMemcpy(self.base, h.ctypes.data_as(C.c_void_p), h.nbytes, H2D) == 0

    def bits(self):
        h = np.empty((self.n_rows, 2), dtype=np.uint64)
        assert self.hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), self.base, h.nbytes, D2H) == 0
        return h

    def rows(self, used, what):
        """the first `used` rows of the destination; every other row of the buffer must still hold the sentinel"""
        h = self.bits()
        untouched = np.concatenate([h[:GUARD], h[GUARD + used:]])
        bad = np.argwhere(untouched != SENTINEL)
        assert bad.size == 0, f"{what}: {bad.shape[0]} values outside the {used} packed rows were written, first at {bad[:4].tolist()}"
        return h[GUARD:GUARD + used].view(np.float64)

    def close(self):
        if self.base:
            self.hip.hipFree(self.base)
            self.base = C.c_void_p()

    def __del__(self):
        self.close()


def raw_pack(b, which, path0, n_paths, ptr, dst_points, total_init=-77):
    """batotp_hip_pack_curves without the exception of Batch.pack_curves: (status, *total_points)"""
    total = C.c_int64(total_init)
    rc = b.lib.batotp_hip_pack_curves(b.handle, which, path0, n_paths, C.c_void_p(ptr), dst_points, C.byref(total))
    return rc, int(total.value)


def make_batch(ctx, cuts, flags=0, margin=0):
    prob = capi.Problem.from_buffer_copy(bytes(cuts[0].problem))
    prob.flags |= flags
    cap = max(c.max_steps() for c in cuts) + margin
    if flags & capi.F_MVC_IN_CURVES:
        cap = max(cap, (3 * max(c.n for c in cuts) + 1) // 2)
    b = capi.Batch(ctx, prob, [c.n for c in cuts], cap)
    for k, c in enumerate(cuts):
        b.upload_knots(k, [c.y], [c.sres])
    return b


def check_pack(b, which, ref, what, from_batch=True):
    """pack every path of the batch: total, content against the oracle (and against the per-path download), guard rows"""
    key, cnt = ("fwd", "n_fwd") if which == 1 else ("rev", "n_rev")
    counts = [int(v) for v in b.results()[cnt]]
    assert counts == [int(o["result"][cnt]) for o in ref], (what, counts)
    buf = Guarded(sum(counts))
    total = b.pack_curves(which, 0, b.n_paths, buf.ptr, buf.points)
    assert total == sum(counts), (what, total, counts)
    rows = buf.rows(total, what)
    at = 0
    for k, c in enumerate(counts):
        part = rows[at:at + c]
        at += c
        assert_bit_equal(part[:, 0], ref[k][key][0], f"{what} path {k} s against the oracle")
        assert_bit_equal(part[:, 1], ref[k][key][1], f"{what} path {k} sdot against the oracle")
        if from_batch:
            s, sd = b.curve(k, which)
            assert_bit_equal(part[:, 0], s, f"{what} path {k} s against Batch.curve")
            assert_bit_equal(part[:, 1], sd, f"{what} path {k} sdot against Batch.curve")


# ---------------------------------------------------------------------------------------------
# a. packed curves of real sweeps, in every curve layout and from every sweep kernel that writes them
# ---------------------------------------------------------------------------------------------
LAYOUTS = {
    # name: (sweep-kernel layout of helpers.set_layout or None, hold, problem flags, launch of either sweep on record)
    "rows_auto": (None, None, 0, ((64, 1, -1), (64, 1, -1))),
    "k_sweep1": (64, None, 0, ((64, 1, -1), (64, 1, -1))),
    "k_sweep8": ("8x8", (4, 8), 0, ((8, 8, 4), (8, 8, 8))),
    "compact": (None, None, COMPACT, ((64, 1, -1), (64, 1, -1))),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_packed_curves_of_a_ragged_batch(hip_lib, oracle_ctx, layout):
    """eight paths of 4 .. 3329 knots through optimize(): both packs equal the per-path downloads and the oracle's curves, the
    total is the sum of the result rows' counts, no guard row is written"""
    cuts, ref = ragged(oracle_ctx)
    shape, hold, flags, launch = LAYOUTS[layout]
    ctx = capi.Context(hip_lib, 0)
    if shape is not None:
        helpers.set_layout(ctx, shape)
    if hold is not None:
        ctx.set_sweep_hold(*hold)
    b = make_batch(ctx, cuts, flags)
    b.optimize()
    assert (b.last_sweep_launch(-1), b.last_sweep_launch(+1)) == launch
    for which in (-1, +1):
        check_pack(b, which, ref, f"{layout} which {which}")
    b.close(); ctx.close()


def test_packed_curves_in_place(hip_ctx, oracle_ctx):
    """BATOTP_F_CURVES_IN_PLACE: the forward curve after optimize(); the reverse curve is gone (state error, *total_points = 0,
    nothing written) until the reverse sweep has run again"""
    cuts, ref = ragged(oracle_ctx)
    b = make_batch(hip_ctx, cuts, capi.F_CURVES_IN_PLACE, margin=16)
    b.optimize()
    check_pack(b, +1, ref, "in place, forward")
    buf = Guarded(sum(int(o["result"]["n_rev"]) for o in ref))
    assert raw_pack(b, -1, 0, b.n_paths, buf.ptr, buf.points) == (ERR_STATE, 0)
    buf.rows(0, "in place, reverse curve gone")
    b.sweep(-1)
    check_pack(b, -1, ref, "in place, reverse sweep run again")
    b.close()


def test_packs_after_a_pointwise_evaluation_into_the_curve_slots(hip_ctx, oracle_ctx):
    """BATOTP_F_MVC_IN_CURVES: a pointwise evaluation after the sweeps overwrites the curve slots: both packs report the state error"""
    cuts, ref = ragged(oracle_ctx)
    b = make_batch(hip_ctx, cuts, capi.F_MVC_IN_CURVES)
    b.optimize()
    for which in (-1, +1):
        check_pack(b, which, ref, f"values in the curve slots, which {which}")
    b.pointwise_mvc()
    buf = Guarded(sum(int(o["result"]["n_fwd"]) for o in ref))
    for which in (-1, +1):
        assert raw_pack(b, which, 0, b.n_paths, buf.ptr, buf.points) == (ERR_STATE, 0), which
    buf.rows(0, "curve slots overwritten by the pointwise evaluation")
    b.close()


# ---------------------------------------------------------------------------------------------
# b. sub-ranges and arguments
# ---------------------------------------------------------------------------------------------
def test_sub_ranges_and_arguments(hip_ctx, oracle_ctx):
    cuts, ref = ragged(oracle_ctx)
    B = len(cuts)
    b = make_batch(hip_ctx, cuts)
    # before any sweep: nothing to pack, and that is not an error
    for which in (-1, +1):
        assert raw_pack(b, which, 0, B, 0, 0) == (0, 0), which
    b.optimize()
    biggest = sum(int(o["result"]["n_fwd"]) for o in ref)
    buf = Guarded(biggest)
    for which, key, cnt in ((-1, "rev", "n_rev"), (+1, "fwd", "n_fwd")):
        counts = [int(o["result"][cnt]) for o in ref]
        for path0 in (0, 1, B - 1):
            for n_paths in sorted({0, 1, 2, B - path0}):
                if path0 + n_paths > B:
                    continue
                what = f"which {which} paths [{path0}, {path0 + n_paths})"
                total = sum(counts[path0:path0 + n_paths])
                buf.fill()
                # room for exactly the total
                assert raw_pack(b, which, path0, n_paths, buf.ptr, total) == (0, total), what
                rows = buf.rows(total, what)
                want_s = np.concatenate([ref[k][key][0] for k in range(path0, path0 + n_paths)] + [np.zeros(0)])
                want_sd = np.concatenate([ref[k][key][1] for k in range(path0, path0 + n_paths)] + [np.zeros(0)])
                assert_bit_equal(rows[:, 0], want_s, what + " s"); assert_bit_equal(rows[:, 1], want_sd, what + " sdot")
                if total:
                    # one row too few, no destination: an argument error that still reports the size, and nothing is written
                    buf.fill()
                    assert raw_pack(b, which, path0, n_paths, buf.ptr, total - 1) == (ERR_ARG, total), what
                    assert raw_pack(b, which, path0, n_paths, 0, total) == (ERR_ARG, total), what
                    buf.rows(0, what + " refused")
    buf.fill()
    for which, path0, n_paths in ((1, 0, B + 1), (1, 1, B), (-1, B, 1), (1, B + 1, 0), (1, -1, 1), (-1, 0, -1), (1, -1, -1), (0, 0, B), (2, 0, B), (-2, 0, 1)):
        assert raw_pack(b, which, path0, n_paths, buf.ptr, buf.points)[0] == ERR_ARG, (which, path0, n_paths)
    assert raw_pack(b, 1, 0, B, buf.ptr, -1)[0] == ERR_ARG
    assert b.lib.batotp_hip_pack_curves(b.handle, 1, 0, B, C.c_void_p(buf.ptr), buf.points, None) == ERR_ARG
    buf.rows(0, "refused arguments")
    assert raw_pack(b, 1, B, 0, buf.ptr, buf.points) == (0, 0)     # the empty range at the end is a range
    b.close()


# ---------------------------------------------------------------------------------------------
# c. synthetic curves at the kernel's own boundaries
# ---------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 255, 256, 0, 513]


def _named(path, n):
    s = path * float(1 << 20) + np.arange(n, dtype=np.float64)
    return s, -s


def test_every_packed_point_is_the_one_its_path_and_index_name(hip_ctx):
    """reverse curves of 0, 1, 255, 256, 0 and 513 points whose values name their path and index, packed over every contiguous range
    of paths: empty paths first, in the middle and last in a range (equal entries of the offset table), a single-point path, totals
    of 255, 256, 511, 512, 513, 769, 1024 and 1025 points around the 256-thread block, curves that start 987 .. 1499 points into
    their slot.

    batotp_hip_upload_curve takes curves of at least two points (like the oracle's; a reverse sweep publishes no shorter one), so
    the single point is the LAST point of an uploaded pair with n_rev of the path's result row set to 1 through
    batotp_hip_results_device_ptr: the reverse curve ends at the end of its slot, so the curve of n_rev = 1 is that point."""
    g = helpers.Case("GEN7DOF")
    B = len(LENGTHS)
    cap = 1500
    b = capi.Batch(hip_ctx, g.problem, [4] * B, cap)
    b.upload_knots(0, [g.y[:, :4]] * B, [g.sres] * B)
    for p, n in enumerate(LENGTHS):
        if n >= 2:
            b.upload_curve(p, *_named(p, n))
        elif n == 1:
            s, sd = _named(p, 1)
            b.upload_curve(p, np.array([-1.0, s[0]]), np.array([-2.0, sd[0]]))
    # n_rev of path 1: 2 -> 1, written in place in the device result table
    ptr, nbytes = b.results_device_ptr()
    assert nbytes == B * capi.RESULT_DTYPE.itemsize
    rows = b.results()
    assert [int(v) for v in rows["n_rev"]] == [0, 2, 255, 256, 0, 513]
    rows["n_rev"][1] = 1
    assert hip_runtime().hipMemcpy(C.c_void_p(ptr), rows.ctypes.data_as(C.c_void_p), nbytes, H2D) == 0
    assert [int(v) for v in b.results()["n_rev"]] == LENGTHS
    s1, sd1 = b.curve(1, -1)
    assert s1.tolist() == [float(1 << 20)] and sd1.tolist() == [-float(1 << 20)]

    buf = Guarded(sum(LENGTHS))
    totals = set()
    for p0 in range(B + 1):
        for p1 in range(p0, B + 1):
            what = f"paths [{p0}, {p1})"
            total = sum(LENGTHS[p0:p1])
            totals.add(total)
            buf.fill()
            assert raw_pack(b, -1, p0, p1 - p0, buf.ptr, total) == (0, total), what
            got = buf.rows(total, what)
            want = [_named(p, LENGTHS[p]) for p in range(p0, p1)]
            assert_bit_equal(got[:, 0], np.concatenate([w[0] for w in want] + [np.zeros(0)]), what + " s")
            assert_bit_equal(got[:, 1], np.concatenate([w[1] for w in want] + [np.zeros(0)]), what + " sdot")
    assert {0, 1, 255, 256, 511, 512, 513, 769, 1024, 1025} <= totals
    # no forward sweep has run: the forward curves are empty
    assert raw_pack(b, +1, 0, B, buf.ptr, buf.points) == (0, 0)
    b.close()


# ---------------------------------------------------------------------------------------------
# d. batotp_amd.dist on device memory, one rank, no process group
# ---------------------------------------------------------------------------------------------
def _cuts():
    g, s = helpers.Case("GEN7DOF"), helpers.Case("synth_gen7dof_s0")
    return [helpers.PrefixCase(c, n, g.problem) for c, n in ((g, 4), (s, 37), (g, g.n), (s, 4), (g, 120), (s, s.n), (g, 29), (s, 700))]


def _single_rank_child(q):
    """a fresh process in the product's order (torch, then the library): batotp_amd.dist on device tensors without a process group"""
    try:
        import torch
        from batotp_amd import dist as bdist
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        ctx = capi.Context(capi.load_hip(), 0)
        b = make_batch(ctx, _cuts())
        b.optimize()
        out = {}
        for w in (-1, +1):
            curves = bdist.gather_curves(b, w, device=dev)
            bufs, counts = bdist.gather_curves(b, w, device=dev, on_device=True)
            out[w] = {"host": [(s.tobytes(), sd.tobytes()) for s, sd in curves],
                      "n_bufs": len(bufs), "n_counts": len(counts), "is_cuda": bool(bufs[0].is_cuda), "dtype": str(bufs[0].dtype),
                      "shape": tuple(bufs[0].shape), "counts": [int(v) for v in counts[0]], "packed": bufs[0].cpu().numpy().tobytes()}
        rows = b.results()
        same = bdist.gather_results(rows, dev)
        out["rows"] = (rows.tobytes(), same.tobytes(), same is rows, str(same.dtype) == str(capi.RESULT_DTYPE))
        b.close(); ctx.close()
        q.put(("ok", out))
    except BaseException:
        q.put(("failed", traceback.format_exc()))


def test_dist_on_device_memory_single_rank(oracle_ctx):
    """gather_curves(batch, w, device=cuda:0) returns the oracle's curves; with on_device=True one (points, 2) CUDA tensor plus the
    counts with the same content; gather_results(rows, cuda:0) returns the rows unchanged.  In a child process: see the top of the file."""
    import multiprocessing as mp
    cuts, ref = ragged(oracle_ctx)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_single_rank_child, args=(q,))
    p.start()
    try:
        status, out = q.get(timeout=120)
        p.join(timeout=60)
    finally:
        if p.is_alive():
            p.terminate()
    assert status == "ok", out
    assert p.exitcode == 0
    for w, key, cnt in ((-1, "rev", "n_rev"), (+1, "fwd", "n_fwd")):
        o = out[w]
        assert len(o["host"]) == len(cuts)
        for k, (s, sd) in enumerate(o["host"]):
            assert_bit_equal(np.frombuffer(s), ref[k][key][0], f"gather_curves {w} path {k} s")
            assert_bit_equal(np.frombuffer(sd), ref[k][key][1], f"gather_curves {w} path {k} sdot")
        want_counts = [int(r["result"][cnt]) for r in ref]
        assert o["n_bufs"] == 1 and o["n_counts"] == 1 and o["is_cuda"] and o["dtype"] == "torch.float64"
        assert o["counts"] == want_counts and o["shape"] == (sum(want_counts), 2)
        packed = np.frombuffer(o["packed"]).reshape(-1, 2)
        assert_bit_equal(packed[:, 0], np.concatenate([r[key][0] for r in ref]), f"gather_curves {w} on the device, s")
        assert_bit_equal(packed[:, 1], np.concatenate([r[key][1] for r in ref]), f"gather_curves {w} on the device, sdot")
    rows, same, is_same_object, same_dtype = out["rows"]
    assert same == rows and not is_same_object and same_dtype
    assert rows == np.array([r["result"] for r in ref], dtype=capi.RESULT_DTYPE).tobytes()


# ---------------------------------------------------------------------------------------------
# e. two ranks over RCCL
# ---------------------------------------------------------------------------------------------
def test_two_ranks_over_rccl_match_the_single_rank_run(hip_lib, oracle_ctx):
    """5 paths as 3 + 2, then 1 path as 1 + 0 (rank 1 has no batch), one process per GPU: rows by all_gather, both curves of every
    path by the size exchange + grouped send / recv of gather_curves on device memory, equal to the oracle's single-rank run"""
    n_dev = hip_lib.device_count()
    if n_dev < 2:
        pytest.skip(f"the two-rank gather over RCCL needs 2 devices, this machine shows {n_dev}")
    import multiprocessing as mp
    ctx = mp.get_context("spawn")      # fresh child processes: nothing of this process's GPU state is inherited
    pool = ["GEN7DOF", "synth_gen7dof_s0"]
    for names in ([pool[k % 2] for k in range(5)], pool[:1]):
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, names, q, "nccl", capi.load_hip, "cuda")) for r in range(2)]
        for p in procs:
            p.start()
        try:
            raw, curves = q.get(timeout=120)
            for p in procs:
                p.join(timeout=60)
            codes = [p.exitcode for p in procs]
        except Exception:
            codes = None
        finally:
            for p in procs:
                if p.is_alive():
                    p.terminate()
        assert codes == [0, 0], f"{len(names)} paths on two ranks: the ranks did not finish in time or failed (exit codes {codes})"
        gathered = np.frombuffer(raw, dtype=capi.RESULT_DTYPE)
        cases = [helpers.Case(n) for n in names]
        for c in cases:
            c.problem = cases[0].problem
        single = helpers.run_pipeline(oracle_ctx, cases, mvc=False, details=False)
        assert gathered.shape[0] == len(names)
        for k, o in enumerate(single):
            for f in capi.RESULT_DTYPE.names:
                assert gathered[k][f] == o["result"][f], (len(names), k, f)
        for w, key in ((-1, "rev"), (1, "fwd")):
            assert len(curves[w]) == len(names)
            for k, o in enumerate(single):
                assert curves[w][k][0] == o[key][0].tobytes() and curves[w][k][1] == o[key][1].tobytes(), (len(names), w, k)
