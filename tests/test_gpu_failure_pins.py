"""GPU (-m gpu): the HIP kernels on the failure pins -- paths whose bisections fail by the thousand and paths that run into the
time limit (tests/golden/pin_*, pinned by the reference binary's log and float32 files; tests/test_oracle_failure_pins.py has
the checker's side).  Every device result is compared with the checker's, rows and curves bit for bit, AND with what the
reference pinned; one path at a time in every sweep layout, and whole families as one ragged batch, where a finishing path, a
path that fails at every stage and a path that gives up share a wavefront."""
import pytest

import helpers
from helpers import assert_bit_equal, assert_matches_pin, pin_case, run_pin_batch, set_layout
from batotp_amd import capi

pytestmark = pytest.mark.gpu

PAIRS = capi.F_NO_SAMPLES | capi.F_COMPACT_SPLINES

# joint velocity / acceleration limits only (families A, C, D): every lane layout of tests/test_gpu_fuzz.py, on coefficient rows and on
# compact pairs; the one-path-per-wavefront kernel, which compact batches of this kind take, with and without the fast-forward and with
# two paths per wavefront
VA_LAYOUTS = [0, 1, 2, 4, 8, 16, "flat0", "flat4", "g4flat0", "g4flat8", "g2flat3"]
VA_PLAN = [(lay, 0) for lay in VA_LAYOUTS] + [(lay, PAIRS) for lay in VA_LAYOUTS + [64, "64noff", "64x2"]]
# tension / torque limits (families B, E): the one-path-per-wavefront kernel (the general kernel where it does not apply: a parallel
# mechanism left parallel); the automatic plan and the 8-lane layout as the second half of the parametrisation
TRQ_PLAN = [(64, 0), ("64noff", 0), ("64x2", 0)]

_ORACLE = {}


def _oracle_single(oracle_ctx, name):
    """the checker's rows and curves of one pin as a one-path batch, computed once for all tests of this file"""
    if name not in _ORACLE:
        _ORACLE[name] = run_pin_batch(oracle_ctx, [pin_case(name)])[0]
    return _ORACLE[name]


def _plan(case):
    if not (case.problem.flags & capi.F_TRQ_ON):
        return VA_PLAN
    serial_cable = (case.problem.flags & capi.F_PARALLEL) and (case.problem.flags & capi.F_PAR2SER)
    # (the cable robot in serial form has every channel as pairs too; two paths per wavefront exist for that form only)
    return TRQ_PLAN + ([(64, PAIRS), ("64x2", PAIRS)] if serial_cable else [])


def _assert_same(case, got, want, what):
    for f in want["result"].dtype.names:
        assert got["result"][f] == want["result"][f], (what, f, got["result"], want["result"])
    for which in ("rev", "fwd"):
        assert (got[which] is None) == (want[which] is None), (what, which)
        if want[which] is not None:
            assert_bit_equal(got[which][0], want[which][0], f"{what}: {which} s")
            assert_bit_equal(got[which][1], want[which][1], f"{what}: {which} sdot")
    assert_matches_pin(case, got)


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("name", helpers.PIN_CASES)
def test_one_path_in_every_layout(hip_lib, oracle_ctx, name, compact):
    """rows (both failure counters, both status words, step counts, durations) and both curves equal the checker's bit for bit, and the
    device's own output passes the assertions against the reference's pin"""
    case = pin_case(name)
    want = _oracle_single(oracle_ctx, name)
    assert_matches_pin(case, want)
    plan = [(layout, extra) for layout, extra in _plan(case) if bool(extra) == bool(compact)]
    if compact and not plan:
        plan = [(0, 0), (8, 0)]      # no compact form of this problem kind (torque limits of a serial arm, a parallel mechanism left parallel)
    for layout, extra in plan:
        ctx = capi.Context(hip_lib, 0)
        set_layout(ctx, layout)
        got = run_pin_batch(ctx, [case], extra_flags=extra)[0]
        _assert_same(case, got, want, f"{name} layout {layout} flags {extra:#x}")
        ctx.close()


def _batch_plan(family):
    if family == "B":
        return [(64, 0), ("64x2", PAIRS), (0, 0), (8, 0)]
    # 8 lanes per path and 8 paths per wavefront (nested and flat loops), 4 and 2 lanes, two paths per wavefront of the one-path kernel
    return [(8, 0), ("flat0", 0), ("flat4", PAIRS), ("g4flat8", 0), ("g2flat3", PAIRS), (0, 0), (0, PAIRS), ("64x2", PAIRS)]


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("family", ["A", "B", "C"])
def test_family_as_one_ragged_batch(hip_lib, oracle_ctx, family, part):
    """the paths of a family that share a config.dat in ONE batch: an aborting path, a path with thousands of failed stages and a
    finishing path in one wavefront.  Every path's rows and curves equal its one-path run of the checker (to which the test above ties
    its one-path run on the device): nothing of a neighbour's abort or certificate reaches another lane group"""
    batches = helpers.pin_batches(family)
    assert max(len(b) for b in batches) >= 3
    for cases in batches:
        if len(cases) < 2:
            continue
        want = [_oracle_single(oracle_ctx, c.name) for c in cases]
        for layout, extra in _batch_plan(family)[part::2]:      # (the layouts in two halves: a few seconds per test)
            if extra and (cases[0].problem.flags & capi.F_TRQ_ON) and not (cases[0].problem.flags & capi.F_PAR2SER):
                continue    # (pairs for every channel exist for the serial form only)
            ctx = capi.Context(hip_lib, 0)
            set_layout(ctx, layout)
            got = run_pin_batch(ctx, cases, extra_flags=extra)
            for c, g, w in zip(cases, got, want):
                _assert_same(c, g, w, f"family {family} as a batch, {c.name}, layout {layout} flags {extra:#x}")
            ctx.close()


@pytest.mark.parametrize("order", [1, 0])
def test_family_a_tiled_three_times(hip_lib, oracle_ctx, order):
    """family A three times over (18 paths: more than the 8 lane groups of a wavefront), launched longest path first and in the
    order given"""
    cases = [c for b in helpers.pin_batches("A") for c in b] * 3
    want = [_oracle_single(oracle_ctx, c.name) for c in cases]
    for layout, extra in ((8, 0), ("flat4", PAIRS), ("g4flat0", 0), (0, PAIRS)):
        ctx = capi.Context(hip_lib, 0)
        set_layout(ctx, layout)
        ctx.set_path_order(order)
        got = run_pin_batch(ctx, cases, extra_flags=extra)
        for k, (c, g, w) in enumerate(zip(cases, got, want)):
            _assert_same(c, g, w, f"family A x 3, path order {order}, path {k} ({c.name}), layout {layout} flags {extra:#x}")
        ctx.close()


@pytest.mark.parametrize("compact", [0, 1])
def test_family_a_certificate_and_fast_forward_switches(hip_lib, oracle_ctx, compact):
    """the failure certificate and the certified fast-forward, off and at every hold tests/test_gpu_fuzz.py uses: k_sweep8 with the hold
    of the stage / of the reverse sweep's certificate phase (-1 automatic, 0 none), k_sweep1 with and without its fast-forward.  Same
    rows, same curves"""
    cases = [c for b in helpers.pin_batches("A") for c in b]
    want = [_oracle_single(oracle_ctx, c.name) for c in cases]
    extra = PAIRS if compact else 0

    def check(ctx, what):
        got = run_pin_batch(ctx, cases, extra_flags=extra)
        for c, g, w in zip(cases, got, want):
            _assert_same(c, g, w, f"family A, {what}, compact {compact}, {c.name}")
        ctx.close()

    for hold, cert in ((-1, -1), (0, -1), (2, -1), (3, -1), (4, -1), (5, -1), (6, -1), (8, -1), (4, 0), (4, 1), (4, 8), (6, 2), (8, 8), (0, 2)):
        ctx = capi.Context(hip_lib, 0)
        ctx.set_sweep_group(8); ctx.set_paths_per_wave(8); ctx.set_sweep_hold(hold, hold); ctx.set_cert_hold(cert)
        check(ctx, f"hold {hold} certificate hold {cert}")
    for ff in (True, False):
        ctx = capi.Context(hip_lib, 0)
        ctx.set_sweep_group(8); ctx.set_paths_per_wave(8); ctx.set_sweep_hold(4, 4); ctx.set_fast_forward(ff)
        check(ctx, f"8 lanes, fast-forward {ff}")
    for layout in (64, "64noff", "64x2"):
        ctx = capi.Context(hip_lib, 0)
        set_layout(ctx, layout)
        check(ctx, f"layout {layout}")
