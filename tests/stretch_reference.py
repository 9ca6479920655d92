"""The definition of the time stretch of finished trajectories (include/batotp_hip_stretch.h) in whole-array numpy operations, in
the stated order, and the rounds of its audit mode driven by tests/audit_reference.py.

binary64 throughout; the ratio rk is formed once with a plain `/`, every other step is one numpy element-wise operation -- the
IEEE ones, never contracted -- so the device has to reproduce these bits.  Values that are not finite propagate through the
stencils that read them; the payload and the sign of a NaN are not part of the definition (assert_rows_equal)."""
import math

import numpy as np

from audit_reference import audit_path
from batotp_amd import capi

MAX_POINTS = capi.STRETCH_MAX_POINTS


def n_out_by(n, factor):
    """the point count batotp_hip_output_stretch_by gives a path of n points"""
    if n < 2:
        return n
    return int(math.ceil(float(n - 1) * float(factor))) + 1


def stretch_rows(rows, n2):
    """one path: rows[R][n] -> [R][n2]"""
    x = np.ascontiguousarray(rows, dtype=np.float64)
    R, n = x.shape
    n2 = int(n2)
    assert n2 >= n and (n >= 2 or n2 == n)
    if n2 == n or n < 2:
        return x.copy()
    rk = np.float64(n - 1) / np.float64(n2 - 1)
    p = np.arange(n2 - 1, dtype=np.int64)
    u = p.astype(np.float64) * rk
    j = np.minimum(u.astype(np.int64), n - 2)
    f = u - j.astype(np.float64)
    y = np.empty((R, n2))
    with np.errstate(all="ignore"):
        x0, x1 = x[:, j], x[:, j + 1]
        d = x1 - x0
        m0 = np.where(j >= 1, (x1 - x[:, np.maximum(j - 1, 0)]) * 0.5, d)
        m1 = np.where(j + 2 <= n - 1, (x[:, np.minimum(j + 2, n - 1)] - x0) * 0.5, d)
        c2 = (3.0 * d - 2.0 * m0) - m1
        c3 = (m0 + m1) - 2.0 * d
        y[:, :-1] = x0 + f * (m0 + f * (c2 + f * c3))
    y[:, -1] = x[:, n - 1]
    return y


def stretch_to(rows_list, n_out):
    return [stretch_rows(r, n2) for r, n2 in zip(rows_list, n_out)]


def path_passes(rec, target):
    """(passes, need) of one audit record: JNT_VEL, JNT_ACC, CART_VEL, CART_ACC each <= target or -1; TRQ takes no part"""
    need, ok = 1.0, True
    for f in (capi.AUDIT_JNT_VEL, capi.AUDIT_CART_VEL):
        peak = float(rec["fam"][f]["peak"])
        if not peak <= target:
            ok, need = False, max(need, peak / target)
    for f in (capi.AUDIT_JNT_ACC, capi.AUDIT_CART_ACC):
        peak = float(rec["fam"][f]["peak"])
        if not peak <= target:
            ok, need = False, max(need, math.sqrt(peak / target))
    return ok, need


def stretch_audit(rows_list, sres, n_theta, n_cart, prob, target=1.0, max_rounds=8, max_factor=16.0, trace=None):
    """the rounds of batotp_hip_output_stretch_audit: (stretched rows of every path, report as capi.STRETCH_DTYPE, final audit).
    trace: a list that takes, per round, (the audit records the round read, n_out, rounds, status) of every path after it"""
    K = len(rows_list)
    sres = np.broadcast_to(np.asarray(sres, dtype=np.float64), (K,))
    src = [np.ascontiguousarray(r, dtype=np.float64) for r in rows_list]
    n_in = [r.shape[1] for r in src]
    n2, rounds, status, capped = list(n_in), [0] * K, [capi.STRETCH_PASSES] * K, [False] * K
    cur = [r.copy() for r in src]
    final = np.zeros(K, dtype=capi.AUDIT_DTYPE)
    stale = [True] * K              # (a path whose rows did not change keeps its record: the audit is a function of the rows)
    while True:
        again = False
        for k in range(K):
            if stale[k]:
                final[k] = audit_path(cur[k], sres[k], n_theta, n_cart, 0, prob, 0.0)
                stale[k] = False
            ok, need = path_passes(final[k], target)
            if ok:
                status[k] = capi.STRETCH_PASSES
                continue
            if capped[k]:
                status[k] = capi.STRETCH_CAPPED
                continue
            if rounds[k] >= max_rounds:
                status[k] = capi.STRETCH_ROUNDS
                continue
            m = n2[k] - 1
            want = float(m) * need
            intervals = max(want if math.isinf(want) else math.ceil(want), float(m + 1))
            bound = min(math.floor(float(n_in[k] - 1) * max_factor), float(MAX_POINTS - 1))
            if intervals > bound:
                intervals, capped[k], status[k] = bound, True, capi.STRETCH_CAPPED
            new = int(intervals) + 1
            if new == n2[k]:
                continue
            n2[k], rounds[k], again = new, rounds[k] + 1, True
            cur[k] = stretch_rows(src[k], new)      # always from the original rows
            stale[k] = True
        if trace is not None:
            trace.append((final.copy(), list(n2), list(rounds), list(status)))
        if not again:
            break
    report = np.zeros(K, dtype=capi.STRETCH_DTYPE)
    for k in range(K):
        report[k] = (n_in[k], n2[k], 1.0 if n_in[k] < 2 else float(n2[k] - 1) / float(n_in[k] - 1), rounds[k], status[k])
    return cur, report, final


def assert_rows_equal(got, want, what):
    """bit for bit as uint64 (the signs of zeros and of infinities count) wherever the expected value is no NaN; a NaN for a NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    g, w = got.view(np.uint64), want.view(np.uint64)
    bad = np.where(nan, ~np.isnan(got), g != w)
    if bad.any():
        r, i = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.size} values differ; first at row {r}, point {i}: got {float(got[r, i])!r} "
                             f"({int(g[r, i]):016x}), want {float(want[r, i])!r} ({int(w[r, i]):016x})")


def assert_report_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in range(got.shape[0]):
        for c in ("n_in", "n_out", "rounds", "status"):
            assert int(got[k][c]) == int(want[k][c]), f"{what}: path {k} {c}: got {int(got[k][c])}, want {int(want[k][c])}"
        assert got[k]["factor"].tobytes() == want[k]["factor"].tobytes(), f"{what}: path {k} factor"
    assert got.tobytes() == want.tobytes(), what
