"""The definition of the continuous torque rating of finished trajectories (include/batotp_hip_duty.h) restated in numpy, driven by
the pieces that are already pinned: the three addends of tests/tscale_reference.py (the oracle's exported bo_rnea), the cubic of
tests/stretch_reference.py and the audit of tests/audit_reference.py.

binary64 throughout; numpy's element-wise `*`, `+`, `/` and sqrt are the IEEE ones, every step is one operation in the stated order.
The sum is part of the definition: blocks of BP points, in a wavefront of 64 values the upper half is added to the lower half six
times, block = wave 0 + wave 1, path = the blocks one after another."""
import math

import numpy as np

import invdyn_reference as ir
import stretch_reference as sr
import tscale_reference as tr
from audit_reference import audit_path
from batotp_amd import capi

BP = capi.DUTY_BLOCK_POINTS
ML = capi.MAX_LINKS


def tree_sum(v):
    """the path sum of the values v[..., n] along the last axis, in the order of the definition"""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1]
    if n == 0:
        return np.zeros(v.shape[:-1])
    nb = -(-n // BP)
    pad = np.zeros(v.shape[:-1] + (nb * BP,))          # lanes past the end of the path contribute +0.0
    pad[..., :n] = v
    w = pad.reshape(v.shape[:-1] + (nb, BP // 64, 64))
    with np.errstate(all="ignore"):
        d = 32
        while d >= 1:
            w = w[..., :d] + w[..., d:2 * d]
            d //= 2
        blocks = w[..., 0, 0] + w[..., 1, 0]
        s = blocks[..., 0].copy()
        for b in range(1, nb):
            s = s + blocks[..., b]
    return s


def pieces(oracle_lib, model, x, h):
    """tscale_reference.pieces, also for rows that hold an Inf: the sine and cosine of an infinite angle are NaN (IEEE; math.cos raises)"""
    x = np.asarray(x, dtype=np.float64)
    if not np.isinf(x).any():
        return tr.pieces(oracle_lib, model, x, h)
    nl, n = model.n_links, x.shape[1]
    unit = np.float64(ir.DEG2RAD if model.degrees else 1.0)
    v, a = ir.differences(x, h)
    with np.errstate(all="ignore"):
        q, qd, qdd = unit * x, unit * v, unit * a
    fv = np.array([model.link[j].fv for j in range(nl)])
    z, zero3 = np.zeros(nl), np.zeros(3)
    g0 = np.array([-model.gravity[0], -model.gravity[1], -model.gravity[2]])
    A, G = np.empty((nl, n)), np.empty((nl, n))
    for i in range(n):
        cq = np.array([math.cos(float(u)) if math.isfinite(u) else math.nan for u in q[:, i]])
        sq = np.array([math.sin(float(u)) if math.isfinite(u) else math.nan for u in q[:, i]])
        A[:, i] = ir._rnea(oracle_lib, model, cq, sq, np.ascontiguousarray(qd[:, i]), np.ascontiguousarray(qdd[:, i]), zero3)
        G[:, i] = ir._rnea(oracle_lib, model, cq, sq, z, z, g0)
    with np.errstate(all="ignore"):
        B = fv[:, None] * qd
    return A, B, G


def point_values(oracle_lib, model, x, h, abg=None):
    """(moments[n_links][7][n], power[n], torque rows[n_links][n]) of one path with joint rows x[n_links][n] and time step h; abg: its
    (A, B, G) of tscale_reference.pieces where the caller has them"""
    x = np.asarray(x, dtype=np.float64)
    nl, n = model.n_links, x.shape[1]
    A, B, G = abg if abg is not None else pieces(oracle_lib, model, x, h)
    unit = np.float64(ir.DEG2RAD if model.degrees else 1.0)
    v, a = ir.differences(x, h)
    with np.errstate(all="ignore"):
        qd = unit * v
        tau = (A + B) + G
        m = np.stack([A * A, A * B, B * B, A * G, B * G, G * G, tau * tau], axis=1)
        p = tau[0] * qd[0] if n else np.zeros(0)
        for j in range(1, nl):
            p = p + tau[j] * qd[j]
    return m, p, tau


def sums_record(m, p):
    """one capi.DUTY_SUMS_DTYPE record from the point values of a path"""
    rec = np.zeros((), dtype=capi.DUTY_SUMS_DTYPE)
    nl, _, n = m.shape
    rec["n_pts"] = n
    rec["S"][:nl] = tree_sum(m)
    with np.errstate(all="ignore"):
        rec["W"] = tree_sum(np.where(p > 0.0, p, 0.0))
    ok = ~np.isnan(p)
    if ok.any():
        top = p[ok].max()
        rec["peak_power"], rec["power_at"] = top, int(np.flatnonzero(ok & (p == top))[0])
    else:
        rec["peak_power"], rec["power_at"] = -np.inf, -1
    return rec


def quartic(c, x):
    c4, c3, c2, c1, c0 = c
    return (((c4 * x + c3) * x + c2) * x + c1) * x + c0


def coefficients(S):
    """(c4, c3, c2, c1, c0) from the seven sums of a joint"""
    S = [np.float64(v) for v in S]
    with np.errstate(all="ignore"):
        return S[0], np.float64(2.0) * S[1], S[2] + np.float64(2.0) * S[3], np.float64(2.0) * S[4], S[5]


def bisect(c, L):
    """exactly 64 passes"""
    lo, hi = np.float64(0.0), np.float64(1.0)
    with np.errstate(all="ignore"):
        for _ in range(64):
            mid = np.float64(0.5) * (lo + hi)
            if quartic(c, mid) <= L:
                lo = mid
            else:
                hi = mid
    return lo


def duty_record(sums, nl, rated, target, h):
    """the host rule: one capi.DUTY_DTYPE record from the sums of a path"""
    d = np.zeros((), dtype=capi.DUTY_DTYPE)
    n = int(sums["n_pts"])
    d["util"], d["row"], d["s"], d["s_row"] = -1.0, -1, np.inf, -1
    nf = np.float64(n)
    t = np.float64(target)
    with np.errstate(all="ignore"):
        for j in range(nl if n > 0 else 0):
            r = np.float64(rated[j])
            rr, lim = np.float64(1.0) / r, t * r
            S = sums["S"][j]
            rms = np.sqrt(S[6] / nf)
            d["rms"][j] = rms
            u = rms * rr
            if np.isfinite(u) and u > d["util"]:
                d["util"], d["row"] = u, j
            L = (lim * lim) * nf
            c = coefficients(S)
            if not c[4] < L:
                d["n_hold"] += 1
                continue
            if quartic(c, np.float64(1.0)) <= L:
                continue
            lo = bisect(c, L)
            if lo < d["s"]:
                d["s"], d["s_row"] = lo, j
        d["energy"] = np.float64(h) * sums["W"]
    d["peak_power"], d["power_at"], d["n_pts"] = sums["peak_power"], sums["power_at"], n
    return d


def path_duty(oracle_lib, model, rows, h, abg=None):
    """(rows with n_links torque rows appended, sums record) of one path rows[n_links + n_cart][n]"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    m, p, tau = point_values(oracle_lib, model, rows[:model.n_links], h, abg)
    return np.concatenate([rows, tau]), sums_record(m, p)


def duty(oracle_lib, model, rows_list, sres, rated, target=1.0):
    """batotp_hip_output_duty: (rows with torques of every path, capi.DUTY_DTYPE records, capi.DUTY_SUMS_DTYPE records)"""
    K = len(rows_list)
    sres = np.broadcast_to(np.asarray(sres, dtype=np.float64), (K,))
    out, rec, raw = [], np.zeros(K, dtype=capi.DUTY_DTYPE), np.zeros(K, dtype=capi.DUTY_SUMS_DTYPE)
    for k, r in enumerate(rows_list):
        w, raw[k] = path_duty(oracle_lib, model, r, sres[k])
        rec[k] = duty_record(raw[k], model.n_links, rated, target, sres[k])
        out.append(w)
    return out, rec, raw


def stretch_duty(oracle_lib, model, rows_list, sres, n_cart, prob, rated, target=1.0, max_rounds=8, max_factor=16.0, cache=None, trace=None):
    """the rounds of batotp_hip_output_stretch_duty: tscale_reference.stretch_torques with the RMS family on top.
    (rows with torques of every path, report as capi.STRETCH_DTYPE, final audit, scale records, duty records).
    cache: a dict shared by calls on the SAME rows, model, limits, ratings and target.  trace: a list that takes, per round, (the
    audit, scale and duty records the round read, n_out, rounds, status) of every path after it"""
    K = len(rows_list)
    nl = model.n_links
    sres = np.broadcast_to(np.asarray(sres, dtype=np.float64), (K,))
    src = [np.ascontiguousarray(r, dtype=np.float64) for r in rows_list]
    n_in = [r.shape[1] for r in src]
    hi, lo = tr.bounds(prob, nl, target)
    probT = tr.with_trq_on(prob)
    cache = {} if cache is None else cache

    def evaluate(k, n2):
        if (k, n2) not in cache:
            rows = sr.stretch_rows(src[k], n2)
            A, B, G = tr.pieces(oracle_lib, model, rows[:nl], sres[k])
            w, sums = path_duty(oracle_lib, model, rows, sres[k], (A, B, G))
            cache[(k, n2)] = (w, tr.scale_record(A, B, G, hi, lo), audit_path(w, sres[k], nl, n_cart, nl, probT, 0.0),
                              duty_record(sums, nl, rated, target, sres[k]))
        return cache[(k, n2)]

    n2, rounds, status, capped = list(n_in), [0] * K, [capi.STRETCH_PASSES] * K, [False] * K
    while True:
        again = False
        read = [evaluate(k, n2[k])[1:] for k in range(K)]
        for k in range(K):
            rec, aud, dut = read[k]
            kin_ok, need = sr.path_passes(aud, target)
            ok = kin_ok
            trq_ok = float(aud["fam"][capi.AUDIT_TRQ]["peak"]) <= target
            if not trq_ok:
                ok = False
                if int(rec["n_static"]) == 0 and float(rec["s"]) < 1.0:
                    need = max(need, 1.0 / float(rec["s"]))
            util = float(dut["util"])
            rms_ok = util <= target or util == -1.0
            if not rms_ok:
                ok = False
                if int(dut["n_hold"]) == 0 and float(dut["s"]) < 1.0:
                    need = max(need, 1.0 / float(dut["s"]))
            if ok:
                status[k] = capi.STRETCH_PASSES
                continue
            if kin_ok and ((not trq_ok and int(rec["n_static"]) > 0) or (not rms_ok and int(dut["n_hold"]) > 0)):
                status[k] = capi.STRETCH_STATIC
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
            bound = min(math.floor(float(n_in[k] - 1) * max_factor), float(sr.MAX_POINTS - 1))
            if intervals > bound:
                intervals, capped[k], status[k] = bound, True, capi.STRETCH_CAPPED
            new = int(intervals) + 1
            if new == n2[k]:
                continue
            n2[k], rounds[k], again = new, rounds[k] + 1, True
        if trace is not None:
            trace.append(([a for r, a, d in read], [r for r, a, d in read], [d for r, a, d in read], list(n2), list(rounds), list(status)))
        if not again:
            break
    report = np.zeros(K, dtype=capi.STRETCH_DTYPE)
    final = np.zeros(K, dtype=capi.AUDIT_DTYPE)
    recs = np.zeros(K, dtype=capi.TSCALE_DTYPE)
    duties = np.zeros(K, dtype=capi.DUTY_DTYPE)
    out = []
    for k in range(K):
        report[k] = (n_in[k], n2[k], 1.0 if n_in[k] < 2 else float(n2[k] - 1) / float(n_in[k] - 1), rounds[k], status[k])
        w, recs[k], final[k], duties[k] = evaluate(k, n2[k])
        out.append(w)
    return out, report, final, recs, duties


def assert_sums_equal(got, want, what):
    """bit for bit where the reference is a number, NaN where it is NaN (which of two NaN operands an addition hands on is not pinned)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in range(got.shape[0]):
        for c in ("S", "W", "peak_power"):
            g, w = np.atleast_1d(got[k][c]).ravel(), np.atleast_1d(want[k][c]).ravel()
            nan = np.isnan(w)
            assert (np.isnan(g) == nan).all() and g[~nan].tobytes() == w[~nan].tobytes(), f"{what}: path {k} {c}: got {g.tolist()}, want {w.tolist()}"
        for c in ("power_at", "n_pts"):
            assert int(got[k][c]) == int(want[k][c]), f"{what}: path {k} {c}: got {int(got[k][c])}, want {int(want[k][c])}"


def assert_duty_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in range(got.shape[0]):
        for c in ("rms", "util", "s", "energy", "peak_power"):
            g, w = np.atleast_1d(got[k][c]).ravel(), np.atleast_1d(want[k][c]).ravel()
            nan = np.isnan(w)
            assert (np.isnan(g) == nan).all() and g[~nan].tobytes() == w[~nan].tobytes(), f"{what}: path {k} {c}: got {g.tolist()}, want {w.tolist()}"
        for c in ("row", "n_hold", "s_row", "reserved", "power_at", "n_pts"):
            assert int(got[k][c]) == int(want[k][c]), f"{what}: path {k} {c}: got {int(got[k][c])}, want {int(want[k][c])}"
