"""The definition of the trajectory audit (include/batotp_hip_audit.h) in whole-array numpy operations, in the stated order.

binary64 throughout; every reciprocal is formed once with a plain `/`, the per-point arithmetic only subtracts, multiplies, takes
fabs and sqrt and compares -- numpy's element-wise operations are the IEEE ones, so the device has to reproduce these bits.
The argmax follows the tie rule of the definition (lowest point, then lowest row) explicitly; nothing here relies on which index a
library routine happens to return."""
import numpy as np

from batotp_amd import capi

FAMILIES = capi.AUDIT_FAMILIES


def audited_families(prob, n_theta, n_cart, n_trq):
    f = prob.flags
    return [n_theta > 0,
            n_theta > 0 and bool(f & capi.F_JNT_ACC_ON),
            n_cart > 0 and bool(f & capi.F_CART_VEL_ON),
            n_cart > 0 and bool(f & capi.F_CART_ACC_ON),
            n_trq > 0 and bool(f & capi.F_TRQ_ON)]


def peak_of(U, pts):
    """(peak, at, row) of the utilisations U[row][k] at the points pts[k]: the largest finite value; ties: lowest point, then lowest row"""
    fin = np.isfinite(U)
    if U.size == 0 or not fin.any():
        return -1.0, -1, -1
    m = U[fin].max()
    hit = fin & (U == m)
    c = int(np.flatnonzero(hit.any(axis=0))[0])
    r = int(np.flatnonzero(hit[:, c])[0])
    return float(m), int(pts[c]), r


def audit_path(rows, h, n_theta, n_cart, n_trq, prob, tol):
    """one path: rows[n_theta + n_cart + n_trq][n]; returns one capi.AUDIT_DTYPE record"""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[1]
    out = np.zeros((), dtype=capi.AUDIT_DTYPE)
    out["fam"]["peak"], out["fam"]["at"], out["fam"]["row"] = -1.0, -1, -1
    out["n_pts"] = n
    if n == 0:
        return out
    on = audited_families(prob, n_theta, n_cart, n_trq)
    lim = np.float64(1.0) + np.float64(tol)
    over = np.zeros(n, dtype=bool)
    out["n_nonfinite"] = int(np.count_nonzero(~np.isfinite(rows)))
    peaks = {}

    def count(U, pts):
        with np.errstate(invalid="ignore"):
            hot = np.isfinite(U) & (U > lim)
        over[pts[hot.any(axis=0)]] = True

    with np.errstate(all="ignore"):
        if n >= 3:
            h = np.float64(h)
            c1 = np.float64(1.0) / (np.float64(2.0) * h)
            c2 = np.float64(1.0) / (h * h)
            pts = np.arange(1, n - 1)
            x = rows[: n_theta + min(3, n_cart)]
            xm, x0, xp = x[:, :-2], x[:, 1:-1], x[:, 2:]
            v = (xp - xm) * c1
            a = ((xp - x0) - (x0 - xm)) * c2
            if on[0]:
                rv = np.array([np.float64(1.0) / np.float64(prob.jnt_vel_max[j]) for j in range(n_theta)])
                U = np.fabs(v[:n_theta]) * rv[:, None]
                peaks[0] = peak_of(U, pts); count(U, pts)
            if on[1]:
                ra = np.array([np.float64(1.0) / np.float64(prob.jnt_acc_max[j]) for j in range(n_theta)])
                U = np.fabs(a[:n_theta]) * ra[:, None]
                peaks[1] = peak_of(U, pts); count(U, pts)
            for fam, d, limit in ((2, v, prob.cart_vel_max), (3, a, prob.cart_acc_max)):
                if not on[fam]:
                    continue
                r = np.float64(1.0) / np.float64(limit)
                c = d[n_theta:]
                s = c[0] * c[0]
                for k in range(1, c.shape[0]):      # (vx*vx + vy*vy) + vz*vz
                    s = s + c[k] * c[k]
                U = (np.sqrt(s) * r)[None, :]
                peaks[fam] = peak_of(U, pts); count(U, pts)
        if on[4]:
            t = rows[n_theta + n_cart:]
            tmax = np.array([np.float64(prob.jnt_trq_max[r]) for r in range(n_trq)])
            tmin = np.array([np.float64(prob.jnt_trq_min[r]) for r in range(n_trq)])
            mid = (tmax + tmin) * 0.5
            half = (tmax - tmin) * 0.5
            rt = np.float64(1.0) / half
            U = np.fabs(t - mid[:, None]) * rt[:, None]
            pts = np.arange(n)
            peaks[4] = peak_of(U, pts); count(U, pts)
    for fam, (p, at, row) in peaks.items():
        out["fam"]["peak"][fam], out["fam"]["at"][fam], out["fam"]["row"][fam] = p, at, row
    out["n_over"] = int(np.count_nonzero(over))
    return out


def audit_reference(rows_list, sres, n_theta, n_cart, n_trq, prob, tol=0.0):
    """every path of a batch: capi.AUDIT_DTYPE array"""
    sres = np.broadcast_to(np.asarray(sres, dtype=np.float64), (len(rows_list),))
    out = np.zeros(len(rows_list), dtype=capi.AUDIT_DTYPE)
    for k, rows in enumerate(rows_list):
        out[k] = audit_path(rows, sres[k], n_theta, n_cart, n_trq, prob, tol)
    return out


def assert_audit_equal(got, want, what=""):
    """bit equality of two audit tables, with the first difference named"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in range(got.shape[0]):
        for f, name in enumerate(FAMILIES):
            g, w = got[k]["fam"][f], want[k]["fam"][f]
            assert g["peak"].tobytes() == w["peak"].tobytes() and int(g["at"]) == int(w["at"]) and int(g["row"]) == int(w["row"]), \
                f"{what}: path {k} {name}: got ({float(g['peak'])!r}, {int(g['at'])}, {int(g['row'])}), want ({float(w['peak'])!r}, {int(w['at'])}, {int(w['row'])})"
        for c in ("n_pts", "n_over", "n_nonfinite"):
            assert int(got[k][c]) == int(w_ := want[k][c]), f"{what}: path {k} {c}: got {int(got[k][c])}, want {int(w_)}"
    assert got.tobytes() == want.tobytes(), what
