"""The definition of the torque rows for finished trajectories (include/batotp_hip_invdyn.h) restated: numpy finite differences in
the audit's order, math.cos / math.sin per value (libm's; numpy's vectorised ones are not), the two passes of the recursion through
the oracle's exported bo_rnea (the CPU twin of rnea_pass, called as tests/test_oracle_dyn.py::_rnea does), and the sum in the
stated order.  binary64 throughout; numpy's element-wise operations and Python's float arithmetic are the IEEE ones."""
import ctypes as C
import math

import numpy as np

D = C.POINTER(C.c_double)
DEG2RAD = 3.14159265358979323846 / 180.0


def differences(x, h):
    """(v, a)[n_links][n] of joint rows x[n_links][n]: central differences at ic = min(max(i, 1), n - 2), +0.0 for n < 3"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    v, a = np.zeros_like(x), np.zeros_like(x)
    if n < 3:
        return v, a
    h = np.float64(h)
    c1 = np.float64(1.0) / (np.float64(2.0) * h)
    c2 = np.float64(1.0) / (h * h)
    with np.errstate(all="ignore"):
        xm, x0, xp = x[:, :-2], x[:, 1:-1], x[:, 2:]
        vi = (xp - xm) * c1
        ai = ((xp - x0) - (x0 - xm)) * c2
    ic = np.clip(np.arange(n), 1, n - 2) - 1
    return vi[:, ic], ai[:, ic]


def _rnea(lib, model, cq, sq, qd, qdd, a0):
    tau = np.zeros(model.n_links)
    lib.lib.bo_rnea.restype = None
    lib.lib.bo_rnea(C.byref(model), cq.ctypes.data_as(D), sq.ctypes.data_as(D), qd.ctypes.data_as(D), qdd.ctypes.data_as(D),
                    a0.ctypes.data_as(D), tau.ctypes.data_as(D))
    return tau


def torque_point(oracle_lib, model, q, qd, qdd):
    """tau[n_links] of one configuration: (t2 + fv * qd) + t4"""
    nl = model.n_links
    cq = np.array([math.cos(float(v)) for v in q])
    sq = np.array([math.sin(float(v)) for v in q])
    qd, qdd = np.ascontiguousarray(qd, dtype=np.float64), np.ascontiguousarray(qdd, dtype=np.float64)
    z, zero3 = np.zeros(nl), np.zeros(3)
    g0 = np.array([-model.gravity[0], -model.gravity[1], -model.gravity[2]])
    t2 = _rnea(oracle_lib, model, cq, sq, qd, qdd, zero3)
    t4 = _rnea(oracle_lib, model, cq, sq, z, z, g0)
    fv = np.array([model.link[j].fv for j in range(nl)])
    with np.errstate(all="ignore"):
        return (t2 + fv * qd) + t4


def torque_rows(oracle_lib, model, x, h):
    """torque rows [n_links][n] of one path with joint rows x[n_links][n] and time step h"""
    x = np.asarray(x, dtype=np.float64)
    nl, n = model.n_links, x.shape[1]
    assert x.shape[0] == nl
    unit = np.float64(DEG2RAD if model.degrees else 1.0)
    v, a = differences(x, h)
    with np.errstate(all="ignore"):
        q, qd, qdd = unit * x, unit * v, unit * a
    out = np.empty((nl, n))
    for i in range(n):
        out[:, i] = torque_point(oracle_lib, model, q[:, i], qd[:, i], qdd[:, i])
    return out


def with_torques(oracle_lib, model, rows_list, sres, n_cart=0):
    """every path of a batch: rows [n_links + n_cart][n] -> [n_links + n_cart + n_links][n]"""
    sres = np.broadcast_to(np.asarray(sres, dtype=np.float64), (len(rows_list),))
    nl = model.n_links
    return [np.concatenate([np.asarray(r, dtype=np.float64), torque_rows(oracle_lib, model, np.asarray(r)[:nl], sres[k])])
            for k, r in enumerate(rows_list)]


def assert_rows_bit_equal(got, want, what):
    """as uint64: NaN payloads and the signs of zeros count"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint64), want.view(np.uint64)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        r, i = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ; first at row {r}, point {i}: got {float(got[r, i])!r} "
                             f"({int(g[r, i]):016x}), want {float(want[r, i])!r} ({int(w[r, i]):016x})")
