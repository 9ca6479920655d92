"""Restatement of the chain tool point of include/batotp_hip_kin.h in plain Python floats.

Every operation is one binary64 operation in the order of the header; the trigonometry is ``math.cos`` / ``math.sin`` --
the C library's functions, called separately.  (numpy's vectorised trig is not libm's, so nothing here is vectorised.)
The built-in tables restate include/batotp_models.h; the CPU tests compare them with the library's through the driver.
"""
from __future__ import annotations

import math

import numpy as np

DEG2RAD = 3.14159265358979323846 / 180.0


class Chain:
    def __init__(self, axis, off, tool, degrees):
        self.axis = [[float(v) for v in a] for a in axis]
        self.off = [[float(v) for v in o] for o in off]
        self.tool = [float(v) for v in tool]
        self.degrees = bool(degrees)
        assert len(self.axis) == len(self.off) and 1 <= len(self.axis) <= 8

    @property
    def n_links(self):
        return len(self.axis)


_KUKA_AXES = [(0, 0, 1), (0, -1, 0), (0, 0, 1), (0, 1, 0), (0, 0, 1), (0, -1, 0), (0, 0, 1)]
_KUKA_OFFS = [(0, 0, 0), (0, 0, 0.3105), (0, 0, 0.2), (0, 0, 0.2), (0, 0, 0.2), (0, 0, 0.19), (0, 0, 0)]


def builtin(name: str) -> Chain:
    if name == "KUKA":
        return Chain(_KUKA_AXES, _KUKA_OFFS, (0, -.08, .545), True)
    if name == "RR":
        return Chain([(0, 0, 1), (0, 0, 1)], [(0, 0, 0), (0.4, 0, 0)], (.6, 0, 0), True)
    if name == "UR":
        return Chain([(0, 0, 1), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, 0, -1), (0, -1, 0)],
                     [(0, 0, 0), (0, 0, .089159), (-.425, 0, 0), (-.39225, 0, 0), (0, -.10915, 0), (0, 0, -.09465)],
                     (0, -.0823, 0), True)
    raise KeyError(name)


def tool_point(chain: Chain, theta) -> tuple:
    """theta: n_links joint values of one point -> (x, y, z)"""
    unit = DEG2RAD if chain.degrees else 1.0
    p0, p1, p2 = chain.tool
    for i in range(chain.n_links - 1, -1, -1):
        q = unit * float(theta[i])
        c = math.cos(q)
        s = math.sin(q)
        a0, a1, a2 = chain.axis[i]
        d = (a0 * p0 + a1 * p1) + a2 * p2
        x0 = a1 * p2 - a2 * p1
        x1 = a2 * p0 - a0 * p2
        x2 = a0 * p1 - a1 * p0
        k = d * (1.0 - c)
        o = chain.off[i]
        n0 = o[0] + ((p0 * c + x0 * s) + a0 * k)
        n1 = o[1] + ((p1 * c + x1 * s) + a1 * k)
        n2 = o[2] + ((p2 * c + x2 * s) + a2 * k)
        p0, p1, p2 = n0, n1, n2
    return p0, p1, p2


def tool_points(chain: Chain, theta: np.ndarray) -> np.ndarray:
    """theta [n_links][n] -> [3][n]"""
    theta = np.asarray(theta, dtype=np.float64)
    assert theta.shape[0] == chain.n_links
    out = np.empty((3, theta.shape[1]), dtype=np.float64)
    for i in range(theta.shape[1]):
        out[:, i] = tool_point(chain, theta[:, i])
    return out


def random_chain(rng: np.random.Generator, n_links: int, degrees: bool) -> Chain:
    """axes normalised so that | |a|^2 - 1 | is a few ulps, offsets and tool point of arm-like size"""
    axis = []
    for _ in range(n_links):
        a = rng.normal(size=3)
        a = a / math.sqrt(float(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))
        axis.append(a)
    return Chain(axis, rng.uniform(-0.5, 0.5, size=(n_links, 3)), rng.uniform(-0.3, 0.3, size=3), degrees)


def edge_angles(rng: np.random.Generator, n_links: int, n: int, degrees: bool) -> np.ndarray:
    """[n_links][n] joint values over +-400 degrees with exact 0 and +-90 (in the chain's unit) among them"""
    th = rng.uniform(-400.0, 400.0, size=(n_links, n))
    special = np.array([0.0, 90.0, -90.0])
    for j in range(n_links):
        for k, v in enumerate(special):
            if n > 0:
                th[j, (j + 3 * k) % n] = v
    return th if degrees else th * DEG2RAD
