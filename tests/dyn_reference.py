"""The dynamics coefficients of a serial chain (include/batotp_hip.h: batotp_serial_model), restated at high precision.

    tau = a1 sddot + a2 sdot^2 + a3 sdot + a4          along a path q(s), q' = dq/ds, q'' = d2q/ds2

is what Lagrange's equations  d/dt (dT/dqdot) - dT/dq + dU/dq + fv .* qdot = tau  give for qdot = q' sdot,
qddot = q' sddot + q'' sdot^2:

    a1 = M(q) q'
    a2 = M(q) q'' + Mdot q' - dT/dq          T = 1/2 q'^T M(q) q',  Mdot = d/ds M(q(s)),  no gravity
    a3 = fv .* q'
    a4 = dU/dq                               U = - sum_i m_i g . c_i(q)

Nothing here is a recursion over forces: the chain's KINEMATICS are written down (frames by Rodrigues rotations), the mass matrix
is the Hessian of the kinetic energy in the joint rates (through the Jacobians of the centres of mass and the angular velocities),
the gravity torques are the gradient of the potential energy (through the same Jacobians), and the velocity-dependent part of a2
is differentiated numerically -- central differences with a step of 10^-(dps/3) in `mp.dps`-digit arithmetic, whose error (~h^2
and ~10^-dps / h) lies some fifteen orders of magnitude under a double's rounding.

What the header fixes and this file restates:
  * every link frame coincides with the base frame at q = 0; joint i turns link i about `axis`, a unit vector that is the same in
    link and in parent coordinates (the stored doubles are normalised here: the definition says unit vector);
  * `off`: joint origin relative to the parent's joint origin, parent coordinates; `com`: relative to the joint origin, link
    coordinates; `inertia`: about the centre of mass, link coordinates, ordered (xx, yy, zz, xy, xz, yz);
  * `gravity` is the gravitational ACCELERATION in base coordinates ((0, 0, -9.81) pulls down): U = - m g . c;
  * `degrees`: joint values (and their path derivatives) are degrees and are scaled by pi / 180 first: the generalised
    coordinates, and therefore the torques, are those of the angles in radians.

Also here: the chain models the tests of the torque-limited planner share (random tilted-axis chains of any link count and the
special cases of tests/test_gpu_dyn_chain.py).  Depends on mpmath and numpy only (and on the ctypes layout of the model).
"""
import numpy as np
from mpmath import mp, mpf

from batotp_amd import capi

DPS = 50


# ---- the definition -----------------------------------------------------------------------------------------------------------
def _v(x):
    return [mpf(float(t)) for t in x]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mv(R, v):
    return [_dot(R[0], v), _dot(R[1], v), _dot(R[2], v)]


def _mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _rodrigues(a, q):
    """rotation by q about the unit vector a"""
    c, s = mp.cos(q), mp.sin(q)
    K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
    return [[c * (1 if i == j else 0) + s * K[i][j] + (1 - c) * a[i] * a[j] for j in range(3)] for i in range(3)]


class _Chain:
    """the model's numbers as mpf"""

    def __init__(self, model):
        self.n = int(model.n_links)
        self.unit = (mp.pi / 180) if model.degrees else mpf(1)
        self.g = _v(model.gravity)
        self.axis, self.off, self.com, self.mass, self.inertia, self.fv = [], [], [], [], [], []
        for i in range(self.n):
            L = model.link[i]
            a = _v(L.axis)
            norm = mp.sqrt(_dot(a, a))
            self.axis.append([t / norm for t in a])
            self.off.append(_v(L.off))
            self.com.append(_v(L.com))
            self.mass.append(mpf(float(L.mass)))
            xx, yy, zz, xy, xz, yz = _v(L.inertia)
            self.inertia.append([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
            self.fv.append(mpf(float(L.fv)))

    def frames(self, q):
        """per link: joint origin p, orientation R, joint axis z and centre of mass c, all in base coordinates"""
        R = [[mpf(1 if i == j else 0) for j in range(3)] for i in range(3)]
        p = [mpf(0)] * 3
        out = []
        for i in range(self.n):
            d = _mv(R, self.off[i])
            p = [p[k] + d[k] for k in range(3)]
            z = _mv(R, self.axis[i])                       # (the axis is the same in link and parent coordinates)
            R = _mm(R, _rodrigues(self.axis[i], q[i]))
            d = _mv(R, self.com[i])
            out.append((p, R, z, [p[k] + d[k] for k in range(3)]))
        return out

    def mass_matrix(self, q):
        """M = sum_i m_i Jv_i^T Jv_i + Jw_i^T (R_i I_i R_i^T) Jw_i: column j of Jv_i is z_j x (c_i - p_j), of Jw_i z_j (j <= i)"""
        n, fr = self.n, self.frames(q)
        M = [[mpf(0)] * n for _ in range(n)]
        for i in range(n):
            _, R, _, c = fr[i]
            Rt = [[R[b][a] for b in range(3)] for a in range(3)]
            Ib = _mm(_mm(R, self.inertia[i]), Rt)
            jv = [_cross(fr[j][2], [c[k] - fr[j][0][k] for k in range(3)]) for j in range(i + 1)]
            iz = [_mv(Ib, fr[j][2]) for j in range(i + 1)]
            for j in range(i + 1):
                for k in range(j, i + 1):
                    M[j][k] += self.mass[i] * _dot(jv[j], jv[k]) + _dot(fr[j][2], iz[k])
        for j in range(n):
            for k in range(j):
                M[j][k] = M[k][j]
        return M

    def gravity_gradient(self, q):
        """dU/dq_k = - sum_{i >= k} m_i g . (z_k x (c_i - p_k))"""
        n, fr = self.n, self.frames(q)
        out = []
        for k in range(n):
            p, _, z, _ = fr[k]
            out.append(-sum(self.mass[i] * _dot(self.g, _cross(z, [fr[i][3][t] - p[t] for t in range(3)])) for i in range(k, n)))
        return out


def _mat_vec(M, v):
    return [sum(M[j][k] * v[k] for k in range(len(v))) for j in range(len(v))]


def coefficients(model, q, q1, q2):
    """(a1, a2, a3, a4), each a list of n_links mpf values, of `model` at the configuration q with path derivatives q1 = q',
    q2 = q'' -- in the model's own unit (degrees if model.degrees), as the knot samples of a batch hold them"""
    with mp.workdps(DPS):
        ch = _Chain(model)
        n = ch.n
        q = [ch.unit * mpf(float(t)) for t in q[:n]]
        q1 = [ch.unit * mpf(float(t)) for t in q1[:n]]
        q2 = [ch.unit * mpf(float(t)) for t in q2[:n]]
        h = mpf(10) ** (-(DPS // 3))
        M = ch.mass_matrix(q)
        a1 = _mat_vec(M, q1)
        # Mdot q' = d/ds [M(q(s))] q' along q' (the momentum M q' differentiated with q' held)
        mp_ = _mat_vec(ch.mass_matrix([q[k] + h * q1[k] for k in range(n)]), q1)
        mm_ = _mat_vec(ch.mass_matrix([q[k] - h * q1[k] for k in range(n)]), q1)
        mdot = [(mp_[k] - mm_[k]) / (2 * h) for k in range(n)]

        def kinetic(qq):
            return _dot_n(q1, _mat_vec(ch.mass_matrix(qq), q1)) / 2
        dT = []
        for k in range(n):
            up = [q[j] + (h if j == k else 0) for j in range(n)]
            dn = [q[j] - (h if j == k else 0) for j in range(n)]
            dT.append((kinetic(up) - kinetic(dn)) / (2 * h))
        mq2 = _mat_vec(M, q2)
        a2 = [mq2[k] + mdot[k] - dT[k] for k in range(n)]
        a3 = [ch.fv[k] * q1[k] for k in range(n)]
        a4 = ch.gravity_gradient(q)
        return a1, a2, a3, a4


def _dot_n(a, b):
    return sum(x * y for x, y in zip(a, b))


def coefficients_f64(model, q, q1, q2):
    """the same rounded to doubles: [4][n_links]"""
    with mp.workdps(DPS):
        return np.array([[float(v) for v in fam] for fam in coefficients(model, q, q1, q2)])


# ---- chain models the tests share ---------------------------------------------------------------------------------------------
def copy_model(model):
    return capi.SerialModel.from_buffer_copy(bytes(model))


def random_chain(n_links, degrees, seed=None):
    """every term in play (tilted axes, offsets, centres of mass, full inertia tensors, friction, tilted gravity): random_model of
    tests/test_gpu_invdyn.py for any link count, in degrees or radians"""
    from test_gpu_invdyn import random_model
    m = random_model(seed=(40 + n_links) if seed is None else seed, n_links=n_links)
    m.degrees = 1 if degrees else 0
    return m


def frictionless(model):
    """fv = 0 in every joint: a3 is identically 0"""
    m = copy_model(model)
    for i in range(m.n_links):
        m.link[i].fv = 0.0
    return m


def weightless(model):
    """no gravity: a4 is identically 0"""
    m = copy_model(model)
    for j in range(3):
        m.gravity[j] = 0.0
    return m


def massless_last_link(model):
    """the last link without mass and inertia: its rows of a1, a2 and a4 are 0 (a1 under the threshold of reference ba.cpp:1500)"""
    m = copy_model(model)
    L = m.link[m.n_links - 1]
    L.mass = 0.0
    for j in range(6):
        L.inertia[j] = 0.0
    return m


def axis_aligned(n_links, degrees, seed=7):
    """axes along x, y or z in turn, principal axes of inertia along the link axes (no products)"""
    m = random_chain(n_links, degrees, seed)
    for i in range(n_links):
        L = m.link[i]
        for j in range(3):
            L.axis[j] = 1.0 if j == (i + 2) % 3 else 0.0
            L.inertia[3 + j] = 0.0
    return m


def knot_scale(model):
    """amplitude factor of helpers.random_knots for joint paths of this model (tens of degrees, or the same in radians)"""
    return 40.0 if model.degrees else 0.7
