"""CPU: the oracle's dynamics coefficients a1..a4 of serial chains of 1 to 8 links against tests/dyn_reference.py -- Lagrange's
equations on the chain's kinematics in 50-digit arithmetic, independent of the recursion (oracle/batotp_oracle_dyn.c: bo_rnea).

The reference has no dynamics model for any chain but the two-link arm, so nothing of it pins these values ("parity unpinned",
DESIGN.md 5).  This file pins the model-independent part -- that the three passes of the recursion ARE M q', M q'' + Mdot q' - dT/dq
and dU/dq of the table's chain, for every link count, both units, tilted axes and full inertia tensors -- to rounding."""
import numpy as np
import pytest

import dyn_reference as dr
import helpers
from batotp_amd import capi

# |oracle - restatement| of a1, a2 and a4, relative to the largest |value| of the coefficient family on the path.  Measured over
# all the cases below (8 knots per path, both ends among them): 6.3e-16 (a1 4.9e-16, a2 3.6e-16, a4 6.3e-16).  The bound is the
# project's usual margin: 100 x the measured maximum, rounded up to a power of ten.
ORACLE_DYN_BOUND = 1e-13
N_SAMPLED = 8

CASES = [(n, deg) for n in range(1, 9) for deg in (1, 0)]
_PATHS = {}


def oracle_path(oracle_ctx, n_links, degrees):
    """(model, samples [nJ][3][N], oracle a1..a4 [4][nJ][N], sampled knots, restatement at those knots [K][4][nJ]) -- once per case"""
    key = (n_links, degrees)
    if key not in _PATHS:
        model = dr.random_chain(n_links, degrees)
        rng = np.random.default_rng(100 * n_links + degrees)
        N = 40 + 3 * n_links
        y = helpers.random_knots(rng, n_links, N, dr.knot_scale(model))
        prob = capi.make_problem(n_links, 0, flags=capi.F_TRQ_ON | capi.F_HOST_TRIG | capi.F_JNT_ACC_ON, jnt_vel_max=[1e3] * n_links,
                                 jnt_acc_max=[1e4] * n_links, jnt_trq_max=[1e9] * n_links, jnt_trq_min=[-1e9] * n_links)
        b = capi.Batch(oracle_ctx, prob, [N], 64)
        b.upload_knots(0, [y], [0.01])
        helpers.precompute_with_trig(oracle_ctx, b, prob, 1, serial_model=model)
        samp = np.stack([b.samples(0, j) for j in range(n_links)])
        dyn = np.stack([np.stack([b.dyn(0, k, r) for r in range(n_links)]) for k in (1, 2, 3, 4)])
        b.close()
        knots = [0, N - 1] + sorted(int(v) for v in rng.choice(np.arange(1, N - 1), N_SAMPLED - 2, replace=False))
        ref = np.stack([dr.coefficients_f64(model, samp[:, 0, k], samp[:, 1, k], samp[:, 2, k]) for k in knots])
        for a in (samp, dyn, ref):
            a.setflags(write=False)
        _PATHS[key] = (model, samp, dyn, knots, ref)
    return _PATHS[key]


def family_errors(dyn, knots, ref):
    """largest |dyn - ref| over the sampled knots per coefficient family, relative to the family's largest |value| on the path"""
    scale = np.abs(dyn).max(axis=(1, 2))
    err = np.array([np.abs(dyn[f][:, knots] - ref[:, f, :].T).max() for f in range(4)])
    return err / np.where(scale > 0, scale, 1.0)


@pytest.mark.parametrize("n_links,degrees", CASES)
def test_oracle_coefficients_are_lagranges(oracle_ctx, n_links, degrees):
    model, samp, dyn, knots, ref = oracle_path(oracle_ctx, n_links, degrees)
    assert np.all(np.isfinite(dyn)) and np.abs(dyn[0]).max() > 0 and np.abs(dyn[3]).max() > 0
    # a3 is one product of two doubles: exact
    unit = (3.14159265358979323846 / 180.0) if degrees else 1.0
    for j in range(n_links):
        fv = float(model.link[j].fv)
        want = np.array([fv * (unit * float(v)) for v in samp[j][1]])
        helpers.assert_bit_equal(dyn[2][j], want, f"{n_links} links, degrees {degrees}: a3 of row {j}")
    err = family_errors(dyn, knots, ref)
    print(f"{n_links} links, degrees {degrees}: |oracle - restatement| / max|family|: a1 {err[0]:.2e}, a2 {err[1]:.2e}, "
          f"a3 {err[2]:.2e}, a4 {err[3]:.2e}")
    for f in (0, 1, 3):
        assert err[f] < ORACLE_DYN_BOUND, (n_links, degrees, f"a{f + 1}", err[f])


def _swap_inertia_products(m):
    L = m.link[m.n_links - 1]
    L.inertia[3], L.inertia[5] = L.inertia[5], L.inertia[3]      # xy <-> yz: the ordering of the header


def _negate_inertia_product(m):
    m.link[0 if m.n_links == 1 else 1].inertia[4] *= -1.0


def _move_centre_of_mass(m):
    m.link[m.n_links - 1].com[1] += 1e-9


def _flip_gravity(m):
    for j in range(3):
        m.gravity[j] *= -1.0


def _other_unit(m):
    m.degrees = 0 if m.degrees else 1


FAULTS = {"inertia products in another order": (_swap_inertia_products, (0, 1)), "one inertia product negated": (_negate_inertia_product, (0, 1)),
          "a centre of mass moved by 1e-9 m": (_move_centre_of_mass, (0, 1, 3)), "gravity's sign": (_flip_gravity, (3,)),
          "the other unit": (_other_unit, (0, 1, 3))}


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("n_links,degrees", [(1, 0), (3, 1), (8, 0)])
def test_the_comparison_notices_a_wrong_model(oracle_ctx, n_links, degrees, fault):
    """the restatement of a model with one seeded fault against the oracle's values of the right model: every family the fault
    reaches leaves the bound (were the oracle wrong in that way, the test above would fail)"""
    model, samp, dyn, knots, _ = oracle_path(oracle_ctx, n_links, degrees)
    seed, families = FAULTS[fault]
    bad = dr.copy_model(model)
    seed(bad)
    ks = knots[:3]
    ref = np.stack([dr.coefficients_f64(bad, samp[:, 0, k], samp[:, 1, k], samp[:, 2, k]) for k in ks])
    err = family_errors(dyn, ks, ref)
    for f in families:
        assert err[f] > 100 * ORACLE_DYN_BOUND, (fault, f"a{f + 1}", err[f])


def test_the_comparison_notices_a_wrong_value(oracle_ctx):
    """a copy of the oracle's values with one entry off by 1e-12 of its family's scale (a sign on a small term) leaves the bound"""
    model, samp, dyn, knots, ref = oracle_path(oracle_ctx, 5, 1)
    for f in (0, 1, 3):
        bad = dyn.copy()
        bad[f][3][knots[-1]] += 1e-12 * np.abs(dyn[f]).max()
        assert family_errors(bad, knots, ref)[f] > ORACLE_DYN_BOUND
        assert family_errors(dyn, knots, ref)[f] < ORACLE_DYN_BOUND
