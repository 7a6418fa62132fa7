"""Adjoint of the Navier-Stokes Jacobian (alfi/solver.py:520-535, alfi_amd.adjoint) on the host: the conventions of the
device path -- sign, homogenised Dirichlet conditions, the pressure nullspace -- pinned by a gradient check of the NumPy / SciPy
restatement in tests/adjoint_restatement.py, and the functionals' gradients.  No GPU."""
import numpy as np
import pytest

from alfi_amd.adjoint import LinearFunctional, LoadFunctional, adjoint_rhs
import adjoint_restatement as R


@pytest.fixture(scope="module")
def rs():
    return R.Restatement()


def _wfield(x):
    w = np.zeros_like(x)
    w[:, 0] = np.cos(0.5 * np.pi * x[:, 0]) * x[:, 1]
    w[:, 1] = 1.0 + x[:, 0] * x[:, 1]
    return w


class _Host(object):
    """What a functional reads of a solver: the levels."""

    def __init__(self, L):
        self.levels = [L]


def test_adjoint_gradient_against_central_differences(rs):
    """dJ/dm = dJ/dm|_z + lam . dF/dm for the body-force amplitude m at Re 50 (continuation 10 -> 50), against central
    differences of J(z(m +- h)); J has a velocity part (a load functional) and a pressure part of nonzero sum."""
    res, m0, h = [10.0, 50.0], 0.7, 1e-4
    u, p, nu = rs.solve(res, m0)
    F = rs.residual(u, p, nu, m0)
    assert np.linalg.norm(F) < 1e-9
    Jl = LoadFunctional(_wfield)
    g_p = np.random.default_rng(1).standard_normal(rs.n_p) + 0.3
    J = LinearFunctional(Jl.gradient(_Host(rs.L), u, p)[0], g_p)
    g_u, gp = J.gradient(None, u, p)
    lam_u, lam_p, _ = rs.adjoint(u, nu, g_u, gp)
    dFdm = rs.residual(u, p, nu, 1.0) - rs.residual(u, p, nu, 0.0)          # the residual is affine in m
    grad = lam_u @ dFdm[:rs.n_u] + lam_p @ dFdm[rs.n_u:]
    up, pp, _ = rs.solve(res, m0 + h)
    um, pm, _ = rs.solve(res, m0 - h)
    fd = (J.value(None, up, pp) - J.value(None, um, pm)) / (2 * h)
    assert abs(grad - fd) <= 1e-6 * abs(fd), (grad, fd)
    # the sign convention: J^T lam = -g on the free rows, zero on the Dirichlet rows
    K = rs.jacobian(u, nu)
    r = K.T @ np.concatenate([lam_u, lam_p]) - adjoint_rhs(g_u, gp, rs.bc, rs.n_p, rs.vol)
    assert np.linalg.norm(r[:rs.n_u]) < 1e-8 * np.linalg.norm(g_u)
    assert np.abs(lam_u[rs.bc]).max() == 0.0


def test_adjoint_rhs_projection(rs):
    rng = np.random.default_rng(4)
    g_u, g_p = rng.standard_normal(rs.n_u), rng.standard_normal(rs.n_p) + 2.0
    rhs = adjoint_rhs(g_u, g_p, rs.bc, rs.n_p, rs.vol)
    assert np.all(rhs[rs.bc] == 0.0)
    free = np.setdiff1d(np.arange(rs.n_u), rs.bc)
    assert np.array_equal(rhs[free], -g_u[free])
    assert abs(rhs[rs.n_u:].sum()) < 1e-12 * np.abs(g_p).sum()
    # P^T g_p: the change is along vol, and pressure parts that already sum to zero pass unchanged
    dp = rhs[rs.n_u:] + g_p
    assert np.allclose(dp, rs.vol * (dp @ rs.vol) / (rs.vol @ rs.vol), rtol=0, atol=1e-12)
    g0 = g_p - g_p.mean()
    assert np.allclose(adjoint_rhs(g_u, g0, rs.bc, rs.n_p, rs.vol)[rs.n_u:], -g0, rtol=0, atol=1e-14)
    # no nullspace: the pressure part as given; no pressure part: zeros
    assert np.array_equal(adjoint_rhs(g_u, g_p, rs.bc, rs.n_p)[rs.n_u:], -g_p)
    assert np.array_equal(adjoint_rhs(g_u, None, rs.bc, rs.n_p, rs.vol)[rs.n_u:], np.zeros(rs.n_p))


def test_load_functional_gradient(rs):
    J = LoadFunctional(_wfield)
    host = _Host(rs.L)
    rng = np.random.default_rng(2)
    u, p = rng.standard_normal(rs.n_u), rng.standard_normal(rs.n_p)
    g_u, g_p = J.gradient(host, u, p)
    assert g_p is None and g_u.shape == (rs.n_u,)
    for seed in range(3):
        v = np.random.default_rng(10 + seed).standard_normal(rs.n_u)
        h = 1e-3
        fd = (J.value(host, u + h * v, p) - J.value(host, u - h * v, p)) / (2 * h)
        assert abs(g_u @ v - fd) <= 1e-10 * max(1.0, abs(fd))
    # J = int w . u: w = 1 in the first component integrates u = e_x to |domain| = 2 x 2
    from alfi_amd.mms import load_vector
    ones = load_vector(rs.L.V, lambda x: np.ones_like(x))
    assert abs(ones @ np.tile([1.0, 0.0], rs.n_u // 2) - 4.0) < 1e-12    # |domain| = 2 x 2


def test_partitioned_solver_refuses_the_adjoint():
    """DistNavierStokesSolver.setup_adjoint: J^T needs the mirror blocks of the ghost columns, which other ranks hold."""
    from alfi_amd.dist import DistNavierStokesSolver as cls
    with pytest.raises(NotImplementedError, match="partitioned"):
        cls.setup_adjoint(object.__new__(cls), LoadFunctional(_wfield))
