"""GLS stabilisation and the body force in the SUPG / GLS strong residual (alfi/stabilisation.py:47-97, alfi/solver.py:204-234):
the C++ host pass against the NumPy restatement of tests/gls_restatement.py, its Newton linearisation against central
differences of that restatement, and the pins that tie the two kinds and the load together.  Host side only."""
import numpy as np
import pytest

from alfi_amd import _hostlib
from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem, build_hierarchy, BSR
import gls_restatement as R

CASES = [(lambda: TwoDimLidDrivenCavityProblem(3), 2), (lambda: ThreeDimLidDrivenCavityProblem(1), 1),
         (lambda: ThreeDimLidDrivenCavityProblem(1), 2)]
IDS = ["2d-p2", "3d-p1fb", "3d-p2fb"]


def _level(mk, k):
    lv, _ = build_hierarchy(mk(), 1, k, Re=100.0, patches=False)
    return lv[1]


def _fields(L, seed=3):
    V, d = L.V, L.bs
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((V.num_nodes, d))
    W = rng.standard_normal((V.num_nodes, d))
    nq = len(_hostlib.supg_rule(V)[1])
    fq = rng.standard_normal((V.cell_nodes.shape[0], nq, d))
    return U, W, fq


def _host(kind, L, U, W, nu, weight, magic, fq, vals=True):
    F = np.zeros(L.n)
    A = np.zeros((L.A.colidx.shape[0], L.bs, L.bs)) if vals else None
    if kind == "gls":
        _hostlib.gls(L.V, U, W, nu, weight, magic, L.A.rowptr, L.A.colidx, A, F, fq=fq)
    else:
        _hostlib.supg(L.V, U, nu, weight, magic, L.A.rowptr, L.A.colidx, A, F, fq=fq)
    return F, A


@pytest.mark.parametrize("mk,k", CASES, ids=IDS)
@pytest.mark.parametrize("kind", ["supg", "gls"])
def test_residual_and_jacobian_against_the_restatement(mk, k, kind):
    L = _level(mk, k)
    V, d = L.V, L.bs
    U, W, fq = _fields(L)
    nu, weight, magic = 0.02, 0.05, 9.0
    F, vals = _host(kind, L, U, W, nu, weight, magic, fq)
    Fr = R.residual(kind, V, U, nu, weight, magic, W=W, fq=fq)
    assert np.abs(F - Fr).max() < 1e-12 * np.abs(Fr).max()
    # linearisation with respect to U, the wind and the load held fixed
    J = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx, vals).to_scipy()
    eps = 1e-6
    for seed in range(2):
        v = np.random.default_rng(seed).standard_normal(L.n)
        fd = (R.residual(kind, V, U + eps * v.reshape(-1, d), nu, weight, magic, W=W, fq=fq)
              - R.residual(kind, V, U - eps * v.reshape(-1, d), nu, weight, magic, W=W, fq=fq)) / (2 * eps)
        assert np.abs(J @ v - fd).max() < 1e-6 * np.abs(fd).max()


@pytest.mark.parametrize("mk,k", CASES, ids=IDS)
def test_supg_without_load_is_unchanged(mk, k):
    """fq = None is the SUPG pass of before the load existed: the same as an explicit zero table, and as the restatement."""
    L = _level(mk, k)
    U, W, fq = _fields(L)
    nu, weight, magic = 0.02, 0.05, 9.0
    F0, A0 = _host("supg", L, U, None, nu, weight, magic, None)
    F1, A1 = _host("supg", L, U, None, nu, weight, magic, np.zeros_like(fq))
    assert np.abs(F0 - F1).max() <= 1e-15 * np.abs(F0).max()
    assert np.array_equal(A0, A1)
    Fr = R.residual("supg", L.V, U, nu, weight, magic)
    assert np.abs(F0 - Fr).max() < 1e-12 * np.abs(Fr).max()


@pytest.mark.parametrize("mk,k", CASES, ids=IDS)
def test_gls_with_no_viscosity_and_the_state_as_wind_is_supg(mk, k):
    L = _level(mk, k)
    U, _, _ = _fields(L)
    weight, magic = 0.05, 9.0
    Fg, Ag = _host("gls", L, U, U, 0.0, weight, magic, None)
    Fs, _ = _host("supg", L, U, None, 0.0, weight, magic, None)
    assert np.abs(Fg - Fs).max() < 1e-13 * np.abs(Fs).max()
    assert np.abs(Ag).max() > 0.0


@pytest.mark.parametrize("mk,k", CASES, ids=IDS)
@pytest.mark.parametrize("kind", ["supg", "gls"])
def test_load_equal_to_the_strong_operator_cancels(mk, k, kind):
    """f = Lu(U) at the points: the strong residual vanishes, so does the stabilisation's residual (a sign error in the load
    would double it instead)."""
    L = _level(mk, k)
    U, W, _ = _fields(L)
    nu, weight, magic = 0.02, 0.05, 9.0
    _, Lu = R.strong_residual(L.V, U, nu)
    F0, _ = _host(kind, L, U, W, nu, weight, magic, None, vals=False)
    F, _ = _host(kind, L, U, W, nu, weight, magic, Lu, vals=False)
    assert np.abs(F0).max() > 0.0
    assert np.abs(F).max() < 1e-12 * np.abs(F0).max()


def test_supg_points_follow_the_rule():
    L = _level(*CASES[1])
    V = L.V
    lam, wq = _hostlib.supg_rule(V)
    x = _hostlib.supg_points(V)
    assert x.shape == (V.cell_nodes.shape[0], len(wq), V.dim)
    m = V.mesh
    assert np.allclose(x[5, 2], lam[2] @ m.coords[m.cells[5]])


def test_refusals():
    """GLS with the Scott-Vogelius pair and GLS on partitioned levels raise before anything is built; SUPG with a body force on
    partitioned levels raises when the load tables would be formed."""
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.dist import DistNavierStokesSolver
    with pytest.raises(NotImplementedError):
        HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 1, 2, discretisation="sv", stabilisation_type="gls")
    with pytest.raises(NotImplementedError):
        DistNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 1, 2, stabilisation_type="gls")
    s = DistNavierStokesSolver.__new__(DistNavierStokesSolver)
    with pytest.raises(NotImplementedError):
        s._stabilisation_load(lambda x: np.zeros_like(x))
