"""solver_type allu on the device: fieldsplit_0 = an exact solve with multifrontal factors of the finest operator
(alfi_saddle_set_velocity_solver / alfi_saddle_factor_velocity; alfi/solver.py:346-352, 414).  The oracle is
oracle.alfi_oracle.saddle_solve with SciPy's sparse LU of the finest operator read back from the device as fieldsplit_0.
-m gpu"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from alfi_amd.adjoint import LoadFunctional, adjoint_rhs
from alfi_amd.nssolver import HipNavierStokesSolver
from alfi_amd.problem import BSR, TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem
from oracle import alfi_oracle as O


class _LU(object):
    """fieldsplit_0 of the oracle: the exact solve (``fcycle`` is the name saddle_solve calls)."""

    def __init__(self, A):
        self.fcycle = spla.splu(sp.csc_matrix(A)).solve


def _finest(s):
    """The finest operator as the device holds it now (scipy CSR)."""
    L = s.levels[-1]
    vals = s.hmg.mg.levels[-1].get_values()
    return BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx, vals).to_scipy().tocsr()


def _precond_ref(s, A, v):
    lu = _LU(A)
    n = s.n_u
    yu = lu.fcycle(v[:n])
    yp = -(s.nu + s.gamma) / s.vol * (v[n:] - s.B @ yu)
    yu = lu.fcycle(v[:n] - s.B.T @ yp)
    return np.concatenate([yu, yp - yp.mean()])


def _check_exact_precond(s, seed=1):
    A = _finest(s)
    v = np.random.default_rng(seed).standard_normal(s.n_u + s.n_p)          # b_p != 0
    dv, dy = s.ctx.vec(v), s.ctx.vec(s.n_u + s.n_p)
    s.saddle.precond(dv, dy)
    got, ref = dy.get(), _precond_ref(s, A, v)
    n = s.n_u
    eu = np.abs(got[:n] - ref[:n]).max() / np.abs(ref[:n]).max()
    ep = np.abs(got[n:] - ref[n:]).max() / np.abs(ref[n:]).max()
    assert eu < 1e-9 and ep < 1e-9, (eu, ep)
    return A


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("case", ["ldc2d-supg", "ldc3d-p1fb"])
def test_exact_preconditioner_and_no_stale_factors(case):
    """Tests 1 and 4 of the feature: alfi_saddle_precond with the direct fieldsplit_0 equals the NumPy restatement with the
    exact A^-1 of an advective operator (the Jacobian of a Newton step at Re 100); after a later Newton step it still does,
    against the operator of then; a refresh / value upload / transpose without re-factoring makes the solve refuse."""
    if case == "ldc2d-supg":
        s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="supg", solver_type="allu",
                                  snes_max_it=1)
    else:                    # [P1+FB]^3: the bubble dofs are part of the factored operator
        s = HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 1, solver_type="allu", snes_max_it=1)
    _, info = s.solve(100.0)
    assert info["nonlinear_iter"] == 1 and info["linear_iter"] >= 1
    A0 = _check_exact_precond(s)
    assert abs(A0 - A0.T).max() > 1e-6 * abs(A0).max()         # advective: not symmetric
    nbytes, probe = s.saddle.velocity_info()
    assert nbytes > 0 and 0.0 <= probe < 1e-8, (nbytes, probe)
    # a later Newton step: new operator, new factors -- exact against the current operator, not the old one
    s.solve(100.0)
    A1 = _check_exact_precond(s, seed=2)
    assert abs(A1 - A0).max() > 1e-8 * abs(A0).max()
    # stale factors are refused (ALFI_E_STATE), never used
    fin = s.hmg.mg.levels[-1]
    db, dx = s.ctx.vec(np.ones(s.n_u)), s.ctx.vec(s.n_u)
    s.saddle.velocity_solve(db, dx)
    s._refresh_device(None, 1.0)                 # device refresh without re-factoring
    with pytest.raises(hip.AlfiHipError, match="error -3"):
        s.saddle.velocity_solve(db, dx)
    dv, dy = s.ctx.vec(s.n_u + s.n_p), s.ctx.vec(s.n_u + s.n_p)
    with pytest.raises(hip.AlfiHipError, match="error -3"):
        s.saddle.precond(dv, dy)
    s.saddle.factor_velocity()
    s.saddle.velocity_solve(db, dx)
    fin.update_values(fin.get_values())          # the host-upload path
    with pytest.raises(hip.AlfiHipError, match="error -3"):
        s.saddle.velocity_solve(db, dx)
    s.saddle.factor_velocity()
    fin.transpose()                              # the adjoint's transpose
    with pytest.raises(hip.AlfiHipError, match="error -3"):
        s.saddle.velocity_solve(db, dx)
    s.saddle.factor_velocity()
    _check_exact_precond(s, seed=3)
    s.close()


def test_ideal_al_counts_match_the_oracle():
    """Test 2: one linearised solve on ldc2d baseN 8, nref 1 at Re 100 per gamma; the device counts equal the oracle's within
    one, and the ideal AL preconditioner needs few iterations at large gamma (the only approximation left is DGMassInv)."""
    its = {}
    ctx = hip.Context(0)
    for gamma in (0.0, 1.0, 1e2, 1e4):
        s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(8), 1, 2, gamma=gamma, solver_type="allu", snes_max_it=1,
                                  ctx=ctx)
        s.solve(100.0)                           # the finest operator is now the Jacobian of that step, factored
        A = _finest(s)
        rng = np.random.default_rng(7)
        b = np.concatenate([rng.standard_normal(s.n_u), np.zeros(s.n_p)])
        b[s.levels[-1].bc_dofs] = 0.0
        db, dx = s.ctx.vec(b), s.ctx.vec(s.n_u + s.n_p)
        n_dev, rn = s.saddle.solve(db, dx, s.rtol, s.atol, 500, 30)
        x, n_ora, _ = O.saddle_solve(_LU(A), A, s.B, s.vol, s.nu, s.gamma, b, rtol=s.rtol, atol=s.atol)
        assert abs(n_dev - n_ora) <= 1, (gamma, n_dev, n_ora)
        assert rn <= 10 * max(s.rtol * np.linalg.norm(b), s.atol), (gamma, rn)
        assert _rel(dx.get()[:s.n_u], x[:s.n_u]) < 1e-6, gamma
        its[gamma] = n_dev
        s.close()
    assert its[1e4] <= 4 and its[1e4] < its[0.0], its
    ctx.close()


def _continuation(s, res):
    out = {}
    for re in res:
        _, info = s.solve(re)
        assert info["converged"], (re, info)
        out[re] = info
    return out


def test_newton_parity_with_almg():
    """Test 3: allu and almg reach the same Newton iterates on ldc2d baseN 8, nref 2 with SUPG, Re 0 -> 1 -> 10 -> 100;
    allu needs no more outer iterations per Newton step than almg."""
    res = (0.0, 1.0, 10.0, 100.0)
    ctx = hip.Context(0)
    out = {}
    for st in ("almg", "allu"):
        s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(8), 2, 2, stabilisation_type="supg", solver_type=st, ctx=ctx)
        info = _continuation(s, res)
        out[st] = (s.u.copy(), s.p.copy(), info, dict(s.timings))
        s.close()
    ua, pa, ia, _ = out["almg"]
    ul, pl, il, tl = out["allu"]
    for re in res:
        assert abs(ia[re]["nonlinear_iter"] - il[re]["nonlinear_iter"]) <= 1, (re, ia[re], il[re])
    assert _rel(ul, ua) < 1e-7 and _rel(pl, pa) < 1e-7, (_rel(ul, ua), _rel(pl, pa))
    avg = lambda info: sum(i["linear_iter"] for i in info.values()) / max(1, sum(i["nonlinear_iter"] for i in info.values()))
    assert avg(il) <= avg(ia), (avg(il), avg(ia))
    assert tl["factor_s"] > 0.0
    ctx.close()


def test_host_assembly_path():
    """ALFI_DEVICE_ASSEMBLY=0: the host rediscretises, uploads the finest operator and the direct factors follow it -- the same
    Newton iterates as the device refresh."""
    res = (0.0, 10.0, 100.0)
    ctx = hip.Context(0)
    u = {}
    for dev in (True, False):
        s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="supg", solver_type="allu",
                                  device_assembly=dev, ctx=ctx)
        assert s.device_assembly == dev
        _continuation(s, res)
        u[dev] = s.u.copy()
        s.close()
    assert _rel(u[False], u[True]) < 1e-7, _rel(u[False], u[True])
    ctx.close()


def test_sv_burman_reaches_re100():
    """Test 5: the Scott-Vogelius pair with Burman stabilisation (weight 5e-3), [P2]^2 baseN 4, nref 1, to Re 100; the
    velocity agrees with almg's."""
    res = (0.0, 1.0, 10.0, 100.0)
    ctx = hip.Context(0)
    u = {}
    for st in ("almg", "allu"):
        s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, discretisation="sv", stabilisation_type="burman",
                                  stabilisation_weight=5e-3, solver_type=st, ctx=ctx)
        _continuation(s, res)
        u[st] = s.u.copy()
        s.close()
    assert _rel(u["allu"], u["almg"]) < 1e-7, _rel(u["allu"], u["almg"])
    ctx.close()


def _w(x):
    w = np.zeros_like(x)
    w[:, 0] = np.cos(0.5 * np.pi * x[:, 1])
    w[:, 1] = 1.0 + x[:, 0] * x[:, 1]
    return w


def test_adjoint_with_allu():
    """Test 6: the allu adjoint (transposed finest operator re-factored) of a LoadFunctional agrees with the almg adjoint, and
    the adjoint system holds against SciPy: J_F^T lam = -dJ with the transposed operator read back from the device."""
    ctx = hip.Context(0)
    lam = {}
    for st in ("almg", "allu"):
        s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="supg", solver_type=st, ctx=ctx)
        _continuation(s, (0.0, 1.0, 10.0, 50.0))
        J = LoadFunctional(_w)
        s.setup_adjoint(J)
        info = s.solver_adjoint.solve(rtol=1e-12, atol=1e-14)
        assert info["converged"], info
        lam[st] = np.concatenate(s.z_adj)
        if st == "allu":
            At = _finest(s)                   # the device holds A^T at z* now (and its factors)
            g_u, g_p = J.gradient(s, s.u, s.p)
            rhs = adjoint_rhs(g_u, g_p, s.levels[-1].bc_dofs, s.n_p, s.vol)
            lu, lp = s.z_adj
            # J_F^T = [[A^T, B^T], [B, 0]] (P0 pressure: the off-diagonal blocks are the forward ones)
            r_u = At @ lu + s.B.T @ lp - rhs[:s.n_u]
            r_p = s.B @ lu
            assert np.linalg.norm(np.concatenate([r_u, r_p])) < 1e-8 * np.linalg.norm(rhs)
            # and A^T is the transpose of the forward Jacobian at z*: refresh without transposing, compare
            s._refresh_device(None, 1.0)
            A = _finest(s)
            assert abs(At - A.T).max() <= 1e-14 * abs(A).max()
        s.close()
    assert _rel(lam["allu"], lam["almg"]) < 1e-7, _rel(lam["allu"], lam["almg"])
    ctx.close()


def test_memory_guard_refuses_and_leaves_the_context_usable():
    """Test 7: a 1 MB cap on factors + fronts is refused at the analysis, the message names both numbers; an almg solve on
    the same context afterwards succeeds."""
    ctx = hip.Context(0)
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(8), 1, 2, solver_type="allu", direct_max_bytes=1 << 20, ctx=ctx)
    with pytest.raises(hip.AlfiHipError) as e:
        s.solve(0.0)
    msg = str(e.value)
    assert "needs" in msg and "1048576" in msg and "free device memory" in msg, msg
    s.close()
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(8), 1, 2, solver_type="almg", ctx=ctx)
    _, info = s.solve(0.0)
    assert info["converged"], info
    s.close()
    ctx.close()


def test_finest_level_is_the_coarse_level():
    """nref = 0: the finest level is level 0 -- its coarse factors and the direct velocity factors live side by side."""
    ctx = hip.Context(0)
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 0, 2, solver_type="allu", ctx=ctx)
    _continuation(s, (0.0, 10.0))
    coarse = s.hmg.mg.levels[0]
    vbytes = s.saddle.velocity_info()[0]
    coarse.coarse_factor_sparse()                    # the coarse slot of the same level, factored beside the direct factors
    assert coarse.coarse_factor_bytes() > 0
    assert s.saddle.velocity_info()[0] == vbytes
    _check_exact_precond(s)                          # the direct factors are still there, current and exact
    db, dx = s.ctx.vec(np.ones(s.n_u)), s.ctx.vec(s.n_u)
    coarse.coarse_solve(db, dx)
    assert _rel(dx.get(), _LU(_finest(s)).fcycle(np.ones(s.n_u))) < 1e-9
    u = s.u.copy()
    s.close()
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 0, 2, solver_type="almg", ctx=ctx)
    _continuation(s, (0.0, 10.0))
    assert _rel(u, s.u) < 1e-7
    s.close()
    ctx.close()
