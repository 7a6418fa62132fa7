"""Burman interior-penalty stabilisation on the device (-m gpu): the facet pass of the operator refresh and of the residual
(alfi_level_burman / alfi_level_assemble_burman) against the host pass (alfi_host_burman, itself checked against the
restatement in tests/test_burman.py), bitwise reproducibility, and Newton with device and host assembly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd.nssolver import HipNavierStokesSolver, run_solver
from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem

CASES = [pytest.param(lambda: TwoDimLidDrivenCavityProblem(2), 2, 2, id="2d-P2"),
         pytest.param(lambda: ThreeDimLidDrivenCavityProblem(1), 1, 3, id="3d-P3")]


def _solver(mk, nref, k, device_assembly=True, weight=5e-3):
    return HipNavierStokesSolver(mk(), nref, k, discretisation="sv", stabilisation_type="burman",
                                 stabilisation_weight=weight, device_assembly=device_assembly)


@pytest.mark.parametrize("mk,nref,k", CASES)
def test_device_refresh_and_residual_match_host(mk, nref, k):
    s = _solver(mk, nref, k)
    try:
        assert s.device_assembly and all(L.facet_coupling for L in s.levels)
        d = s.problem.dim
        rng = np.random.default_rng(0)
        u = rng.standard_normal(s.n_u)
        u[s.levels[-1].bc_dofs] = 0.0
        s.nu = 0.05
        s._device_states(u)
        winds = [st.get().reshape(-1, d) for st in s._dstate]          # the device's injected states, on the host
        mgl = s.hmg.mg.levels
        for L, dl, st, w in zip(s.levels, mgl, s._dstate, winds):
            host = s.level_values(L, w, 1.0, True)
            dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
            dev = dl.get_values()
            assert np.abs(dev - host).max() <= 1e-12 * np.abs(host).max(), L.level
            # the same refresh in three calls: cell pass without boundary conditions, facet pass added, boundary conditions
            dl.assemble(s.nu, s.gamma, 1.0, st, False)
            dl.burman(s.burman_weight, st, True)
            dl.apply_bc()
            assert np.array_equal(dl.get_values(), dev)
            # other scratch sizes (cells in batches) and a repeat: the same bits
            for scratch in (1 << 16, 1 << 22):
                s.ctx.set_assembly_scratch(scratch)
                dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
                assert np.array_equal(dl.get_values(), dev)
            s.ctx.set_assembly_scratch(24 << 30)
        # residual: device against host
        p = rng.standard_normal(s.n_p)
        Fu_d, Fp_d = s._residual_device(u, p, 1.0)
        s.device_assembly = False
        Fu_h, Fp_h = s.residual(u, p, 1.0)
        s.device_assembly = True
        assert np.abs(Fu_d - Fu_h).max() <= 1e-12 * np.abs(Fu_h).max()
        assert np.abs(Fp_d - Fp_h).max() <= 1e-12 * np.abs(Fp_h).max()
        # the Burman part is really there: the residual without it differs
        s.burman = False
        Fu_0, _ = s._residual_device(u, p, 1.0)
        s.burman = True
        assert np.abs(Fu_0 - Fu_d).max() > 1e-6 * np.abs(Fu_d).max()
    finally:
        s.close()


def test_newton_2d_device_and_host_assembly_agree():
    """Reynolds continuation 10 -> 100 on 2-D SV-P2 with weight 5e-3 (the reference's iters2dsv line)."""
    res = [10.0, 100.0]
    out = []
    for dev in (True, False):
        s = _solver(lambda: TwoDimLidDrivenCavityProblem(2), 2, 2, device_assembly=dev)
        try:
            info = run_solver(s, res)
            out.append((s.u.copy(), s.p.copy(), info))
        finally:
            s.close()
    (ud, pd, idev), (uh, ph, ihost) = out
    for re in res:
        assert idev[re]["converged"] and ihost[re]["converged"], (idev[re], ihost[re])
        assert idev[re]["nonlinear_iter"] == ihost[re]["nonlinear_iter"]
        assert idev[re]["linear_iter"] == ihost[re]["linear_iter"]
    assert np.abs(ud - uh).max() < 1e-8 * np.abs(uh).max()
    # the converged state is a root of the host residual, Burman term included
    s = _solver(lambda: TwoDimLidDrivenCavityProblem(2), 2, 2, device_assembly=False)
    try:
        s.nu = s.char_L * s.char_U / res[-1]
        Fu, Fp = s.residual(ud, pd, 1.0)
        F0u, F0p = s.residual(np.zeros_like(ud) + s.u, np.zeros_like(pd), 1.0)
        assert np.sqrt(Fu @ Fu + Fp @ Fp) < 1e-5 * np.sqrt(F0u @ F0u + F0p @ F0p)
    finally:
        s.close()


def test_newton_3d_p3_device_and_host_assembly_agree():
    res = [10.0]
    out = []
    for dev in (True, False):
        s = _solver(lambda: ThreeDimLidDrivenCavityProblem(1), 1, 3, device_assembly=dev)
        try:
            info = run_solver(s, res)
            out.append((s.u.copy(), info))
        finally:
            s.close()
    (ud, idev), (uh, ihost) = out
    assert idev[10.0]["converged"] and ihost[10.0]["converged"]
    assert idev[10.0]["nonlinear_iter"] == ihost[10.0]["nonlinear_iter"]
    assert np.abs(ud - uh).max() < 1e-8 * np.abs(uh).max()


@pytest.mark.parametrize("mk,nref,k", CASES)
def test_patch_inverses_follow_the_pcpatch_facet_rule(mk, nref, k):
    """After a Burman refresh every macro-star factor is the inverse of A[P, P] minus the K-side facet terms of the facets with
    one cell in the patch (burman.patch_facet_corrections; the rule itself is checked in tests/test_burman.py), and Burman levels
    store dense (not condensed) factors."""
    from alfi_amd.burman import patch_facet_corrections
    from alfi_amd.problem import BSR
    s = _solver(mk, nref, k)
    try:
        d = s.problem.dim
        u = np.random.default_rng(5).standard_normal(s.n_u)
        u[s.levels[-1].bc_dofs] = 0.0
        s.nu = 0.05
        s._device_states(u)
        for L, dl, st, obj in zip(s.levels, s.hmg.mg.levels, s._dstate, s.hmg.pc_objs):
            if obj is None:
                continue
            assert not obj.condensed
            dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
            dl.factor()
            A = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx,
                    s.level_values(L, st.get().reshape(-1, d), 1.0, True)).to_scipy().tocsr()
            beta, scale = L.facet_beta
            ptr, col, fac, sv = patch_facet_corrections(L.V, L.facets, obj.patch_ptr, obj.patch_dofs)
            npatch = len(obj.patch_ptr) - 1
            ncorr = 0
            for p in sorted(set([0, npatch // 2, npatch - 1])):
                dofs = obj.patch_dofs[obj.patch_ptr[p]:obj.patch_ptr[p + 1]]
                n = dofs.size
                Ap = A[dofs][:, dofs].toarray()
                r0 = obj.patch_ptr[p] // d
                for i in range(n // d):
                    for q in range(ptr[r0 + i], ptr[r0 + i + 1]):
                        ncorr += 1
                        for c in range(d):
                            Ap[i * d + c, col[q] * d + c] -= scale * beta[fac[q]] * sv[q]
                X = dl.patch_inverse(p, n)
                ref = np.linalg.inv(Ap)
                assert np.abs(X - ref).max() <= 1e-8 * np.abs(ref).max(), (L.level, p)
            assert ncorr > 0
    finally:
        s.close()
