"""Burman interior-penalty stabilisation of the Scott-Vogelius pair (alfi/stabilisation.py:139-162, alfi/solver.py:226-234),
host side: the facet tables and the C++ pass (alfi_host_burman) against the independent restatement in
tests/burman_restatement.py, the facet-coupled sparsity, and the solver's refusals.  No GPU."""
import numpy as np
import pytest

from alfi_amd import _hostlib
from alfi_amd.burman import HostBurman, FacetTable
from alfi_amd.problem import BSR, TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem
from alfi_amd.sv import build_sv_hierarchy

from tests import burman_restatement as RS

CASES = [pytest.param(lambda: TwoDimLidDrivenCavityProblem(2), 2, id="2d-P2"),
         pytest.param(lambda: ThreeDimLidDrivenCavityProblem(1), 3, id="3d-P3")]


def _level(mk, k, nref=1, **kw):
    lv, tr = build_sv_hierarchy(mk(), nref, k, Re=10.0, patches=False, facet_coupling=True, **kw)
    return lv, tr


@pytest.mark.parametrize("mk,k", CASES)
def test_residual_and_jacobian_against_restatement(mk, k):
    lv, _ = _level(mk, k)
    L = lv[1]
    V, d = L.V, L.bs
    hb = HostBurman(L)
    U = np.random.default_rng(0).standard_normal((V.num_nodes, d))
    w = 5e-3
    F = np.zeros(L.n)
    vals = np.zeros((L.A.colidx.shape[0], d, d))
    hb(U, w, vals, F)
    Fo = RS.residual(V, U, w)
    assert np.abs(F - Fo).max() < 1e-12 * np.abs(Fo).max()
    J = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx, vals).to_scipy()
    for seed in range(2):
        v = np.random.default_rng(10 + seed).standard_normal(L.n).reshape(-1, d)
        eps = 1e-6
        fd = (RS.residual(V, U + eps * v, w) - RS.residual(V, U - eps * v, w)) / (2 * eps)
        assert np.abs(J @ v.ravel() - fd).max() < 1e-6 * np.abs(fd).max()
    # a second pass gives the same bits
    Fz = np.zeros(L.n)
    Js = np.zeros_like(vals)
    hb(U, w, Js, Fz)
    assert np.array_equal(Js, vals) and np.array_equal(Fz, F)


@pytest.mark.parametrize("mk,k", CASES)
def test_polynomial_velocity_has_no_burman_residual(mk, k):
    lv, _ = _level(mk, k)
    L = lv[1]
    V, d = L.V, L.bs
    x = V.node_coords
    rng = np.random.default_rng(1)
    U = np.zeros((V.num_nodes, d))
    for i in range(d):                                                  # a random polynomial of degree k per component
        c = rng.standard_normal((d, k + 1))
        U[:, i] = sum((c[j, p] * x[:, j] ** p) for j in range(d) for p in range(k + 1)) + x[:, 0] * x[:, d - 1] * c[0, 0]
    F = np.zeros(L.n)
    HostBurman(L)(U, 5e-3, F=F)
    Fr = np.zeros(L.n)
    HostBurman(L)(rng.standard_normal(U.shape), 5e-3, F=Fr)
    assert np.abs(F).max() < 1e-12 * max(1.0, np.abs(Fr).max()) * np.abs(U).max()


def test_hand_pin_kink_along_a_grid_line():
    """u = max(0, x - x0) e_1 with x0 a grid line of the base mesh: the P2 interpolant is exact cell by cell, jump(grad u, n)
    is e_1 (up to sign) on the facets of x = x0 and zero elsewhere, so u . R_B(u) = sum c_F beta_F |F| over those facets,
    beta_F = |F|^-1 int_F sqrt(0 + 1e-10) = 1e-5."""
    lv, _ = _level(lambda: TwoDimLidDrivenCavityProblem(2), 2)
    L = lv[1]
    V = L.V
    x0, w = 0.5, 5e-3
    U = np.zeros((V.num_nodes, 2))
    U[:, 0] = np.maximum(0.0, V.node_coords[:, 0] - x0)
    F = np.zeros(L.n)
    HostBurman(L)(U, w, F=F)
    mesh = V.mesh
    fx = mesh.coords[mesh.facets][:, :, 0]
    on = np.flatnonzero(np.all(np.abs(fx - x0) < 1e-14, axis=1))
    t = L.facets
    sel = np.isin(t.facet_ids, on)
    assert sel.sum() == 4                                               # the 4 x 4 level-1 mesh: four edges on x = 0.5
    area = t.area[sel]
    expect = np.sum(0.5 * w * area ** 2 * 1e-5 * area)
    assert abs(U.ravel() @ F - expect) < 1e-9 * expect


@pytest.mark.parametrize("mk,k", CASES)
def test_facet_coupled_graph(mk, k):
    prob = mk()
    lv0, tr0 = build_sv_hierarchy(prob, 1, k, Re=10.0, patches=True)
    lvo, tro = build_sv_hierarchy(mk(), 1, k, Re=10.0, patches=True, facet_coupling=False)
    lv1, tr1 = build_sv_hierarchy(mk(), 1, k, Re=10.0, patches=True, facet_coupling=True)
    for a, b, c in zip(lv0, lvo, lv1):
        # off: bit for bit the hierarchy without the keyword
        assert np.array_equal(a.A.rowptr, b.A.rowptr) and np.array_equal(a.A.colidx, b.A.colidx)
        assert np.array_equal(a.A.vals, b.A.vals)
        # on: the cell graph united with the facet-pair blocks
        V = c.V
        n = V.num_nodes
        rc, cc = _hostlib.node_graph(V.cell_nodes, n)
        keys = set((np.repeat(np.arange(n), np.diff(rc)) * n + cc).tolist())
        r, col = FacetTable(V).pairs()
        keys |= set((r * n + col).tolist())
        got = np.repeat(np.arange(n), np.diff(c.A.rowptr)) * n + c.A.colidx
        assert sorted(keys) == got.tolist()
        assert c.A.colidx.shape[0] > a.A.colidx.shape[0]
        # the cell operator itself is unchanged on the cell blocks, zero on the facet-only blocks
        Ac, Ab = a.A.to_scipy(), c.A.to_scipy()
        assert abs(Ab - Ac).max() == 0.0
        if c.level > 0:
            assert getattr(c, "patch_groups", None) is None and getattr(a, "patch_groups", None) is not None
    # transfers: built from the cell graph, bitwise the same
    for A, B in zip(tr0, tr1):
        for name in ("P", "D_I"):
            pa, pb = getattr(A, name), getattr(B, name)
            assert np.array_equal(pa.rowptr, pb.rowptr) and np.array_equal(pa.colidx, pb.colidx)
            assert np.array_equal(pa.vals, pb.vals)
        assert np.array_equal(A.K_II, B.K_II) and np.array_equal(A.D_II, B.D_II)


def test_facet_table_geometry():
    lv, _ = _level(lambda: ThreeDimLidDrivenCavityProblem(1), 3)
    t = lv[1].facets
    assert t.nu == 30 and t.J.shape[1:] == (9, 30) and len(t.wn) == 25
    assert np.allclose(np.linalg.norm(t.normal, axis=1), 1.0)
    # the normal points from K+ into K-
    mesh = lv[1].V.mesh
    cen = mesh.coords[mesh.cells].mean(axis=1)
    assert (np.einsum("fx,fx->f", cen[t.cells[:, 1]] - cen[t.cells[:, 0]], t.normal) > 0).all()
    # sum of |F| over the interior facets from the facet vertices
    X = mesh.coords[mesh.facets[t.facet_ids]]
    area = 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)
    assert np.allclose(t.area, area, rtol=1e-13)
    lv2, _ = _level(lambda: TwoDimLidDrivenCavityProblem(2), 2)
    assert lv2[1].facets.nu == 9


def test_refusals():
    from alfi_amd.nssolver import HipNavierStokesSolver
    with pytest.raises(NotImplementedError):
        HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 1, 2, discretisation="pkp0", stabilisation_type="burman")
    with pytest.raises(NotImplementedError):
        HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 1, 2, discretisation="sv", stabilisation_type="gls")

    # (burman on partitioned levels is built, alfi_amd.dist_nssolver: the hook that refused it is gone)
    assert not hasattr(HipNavierStokesSolver, "_partitioned_burman")
    # multiplicative patch sweeps on a facet-coupled level: refused before any device object exists
    from alfi_amd.solver import HipPatchPC
    lv, _ = _level(lambda: TwoDimLidDrivenCavityProblem(2), 2)

    class PC(object):
        options = {"patch_pc_patch_local_type": "multiplicative"}
        level_data = lv[1]
        ctx = None

        def getOptionsPrefix(self):
            return ""
    with pytest.raises(NotImplementedError, match="multiplicative"):
        HipPatchPC().initialize(PC())


@pytest.mark.parametrize("mk,k", CASES)
def test_pcpatch_facet_rule(mk, k):
    """The patch matrix PCPATCH assembles -- cell terms of the patch's cells, facet terms of the facets with BOTH cells in the
    patch -- equals the global sub-block minus the K-side terms listed by burman.patch_facet_corrections (scaled by beta_F)."""
    import copy
    from alfi_amd.burman import patch_cells, patch_facet_corrections
    lv, _ = build_sv_hierarchy(mk(), 1, k, Re=10.0, patches=True, facet_coupling=True)
    L = lv[1]
    V, d, t = L.V, L.bs, L.facets
    U = np.random.default_rng(2).standard_normal((V.num_nodes, d))
    w = 5e-3
    vals = np.zeros((L.A.colidx.shape[0], d, d))
    beta = np.empty(t.nf)
    HostBurman(L)(U, w, vals=vals, beta=beta)
    Ball = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx, vals).to_scipy().tocsr()
    ptr, col, fac, s = patch_facet_corrections(V, t, L.patch_ptr, L.patch_dofs)
    npatch = len(L.patch_ptr) - 1
    for p in sorted(set([0, npatch // 3, npatch // 2, npatch - 1])):
        dofs = L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]]
        nodes = dofs[::d] // d
        inside = np.zeros(V.mesh.num_cells, dtype=bool)
        inside[patch_cells(V, nodes)] = True
        both = inside[t.cells[:, 0]] & inside[t.cells[:, 1]]
        sub = copy.copy(t)
        sub.coef = np.where(both, t.coef, 0.0)            # the facet terms of the patch's own facets only
        vin = np.zeros_like(vals)
        HostBurman(L, sub)(U, w, vals=vin)
        Bin = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx, vin).to_scipy().tocsr()[dofs][:, dofs].toarray()
        C = np.zeros((nodes.size * d, nodes.size * d))
        r0 = L.patch_ptr[p] // d
        for i in range(nodes.size):
            for q in range(ptr[r0 + i], ptr[r0 + i + 1]):
                for c in range(d):
                    C[i * d + c, col[q] * d + c] += w * beta[fac[q]] * s[q]
        assert np.abs(C).max() > 0.0 or not (inside[t.cells[:, 0]] ^ inside[t.cells[:, 1]]).any()
        Bp = Ball[dofs][:, dofs].toarray()
        assert np.abs(Bp - C - Bin).max() <= 1e-13 * np.abs(Bp).max()
