"""2-D Scott-Vogelius [P3]^2-P2dg on the barycentric hierarchy (the k = 3 lines of the reference's iters2dsv target,
examples/Makefile:13, 16; alfi/solver.py:625-630), host side: the cubic triangle -- the first element here with a node in
the CELL interior -- through element, space, patches, transfer, injection, pressure coupling, Burman tables, rank-local
pieces and the gamma-robustness experiment on the oracle.  Tolerances are those of the tests named in each docstring.
No GPU."""
import hashlib
from fractions import Fraction

import numpy as np
import pytest

from alfi_amd import _hostlib, sv
from alfi_amd.elements import NodalElement
from alfi_amd.fespace import VectorFunctionSpace
from oracle import alfi_oracle as O
from oracle import exact_pins as X
from tests import exact_cases as C
from tests.sv_p3_2d_cases import PROBLEMS, hierarchy
from tests.test_exact_pins import SIMPLEX, _match, _one_cell_space

ARGS = (2, 3, False)


def test_element_nodes_entities_and_refusals():
    el = NodalElement(*ARGS)
    assert el.nloc == 10 and el.entity_nodes[-1] == (2, 0, 0) and el.nodes_per_edge == 2
    assert [e[0] for e in el.entity_nodes] == [0] * 3 + [1] * 6 + [2]
    assert el.has_cell_nodes and el.has_edge_nodes and not el.has_face_nodes
    assert np.allclose(el.node_bary[-1], 1.0 / 3.0)
    for args in ((2, 2, False), (3, 2, True), (3, 3, False), (3, 1, True)):
        assert not NodalElement(*args).has_cell_nodes
    assert NodalElement(3, 3, False).has_face_nodes
    with pytest.raises(AssertionError):
        NodalElement(2, 3, True)
    # the Hessian (central differences of the quadratic first derivatives) against a finer difference of the gradient
    lam = np.random.default_rng(0).dirichlet(np.ones(3), size=4)
    H = el.tabulate_hessian(lam)
    assert H.shape == (4, 10, 3, 3) and np.abs(H - H.transpose(0, 1, 3, 2)).max() < 1e-12
    T = el.reference_tensors()
    assert T["M"].shape == (10, 10) and abs(T["M"].sum() - 1.0) < 1e-14        # partition of unity, averages over the cell


def test_nodal_basis_and_gradients_match_the_exact_dual_basis():
    """tests/test_exact_pins.py::test_nodal_basis_and_gradients_match_the_exact_dual_basis for (2, "P3")."""
    el = NodalElement(*ARGS)
    nodes, basis = X.nodal_basis(2, "P3")
    assert el.nloc == len(nodes) == 10
    perm = _match(el.node_bary, nodes)
    lam = np.random.default_rng(1).dirichlet(np.ones(3), size=7)
    phi, dphi = el.tabulate(lam)
    grads, _ = X.barycentric_gradients(SIMPLEX[2])
    G = np.array([[float(x) for x in g] for g in grads])
    for a in range(el.nloc):
        b = basis[perm[a]]
        exact = np.array([float(X.p_eval(b, [Fraction(x).limit_denominator(10 ** 12) for x in l])) for l in lam])
        assert np.abs(phi[:, a] - exact).max() < 1e-10
        db = [X.p_diff(b, i) for i in range(3)]
        ge = np.array([[sum(float(X.p_eval(db[i], list(l))) * G[i, x] for i in range(3)) for x in range(2)] for l in lam])
        gp = np.einsum("pi,ix->px", dphi[:, a, :], G)
        assert np.abs(gp - ge).max() < 1e-9 * max(1.0, np.abs(ge).max())
    assert np.abs(el.tabulate(el.node_bary)[0] - np.eye(el.nloc)).max() < 1e-13


@pytest.mark.parametrize("ncell", [1, 2])
def test_element_matrices_are_exact(ncell):
    """nu K + gamma D + adv N(w) of the host assembler on one and two cells (test_state_dependent_terms_of_the_host_assembler_
    are_exact, 1e-12) and, on one cell, the oracle's quadrature assembly (test_element_matrix_of_the_velocity_form_is_exact)."""
    import scipy.sparse as sp
    mesh, V = C.build_space(2, ARGS, ncell)
    assert V.num_nodes == (10 if ncell == 1 else 16)
    nu, gamma, adv = Fraction(3, 70), Fraction(1250, 3), Fraction(3, 4)
    w = C.rational_field(2, V)
    wf = np.array([[float(x) for x in r] for r in w])
    rowptr, colidx = _hostlib.node_graph(V.cell_nodes, V.num_nodes)
    g, vol = mesh.cell_geometry()
    for a_ in (adv, Fraction(0)):
        exact = C.exact_operator(2, "P3", ncell, V, nu, gamma, a_, w)
        vals = _hostlib.assemble_bsr(V.cell_nodes, g, vol, V.element.reference_tensors(), 2, rowptr, colidx, nu=float(nu),
                                     gamma=float(gamma), adv=float(a_), wind=wf if a_ else None)
        prod = sp.bsr_matrix((vals, colidx, rowptr), shape=(V.num_nodes * 2,) * 2).toarray()
        assert np.abs(prod - exact).max() < 1e-12 * np.abs(exact).max()
    orc = O.assemble_form(V, nu=float(nu), gamma=float(gamma)).toarray()
    assert np.abs(orc - exact).max() < 1e-12 * np.abs(exact).max()


def test_scott_vogelius_matrices_are_exact():
    """tests/test_exact_pins.py::test_scott_vogelius_matrices_are_exact for (2, "P3", "P2"): the full grad-div block, the
    discrete divergence against P2dg (6 rows per cell) and the 6 x 6 mass block."""
    import scipy.sparse as sp
    nu, gamma = Fraction(3, 7), Fraction(1250, 3)
    mesh, V = _one_cell_space(2, ARGS)
    el, d, n = V.element, 2, 10
    nodes, pnodes, A, B, M = X.sv_matrices(2, "P3", "P2", SIMPLEX[2], nu, gamma)
    perm = _match(el.node_bary, nodes)
    cn = V.cell_nodes[0]
    exact = np.zeros((n * d, n * d))
    for a in range(n):
        for b in range(n):
            for c in range(d):
                for e in range(d):
                    exact[cn[a] * d + c, cn[b] * d + e] = float(A[perm[a]][c][perm[b]][e])
    rowptr, colidx = _hostlib.node_graph(V.cell_nodes, V.num_nodes)
    g, vol = mesh.cell_geometry()
    vals = _hostlib.assemble_bsr(V.cell_nodes, g, vol, el.reference_tensors(), d, rowptr, colidx, nu=float(nu), gamma=0.0,
                                 gamma_full=float(gamma))
    prod = sp.bsr_matrix((vals, colidx, rowptr), shape=(n * d, n * d)).toarray()
    assert np.abs(prod - exact).max() < 1e-12 * np.abs(exact).max()

    class _L(object):
        pass
    L = _L()
    L.V = V
    Bp, Mp, Mip = sv.build_sv_pressure_coupling(L, zero_bc_columns=False)
    pperm = _match(NodalElement(2, 2, False).node_bary, pnodes)
    m = len(pnodes)
    assert m == 6 and Bp.shape == (6, 20)
    Bex = np.zeros((m, n * d))
    for j in range(m):
        for a in range(n):
            for x in range(d):
                Bex[j, cn[a] * d + x] = float(B[pperm[j]][perm[a]][x])
    Mex = np.array([[float(M[pperm[j]][pperm[l]]) for l in range(m)] for j in range(m)])
    assert np.abs(Bp.toarray() - Bex).max() < 1e-12 * np.abs(Bex).max()
    assert np.abs(Mp.toarray() - Mex).max() < 1e-13 * np.abs(Mex).max()
    assert np.abs(Mip.toarray() @ Mex - np.eye(m)).max() < 1e-10


def test_space_has_one_node_per_cell():
    lv, _ = hierarchy("ldc2d", 2, 0, 100.0, False)
    for L in lv:
        V, m = L.V, L.V.mesh
        assert V.num_nodes == m.num_vertices + 2 * m.num_edges + m.num_cells
        cin = V.cell_interior_nodes
        assert cin.shape == (m.num_cells,) and np.array_equal(V.cell_nodes[:, -1], cin)
        assert np.abs(V.node_coords[cin] - m.coords[m.cells].mean(axis=1)).max() < 1e-14
        assert not V.bc_node_mask[cin].any() and V.face_nodes is None
        groups = np.concatenate([V.vertex_nodes, np.asarray(V.edge_nodes).ravel(), cin])
        assert np.array_equal(np.sort(groups), np.arange(V.num_nodes))           # one Morton order through all four groups
        assert not np.array_equal(np.sort(cin), np.arange(V.num_nodes - m.num_cells, V.num_nodes))
        # every node of a cell sits where the element says
        x = np.einsum("ai,civ->cav", V.element.node_bary, m.coords[m.cells])
        assert np.abs(V.node_coords[V.cell_nodes] - x).max() < 1e-13


def test_vertex_star_patches_hold_the_cell_nodes():
    """star_patches of a space with cell nodes: the cells around the seed bring their interior node (never dropped)."""
    V = hierarchy("ldc2d", 1, 0, 100.0, False)[0][1].V
    ptr, dofs, seeds = V.star_patches()
    m = V.mesh
    for p, v in enumerate(seeds):
        nodes = set((dofs[ptr[p]:ptr[p + 1]:2] // 2).tolist())
        cells = np.flatnonzero((m.cells == v).any(axis=1))
        assert set(V.cell_interior_nodes[cells].tolist()) <= nodes
        assert len(nodes) == (0 if V.bc_node_mask[V.vertex_nodes[v]] else 1) + len(cells) + 2 * np.count_nonzero(
            ((m.edges == v).any(axis=1)) & ~V.bc_node_mask[np.asarray(V.edge_nodes)[:, 0]])


def test_existing_spaces_are_unchanged():
    """cell_nodes, node_coords and bc_nodes of [P2]^2, [P2+FB]^3 and [P3]^3: SHA-256 of the arrays the parent revision
    (without the fourth node group) produced on these meshes."""
    from alfi_amd.mesh import bary_refine, box_mesh, rectangle_mesh, refine

    def h(V):
        m = hashlib.sha256()
        for a in (V.cell_nodes, V.node_coords, V.bc_nodes):
            m.update(np.ascontiguousarray(a).tobytes())
        return m.hexdigest()[:16]
    m2 = bary_refine(refine(rectangle_mesh(3, 2, 2.0, 1.0, "left")))
    m3 = refine(box_mesh(2, 1, 2, 1.0, 1.0, 1.0))
    assert h(VectorFunctionSpace(m2, NodalElement(2, 2, False))) == "754ffc9f08155f72"
    assert h(VectorFunctionSpace(m3, NodalElement(3, 2, True))) == "5149e2cb2ddeb8e4"
    V = VectorFunctionSpace(bary_refine(m3), NodalElement(3, 3, False))
    assert h(V) == "8b99c0a93aa942b8" and V.cell_interior_nodes is None and len(V.raw_offsets) == 5


def test_generator_against_quadrature_and_polynomials():
    """tests/test_sv.py::test_sv_generator_against_quadrature_and_polynomials for k = 3 (1e-11 operator, 1e-12 blocks, 1e-12
    prolongation / injection of a cubic field, the divergence bound of test_sv_p3_generator_3d)."""
    lv, tr = hierarchy("ldc2d", 2, 0, 100.0, False)
    assert [L.n for L in lv] == [242, 914, 3554]
    assert all(np.diff(L.patch_ptr).max() == 146 for L in lv[1:])
    assert tr[0].blk_dofs.shape == (8, 92) and tr[1].blk_dofs.shape == (32, 92)
    for L, T in zip(lv[1:], tr):
        assert len(np.unique(T.blk_dofs)) == T.blk_dofs.size
        assert len(np.unique(T.blk_dofs)) + len(T.skeleton_dofs) == L.n
        assert np.intersect1d(T.blk_dofs.ravel(), T.skeleton_dofs).size == 0
        # a fine cell node is interior to its coarse macro cell, never skeleton
        cin = L.V.cell_interior_nodes
        assert not sv.macro_skeleton_mask(L.V)[cin].any() and np.isin(cin * 2, T.blk_dofs).all()
        free = np.ones(L.n, dtype=bool)
        free[L.bc_dofs] = False
        hit = np.zeros(L.n, dtype=bool)
        hit[L.patch_dofs] = True
        assert np.array_equal(hit, free)                  # every non-Dirichlet dof, cell nodes included, lies in a patch
    L, T = lv[1], tr[0]
    A = O.apply_bcs_matrix(O.assemble_form(L.V, nu=L.nu, gamma_full=100.0), L.bc_dofs)
    assert abs(A - L.A.to_scipy()).max() < 1e-11
    Ks, Ds = O.assemble_form(L.V, nu=1.0).tocsr(), O.assemble_form(L.V, gamma_full=1.0).tocsr()
    for b in (0, 5):
        d = T.blk_dofs[b]
        assert np.abs(Ks[d][:, d].toarray() - T.K_II[b]).max() < 1e-12
        assert np.abs(Ds[d][:, d].toarray() - T.D_II[b]).max() < 1e-12
    assert abs(Ds[T.blk_dofs.ravel()] - T.D_I.to_scipy()).max() < 1e-12

    def f(X_):
        return np.stack([X_[:, 0] ** 3 - X_[:, 1] * X_[:, 0], X_[:, 0] * X_[:, 1] ** 2 + 1.0], axis=1).ravel()
    P = T.P.to_scipy()
    assert np.abs(P @ f(lv[0].V.node_coords) - f(L.V.node_coords)).max() < 1e-12
    J = T.inject_matrix
    assert np.abs(J @ f(L.V.node_coords).reshape(-1, 2) - f(lv[0].V.node_coords).reshape(-1, 2)).max() < 1e-12
    assert np.abs(np.asarray(J.sum(axis=1)).ravel() - 1.0).max() < 1e-12
    ot = O.oracle_transfer(T, L, True).st
    Xc = lv[0].V.node_coords
    uc = np.stack([Xc[:, 1] ** 3, Xc[:, 0] ** 3], axis=1).ravel()             # div = 0, in P3
    uf = ot.prolong(uc)
    assert abs(uf @ (Ds @ uf)) < 1e-8 * (uf @ (Ks @ uf))


def test_nodal_prolongation_on_a_uniform_refinement_reproduces_cubics():
    """fespace.nodal_prolongation evaluates the cell node's row too (the pkp0 pair with k = 3 itself is out of scope)."""
    from alfi_amd.fespace import nodal_prolongation
    from alfi_amd.mesh import refine
    mesh, Vc = C.build_space(2, ARGS, 2)
    Vf = VectorFunctionSpace(refine(mesh), NodalElement(*ARGS))
    P = nodal_prolongation(Vc, Vf)

    def f(x):
        return x[:, 0] ** 3 - 2.0 * x[:, 0] * x[:, 1] ** 2 + x[:, 1]
    assert np.abs(P @ f(Vc.node_coords) - f(Vf.node_coords)).max() < 1e-12
    assert np.abs(np.asarray(P.sum(axis=1)).ravel() - 1.0).max() < 1e-12


def test_pressure_coupling():
    """tests/test_sv.py::test_sv_pressure_coupling for (2, 3)."""
    lv, _ = hierarchy("ldc2d", 1, 0, 1.0, False)
    L = lv[1]
    B, M, Minv = sv.build_sv_pressure_coupling(L, zero_bc_columns=False)
    assert B.shape == (L.V.mesh.num_cells * 6, L.n)
    assert abs((M @ Minv) - np.eye(M.shape[0])).max() < 1e-10
    D = O.assemble_form(L.V, gamma_full=1.0)
    assert abs(D - B.T @ Minv @ B).max() < 1e-10 * abs(D).max()
    flux = B.T @ np.ones(B.shape[0])
    interior = np.setdiff1d(np.arange(L.n), L.bc_dofs)
    assert abs(flux[interior]).max() < 1e-12


@pytest.mark.parametrize("mesh,nref,largest", [("ldc2d", 2, 146), ("unionjack", 1, 194)])
def test_vectorised_macro_stars_equal_the_literal_constructor(mesh, nref, largest):
    lv, _ = hierarchy(mesh, nref, 100.0, 1e4)
    for L in lv[1:]:
        a, b = sv.macro_star_patches(L.V), sv.macro_star_patches_fast(L.V)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert np.array_equal(L.patch_ptr, b[0]) and np.array_equal(L.patch_dofs, b[1])
        assert np.diff(a[0]).max() == largest
    if mesh == "unionjack":
        assert [L.n for L in lv] == [242, 914]
        assert lv[1].patch_seeds[np.argmax(np.diff(lv[1].patch_ptr))] == 4           # the 8-valent centre


def test_macro_cell_groups_give_an_exact_block_factorisation():
    """The algebra of tests/test_sv.py::test_macro_cell_groups_give_an_exact_block_factorisation (1e-8) on the [P3]^2 macro
    stars: groups of 20 dofs (barycentre vertex, 3 x 2 interior-edge nodes, 3 cell nodes of a macro cell).  The 20 interior
    dofs of a cubic macro cell hold divergence-free functions, so cond(A_gg) ~ gamma / nu = 1.8e6 (28 for [P2]^2): X_g is
    applied by LU solves here.  With the explicit np.linalg.inv(A_gg) of the [P2] test the products lose cond(A_gg) eps |A_gS|
    and the same algebra ends at 2.7e-6 -- which is why the device refines W_g (kernels_bigpatch.hip: cond_group_body)."""
    lv, _ = hierarchy("ldc2d", 2, 100.0, 1e4)
    L = lv[-1]
    A = L.A.to_scipy().tocsr()
    rng = np.random.default_rng(0)
    sizes, empty_skeleton = set(), 0
    for p in range(len(L.patch_ptr) - 1):
        sl = slice(L.patch_ptr[p], L.patch_ptr[p + 1])
        dofs, lab = L.patch_dofs[sl], L.patch_groups[sl]
        Ap = A[dofs][:, dofs].toarray()
        n = len(dofs)
        S = np.flatnonzero(lab < 0)
        groups = [np.flatnonzero(lab == g) for g in np.unique(lab[lab >= 0])]
        assert len(groups) > 0                    # (a corner's single macro cell: all of its skeleton is Dirichlet, S empty)
        sizes |= set(len(g) for g in groups)
        empty_skeleton += len(S) == 0
        for i, gi in enumerate(groups):
            for gj in groups[i + 1:]:
                assert not Ap[np.ix_(gi, gj)].any() and not Ap[np.ix_(gj, gi)].any()
        x = rng.standard_normal(n)
        Sigma = Ap[np.ix_(S, S)].copy()
        rhs = x[S].copy()
        t, W = {}, {}
        for k, g in enumerate(groups):
            Agg = Ap[np.ix_(g, g)]
            W[k] = np.linalg.solve(Agg, Ap[np.ix_(g, S)])
            t[k] = np.linalg.solve(Agg, x[g])
            Sigma -= Ap[np.ix_(S, g)] @ W[k]
            rhs -= Ap[np.ix_(S, g)] @ t[k]
        y = np.zeros(n)
        y[S] = np.linalg.solve(Sigma, rhs)
        for k, g in enumerate(groups):
            y[g] = t[k] - W[k] @ y[S]
        ref = np.linalg.solve(Ap, x)
        assert np.abs(y - ref).max() < 1e-8 * np.abs(ref).max()
    assert sizes == {20} and empty_skeleton < len(L.patch_ptr) - 1
    # the cell nodes carry their macro cell's label
    lab = sv.macro_cell_groups(L.V, np.arange(L.n))
    cin = L.V.cell_interior_nodes
    assert np.array_equal(lab[cin * 2], np.arange(L.V.mesh.num_cells) // 3)


def test_burman_host_pass_against_restatement():
    """tests/test_burman.py::test_residual_and_jacobian_against_restatement / test_polynomial_velocity_has_no_burman_residual /
    test_facet_table_geometry / test_pcpatch_facet_rule for k = 3, dim = 2: 16-node facet unions, rules of 3 and 5 points."""
    import copy
    from alfi_amd.burman import HostBurman, patch_cells, patch_facet_corrections
    from alfi_amd.problem import BSR
    from tests import burman_restatement as RS
    lv, _ = hierarchy("ldc2d", 1, 10.0, 1e4, True, True)
    L = lv[1]
    V, d, t = L.V, 2, L.facets
    assert t.nu == 16 and t.nloc == 10 and t.J.shape[1:] == (3, 16) and len(t.wn) == 5
    hb = HostBurman(L)
    U = np.random.default_rng(0).standard_normal((V.num_nodes, d))
    w = 5e-3
    F = np.zeros(L.n)
    vals = np.zeros((L.A.colidx.shape[0], d, d))
    beta = np.empty(t.nf)
    hb(U, w, vals, F, beta)
    Fo = RS.residual(V, U, w)
    assert np.abs(F - Fo).max() < 1e-12 * np.abs(Fo).max()
    J = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx, vals).to_scipy()
    for seed in range(2):
        v = np.random.default_rng(10 + seed).standard_normal(L.n).reshape(-1, d)
        eps = 1e-6
        fd = (RS.residual(V, U + eps * v, w) - RS.residual(V, U - eps * v, w)) / (2 * eps)
        assert np.abs(J @ v.ravel() - fd).max() < 1e-6 * np.abs(fd).max()
    # a cubic velocity has no jumps
    x = V.node_coords
    rng = np.random.default_rng(1)
    Up = np.zeros((V.num_nodes, d))
    for i in range(d):
        c = rng.standard_normal((d, 4))
        Up[:, i] = sum((c[j, p] * x[:, j] ** p) for j in range(d) for p in range(4)) + x[:, 0] * x[:, 1] * c[0, 0]
    Fp = np.zeros(L.n)
    hb(Up, w, F=Fp)
    assert np.abs(Fp).max() < 1e-12 * max(1.0, np.abs(F).max()) * np.abs(Up).max()
    # PCPATCH's facet rule on the macro stars
    Ball = J.tocsr()
    ptr, col, fac, s = patch_facet_corrections(V, t, L.patch_ptr, L.patch_dofs)
    npatch = len(L.patch_ptr) - 1
    for p in sorted(set([0, npatch // 3, npatch // 2, npatch - 1])):
        dofs = L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]]
        nodes = dofs[::d] // d
        inside = np.zeros(V.mesh.num_cells, dtype=bool)
        inside[patch_cells(V, nodes)] = True
        both = inside[t.cells[:, 0]] & inside[t.cells[:, 1]]
        sub = copy.copy(t)
        sub.coef = np.where(both, t.coef, 0.0)
        vin = np.zeros_like(vals)
        HostBurman(L, sub)(U, w, vals=vin)
        Bin = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx, vin).to_scipy().tocsr()[dofs][:, dofs].toarray()
        Cm = np.zeros((nodes.size * d, nodes.size * d))
        r0 = L.patch_ptr[p] // d
        for i in range(nodes.size):
            for q in range(ptr[r0 + i], ptr[r0 + i + 1]):
                for c in range(d):
                    Cm[i * d + c, col[q] * d + c] += w * beta[fac[q]] * s[q]
        Bp = Ball[dofs][:, dofs].toarray()
        assert np.abs(Bp - Cm - Bin).max() <= 1e-13 * np.abs(Bp).max()


def test_rank_local_pieces():
    """alfi_amd.dist on the new space: a rank's Burman host pass equals the global rows bit for bit
    (tests/test_dist_burman.py::test_rank_host_pass_equals_global_rows), and lazy.LazyOperator gives the rows of the assembled
    operator (tests/test_lazy.py::test_lazy_operator_with_the_full_grad_div_term, 1e-13)."""
    from alfi_amd.dist import FacetPart, assembly_cells, build_parts, choose_splits, localize
    from alfi_amd.lazy import LazyOperator
    levels, transfers = hierarchy("ldc2d", 1, 0.0, 1e4, True, True)
    world = 2
    splits = choose_splits(levels, world, min_dofs=1)
    seen = set()
    for rank in range(world):
        parts = build_parts(levels, transfers, splits, rank, exchange_lists=None)
        llev, _, _ = localize(levels, transfers, parts)
        for LL in llev:
            if LL.part.nb_own == 0:
                continue
            L, part = levels[LL.level], LL.part
            d, n = 2, L.V.num_nodes
            U = np.random.default_rng(LL.level + 10 * rank).standard_normal((n, d))
            gvals, gF, gbeta = np.zeros((L.A.colidx.size, d, d)), np.zeros(n * d), np.empty(L.facets.nf)
            _hostlib.burman(L.facets, U, 3.5e-3, L.facets.contributors(L.A.rowptr, L.A.colidx, n), vals=gvals, F=gF, beta=gbeta)
            fp = FacetPart(L.V, L.facets, part)
            lvals, lF, lbeta = np.zeros((LL.A.colidx.size, d, d)), np.zeros(part.nb_loc * d), np.empty(fp.table.nf)
            fp.host(LL.A, U[fp.state_nodes], 3.5e-3, vals=lvals, F=lF, beta=lbeta)
            gkey = np.repeat(np.arange(n, dtype=np.int64), np.diff(L.A.rowptr)) * n + L.A.colidx
            idx = np.searchsorted(gkey, np.repeat(part.nodes, np.diff(LL.A.rowptr)).astype(np.int64) * n + part.nodes[LL.A.colidx])
            assert np.array_equal(lvals, gvals[idx]) and np.array_equal(lF.reshape(-1, d), gF.reshape(-1, d)[part.nodes])
            assert np.array_equal(lbeta, gbeta[fp.facets]) and np.abs(lvals).max() > 0.0
            cells, cn, state = assembly_cells(L.V, part)
            assert np.array_equal(state[cn], L.V.cell_nodes[cells])
            seen.add(rank)
    assert seen == {0, 1}
    lv, _ = hierarchy("ldc2d", 1, 50.0, 1e4)
    L = lv[-1]
    V = L.V
    wind = PROBLEMS["ldc2d"]().driver(V.node_coords)
    op = LazyOperator(V, L.A.rowptr, L.A.colidx, V.mesh.cell_geometry(), V.element.reference_tensors(), L.nu, L.gamma, 1.0,
                      np.ascontiguousarray(wind), full_div=True)
    rows = np.arange(1, V.num_nodes, 3)
    a, b = op.select_rows(rows), L.A.select_rows(rows)
    assert np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.colidx, b.colidx)
    assert np.abs(a.vals - b.vals).max() <= 1e-13 * np.abs(b.vals).max()


def test_front_end_refusals():
    from alfi_amd.sv import build_sv_hierarchy
    for k in (1, 4):
        with pytest.raises(NotImplementedError, match=r"\[P3\]\^d"):
            build_sv_hierarchy(PROBLEMS["ldc2d"](), 1, k, Re=10.0)


def test_gamma_robustness_on_the_oracle():
    """tests/test_sv.py::test_sv_gamma_robustness with [P3]^2: FGMRES + one V-cycle (3 smoothing steps, robust restriction) on
    the oracle, gamma in {0, 1e2, 1e4, 1e6}.  The counts of the deterministic CPU oracle are 4 / 6 / 6 / 6 (CHANGELOG.md)."""
    from alfi_amd.sv import build_sv_hierarchy
    from tests.test_graddiv import fgmres_solve
    its = {}
    for gamma in (0.0, 1e2, 1e4, 1e6):
        lv, tr = build_sv_hierarchy(PROBLEMS["ldc2d"](), 2, 3, Re=0, gamma=gamma, advect=False)
        mg = O.build_oracle_mg(lv, tr, k=3, schoeberl_restriction=True)
        A = mg.levels[-1]["A"]
        b = np.ones(A.shape[0])
        b[lv[-1].bc_dofs] = 0
        its[gamma] = fgmres_solve(A, lambda r: mg.vcycle(len(lv) - 1, r, np.zeros_like(r)), b)
    print("gamma-robustness [P3]^2:", its)
    assert its[1e6] - its[1e2] <= 2, its
    assert its == {0.0: 4, 1e2: 6, 1e4: 6, 1e6: 6}, its
