"""The Chebyshev smoother, point Jacobi, the W-cycle and the device CG -- the solver of the reference's grad-div experiment
(examples/graddiv/graddiv.py:85-135) -- on the GPU against the NumPy restatement (tests/chebyshev_restatement.py, pinned by
tests/test_chebyshev.py).  -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd.problem import BSR
from tests import chebyshev_restatement as R

# patch apply / smoother parity against the oracle: 1e-7 relative to the max-norm, the tolerance of
# tests/test_gpu_parity.py::test_fgmres_smoother (two independent inversions of patch operators of condition ~1e7)
SMOOTHER_TOL = 1e-7


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ctx():
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_mg(ctx):
    """(case, gamma) -> hip.Multigrid with k = 2 and the Schoeberl transfer both ways, built once per module."""
    from alfi_amd import hip
    made = {}

    def get(case, gamma):
        if (case, gamma) not in made:
            lv, tr = R.hierarchy(case, gamma)
            made[(case, gamma)] = hip.Multigrid(ctx, lv, tr, 2, robust_restriction=True)
        return made[(case, gamma)]
    yield get
    for m in made.values():
        m.close()


def seeded(n, bc, seed):
    v = np.random.default_rng(seed).standard_normal(n)
    v[bc] = 0.0
    return v


# ---- 4. kernel shapes: Chebyshev around point Jacobi on small block-tridiagonal operators ------------------------------------
def tridiagonal(nodes, bs, layout, seed=0):
    """Block-tridiagonal SPD operator.  layout "flat": every block row is non-empty, which the library stores lane-major;
    "plain": one more, EMPTY block row (its dofs are Dirichlet dofs) -- such an operator keeps the host layout."""
    rng = np.random.default_rng(seed)
    rowptr, colidx, vals = [0], [], []
    for i in range(nodes):
        for j in (i - 1, i, i + 1):
            if 0 <= j < nodes:
                colidx.append(j)
                if j == i:
                    S = 0.2 * rng.standard_normal((bs, bs))
                    vals.append((3.0 + i % 3) * np.eye(bs) + 0.5 * (S + S.T))
                else:
                    lo, hi = min(i, j), max(i, j)
                    C = 0.4 * np.random.default_rng(1000 * seed + lo).standard_normal((bs, bs)) - 0.5 * np.eye(bs)
                    vals.append(C if j > i else C.T)
                    assert hi == lo + 1
        rowptr.append(len(colidx))
    nb = nodes
    bc = np.zeros(0, dtype=np.int32)
    if layout == "plain":
        rowptr.append(len(colidx))
        nb = nodes + 1
        bc = np.arange(nodes * bs, nb * bs, dtype=np.int32)
    A = BSR(nb, nb, bs, np.asarray(rowptr, dtype=np.int32), np.asarray(colidx, dtype=np.int32), np.asarray(vals))
    return A, bc


@pytest.mark.parametrize("layout", ["flat", "plain"])
@pytest.mark.parametrize("bs,nodes", [(2, 1), (2, 32), (2, 33), (2, 129), (3, 1), (3, 21), (3, 22), (3, 85)])
def test_chebyshev_jacobi_kernel_shapes(ctx, bs, nodes, layout):
    """n = 2, 64, 66, 258 and 3, 63, 66, 255 (+ bs in the plain layout): one lane, one wave, the 16-byte tail, one workgroup.
    Pure FP64 vector arithmetic, only FMA contraction differs: 1e-12 max|x|."""
    from alfi_amd import hip
    A, bc = tridiagonal(nodes, bs, layout)
    As = A.to_scipy().tocsr()
    n = A.nbrows * bs
    diag = As.diagonal()
    jac = R.JacobiSmoother(As, bc)
    jac.diag = np.where(diag == 0.0, 1.0, diag)
    lvl = hip.Level(ctx, A, bc)
    lvl.set_jacobi(True)
    try:
        x0, b = np.random.default_rng(5).standard_normal(n), np.random.default_rng(6).standard_normal(n)
        dy = ctx.vec(n)
        lvl.patch_apply(ctx.vec(x0), dy)                       # the Jacobi apply itself
        ref = jac.apply(x0)
        assert np.abs(dy.get() - ref).max() <= 1e-14 * np.abs(ref).max()
        assert np.array_equal(dy.get()[bc], x0[bc])
        emin, emax = 0.15, 1.8
        for k in (1, 2, 5):
            for nonzero in (False, True):
                db, dx = ctx.vec(b), ctx.vec(x0)
                lvl.smooth_chebyshev(k, emin, emax, db, dx, nonzero_guess=nonzero)
                ref = R.chebyshev(As, jac.apply, b, x0, k, emin, emax, nonzero_guess=nonzero)
                err = np.abs(dx.get() - ref).max()
                assert err <= 1e-12 * np.abs(ref).max(), (k, nonzero, err)
    finally:
        lvl.close()


def test_unaligned_vectors_take_the_scalar_kernels(ctx):
    """b and x 8 bytes off a 16-byte boundary (views into larger buffers): the update and the Jacobi apply take their scalar
    branches, entry by entry the same arithmetic."""
    from alfi_amd import hip
    for bs, nodes in ((2, 33), (3, 85)):
        A, bc = tridiagonal(nodes, bs, "flat")
        As = A.to_scipy().tocsr()
        n = A.nbrows * bs
        jac = R.JacobiSmoother(As, bc)
        lvl = hip.Level(ctx, A, bc)
        lvl.set_jacobi(True)
        try:
            x0, b = np.random.default_rng(7).standard_normal(n), np.random.default_rng(8).standard_normal(n)
            big_b, big_x, big_y = ctx.vec(n + 1), ctx.vec(n + 1), ctx.vec(n + 1)
            db, dx, dy = hip.view(big_b, 1, n), hip.view(big_x, 1, n), hip.view(big_y, 1, n)
            assert db.ptr.value % 16 == 8 and dx.ptr.value % 16 == 8
            dx.set(x0)
            lvl.patch_apply(dx, dy)
            ref = jac.apply(x0)
            assert np.abs(dy.get() - ref).max() <= 1e-14 * np.abs(ref).max()
            for k in (1, 3):
                for nonzero in (False, True):
                    db.set(b)
                    dx.set(x0)
                    lvl.smooth_chebyshev(k, 0.15, 1.8, db, dx, nonzero_guess=nonzero)
                    ref = R.chebyshev(As, jac.apply, b, x0, k, 0.15, 1.8, nonzero_guess=nonzero)
                    assert np.abs(dx.get() - ref).max() <= 1e-12 * np.abs(ref).max(), (bs, k, nonzero)
            assert big_x.get()[0] == 0.0 and big_b.get()[0] == 0.0        # nothing written in front of the views
        finally:
            lvl.close()


def test_jacobi_diagonal_follows_the_operator_values_and_serves_the_fgmres_smoother(ctx):
    from alfi_amd import hip
    from oracle import alfi_oracle as O
    A, bc = tridiagonal(33, 3, "flat")
    As = A.to_scipy().tocsr()
    n = A.nbrows * 3
    lvl = hip.Level(ctx, A, bc)
    lvl.set_jacobi(True)
    try:
        x0, b = np.random.default_rng(9).standard_normal(n), np.random.default_rng(10).standard_normal(n)
        dx0, dy = ctx.vec(x0), ctx.vec(n)
        lvl.patch_apply(dx0, dy)
        assert np.abs(dy.get() - x0 / As.diagonal()).max() <= 1e-14 * np.abs(x0 / As.diagonal()).max()
        # FGMRES(3) over point Jacobi (the smoother's general path) against the oracle's FGMRES
        jac = R.JacobiSmoother(As, bc)
        for nonzero in (False, True):
            dx = ctx.vec(x0)
            lvl.smooth(3, ctx.vec(b), dx, nonzero_guess=nonzero)
            ref = O.fgmres(lambda v: As @ v, jac.apply, b, x0 if nonzero else np.zeros(n), 3, nonzero_guess=nonzero)
            assert relerr(dx.get(), ref) < 1e-10, nonzero
        # new operator values: the next apply divides by the NEW diagonal
        vals2 = np.asarray(A.vals).copy()
        vals2[:] *= 1.0 + 0.5 * np.random.default_rng(11).random(vals2.shape[0])[:, None, None]
        lvl.update_values(vals2)
        A2 = BSR(A.nbrows, A.nbcols, 3, A.rowptr, A.colidx, vals2).to_scipy().tocsr()
        assert np.abs(A2.diagonal() - As.diagonal()).max() > 0.1
        lvl.patch_apply(dx0, dy)
        ref = x0 / A2.diagonal()
        assert np.abs(dy.get() - ref).max() <= 1e-14 * np.abs(ref).max()
    finally:
        lvl.close()


def test_arnoldi_two_pass_projection_and_breakdown(ctx, device_mg):
    """m = 20 > 16 basis vectors: the multi-dot / multi-axpy kernels run in two passes; the largest Ritz value against the
    restatement's Arnoldi of the same length.  A 2-dof level: the Krylov space is exhausted after two steps, m_done = 2 < 5 and
    the columns from there on are zero."""
    from alfi_amd import hip
    lv, _ = R.hierarchy("2d", 1e4)
    rmg, dmg = R.multigrid("2d", 1e4), device_mg("2d", 1e4)
    L, ol, dl = lv[-1], rmg.levels[-1], dmg.levels[-1]
    v0 = R.seed_vector(L.n, L.bc_dofs)
    H, m = dl.arnoldi(20, ctx.vec(v0))
    Href = R.arnoldi(ol["A"], ol["smoother"].apply, v0, 20)
    lam, lam_ref = np.linalg.eigvals(H[:20, :20]).real.max(), np.linalg.eigvals(Href[:20, :20]).real.max()
    print("arnoldi 20 steps", lam, lam_ref, relerr(H, Href))
    assert m == 20 and abs(lam - lam_ref) <= 1e-6 * lam_ref
    assert relerr(H[:, :10], Href[:, :10]) < 1e-6
    A, bc = tridiagonal(1, 2, "flat")
    lvl = hip.Level(ctx, A, bc)
    lvl.set_jacobi(True)
    try:
        H, m = lvl.arnoldi(5, ctx.vec(np.array([1.0, 2.0])))
        assert m == 2 and not H[:, 2:].any() and H[1, 0] > 0
        MA = A.to_scipy().toarray() / A.to_scipy().toarray().diagonal()[:, None]
        assert np.allclose(np.sort(np.linalg.eigvals(H[:2, :2]).real), np.sort(np.linalg.eigvals(MA).real), rtol=1e-12)
    finally:
        lvl.close()


# ---- 5. smoother parity with the patch preconditioner ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["2d", "3d"])
def test_chebyshev_patch_smoother_matches_the_restatement(ctx, device_mg, case):
    lv, _ = R.hierarchy(case, 1e4)
    rmg, dmg = R.multigrid(case, 1e4), device_mg(case, 1e4)
    L, ol, dl = lv[-1], rmg.levels[-1], dmg.levels[-1]
    emin, emax = rmg.bounds[-1]
    b, x0 = seeded(L.n, L.bc_dofs, 4), seeded(L.n, L.bc_dofs, 5)
    for k in (1, 2, 3):
        for nonzero in (False, True):
            db, dx = ctx.vec(b), ctx.vec(x0)
            dl.smooth_chebyshev(k, emin, emax, db, dx, nonzero_guess=nonzero)
            ref = R.chebyshev(ol["A"], ol["smoother"].apply, b, x0, k, emin, emax, nonzero_guess=nonzero)
            err = relerr(dx.get(), ref)
            print("chebyshev parity", case, k, nonzero, err)
            assert err < SMOOTHER_TOL, (k, nonzero, err)


# ---- 6. Arnoldi and the interval -----------------------------------------------------------------------------------------------
# There is no project number for this tolerance: it is 10 x the largest relative difference between the device estimate and the
# restatement's lambda measured on an MI355X (the spread between boxes is unknown), and far below the 1e-6 beyond which the two
# would not be estimating the same thing.  Measured (levels 1 / 2 of the 2-D case, level 1 of the 3-D case): gamma = 0:
# 1.8e-15, 1.8e-15, 3.5e-15; gamma = 1e4: 6.5e-15, 3.4e-15, 2.0e-15.
BOUNDS_MEASURED = 6.5e-15
BOUNDS_TOL = 10 * BOUNDS_MEASURED


@pytest.mark.parametrize("case", ["2d", "3d"])
@pytest.mark.parametrize("gamma", [0.0, 1e4])
def test_chebyshev_bounds_match_the_restatement(ctx, device_mg, case, gamma):
    rmg, dmg = R.multigrid(case, gamma), device_mg(case, gamma)
    got = dmg.chebyshev_bounds()
    assert len(got) == len(rmg.levels) - 1
    for l, (emin, emax) in enumerate(got, start=1):
        lam = rmg.bounds[l][1] / 1.1
        diff = max(abs(emax / 1.1 - lam), abs(emin / 0.1 - lam)) / lam
        print("chebyshev bounds", case, gamma, "level", l, "lambda", lam, "relative difference", diff)
        assert diff <= BOUNDS_TOL, (case, gamma, l, diff)
    L = dmg.levels[-1]
    H, m = L.arnoldi(3, ctx.vec(R.seed_vector(L.n, R.hierarchy(case, gamma)[0][-1].bc_dofs)))
    assert m == 3 and H.shape == (4, 3) and H[2, 0] == 0.0 and H[3, 0] == 0.0 and H[3, 1] == 0.0 and (np.diag(H, -1) > 0).all()


# ---- 7. W-cycle --------------------------------------------------------------------------------------------------------------------
def cheb_cycle(ctx, dmg, rmg, b, cycle):
    dmg.set_smoother("chebyshev", rmg.bounds[1:])
    dmg.set_cycle_type(cycle)
    db, dx = ctx.vec(b), ctx.vec(b.shape[0])
    dmg.vcycle(db, dx)
    dmg.set_smoother("fgmres")
    dmg.set_cycle_type("v")
    return dx.get()


def test_w_cycle_matches_the_restatement_on_three_levels(ctx, device_mg):
    lv, _ = R.hierarchy("2d", 1e4)
    rmg, dmg = R.multigrid("2d", 1e4), device_mg("2d", 1e4)
    assert len(lv) == 3
    b = seeded(lv[-1].n, lv[-1].bc_dofs, 7)
    xw = cheb_cycle(ctx, dmg, rmg, b, "w")
    ref = rmg.vcycle(2, b, np.zeros_like(b))
    err = relerr(xw, ref)
    print("W-cycle parity", err)
    assert err < SMOOTHER_TOL
    xv = cheb_cycle(ctx, dmg, rmg, b, "v")
    assert relerr(xv, xw) > 1e-3                               # cycles = 2 does something
    vref = R.ChebyshevMultigrid(rmg.levels, rmg.transfers, 2, bounds=rmg.bounds, cycles=1).vcycle(2, b, np.zeros_like(b))
    assert relerr(xv, vref) < SMOOTHER_TOL


def test_w_cycle_is_the_v_cycle_on_two_levels(ctx, device_mg):
    lv, _ = R.hierarchy("3d", 1e4)
    rmg, dmg = R.multigrid("3d", 1e4), device_mg("3d", 1e4)
    assert len(lv) == 2
    b = seeded(lv[-1].n, lv[-1].bc_dofs, 7)
    xw, xv = cheb_cycle(ctx, dmg, rmg, b, "w"), cheb_cycle(ctx, dmg, rmg, b, "v")
    assert relerr(xw, xv) <= 1e-14                             # level 1 recurses once
    assert relerr(xw, rmg.vcycle(1, b, np.zeros_like(b))) < SMOOTHER_TOL


# ---- 8. the experiment -----------------------------------------------------------------------------------------------------------
def run_cg(ctx, case, gamma, smoother="patch", transfer=True, patch="star"):
    from alfi_amd.solver import HipCG, graddiv_solver
    lv, tr = R.sv_hierarchy(gamma) if case == "sv" else R.hierarchy(case, gamma)
    cg = HipCG(ctx, lv, tr, graddiv_solver(smoother, patch=patch), transfer=transfer)
    try:
        b = R.rhs(lv[-1])
        x, its, rn = cg.solve(b)
    finally:
        cg.close()
    true = np.linalg.norm(b - lv[-1].A.to_scipy().tocsr() @ x)
    return its, rn, true, np.linalg.norm(b)


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_graddiv_experiment_patch_and_robust_transfer(ctx, case):
    its = {}
    for g in R.GAMMAS:
        its[g], rn, true, bn = run_cg(ctx, case, g)
        ref = R.solve(case, g)[0]
        print("graddiv", case, g, "iterations", its[g], "restatement", ref, "rnorm", rn, "true", true)
        assert abs(its[g] - ref) <= 1, (case, g, its[g], ref)
        assert abs(rn - true) <= 1e-2 * true, (rn, true)
        assert rn <= 1e-8 * bn * (1 + 1e-2)
    assert max(its.values()) <= 16 and max(its.values()) - min(its.values()) <= 6, its


def test_graddiv_experiment_plain_transfers_are_not_robust(ctx):
    its = run_cg(ctx, "2d", 1e4, transfer=False)[0]
    assert its > 100, its


def test_plain_transfers_of_the_bubble_corrected_pair_are_p_and_its_transpose(ctx):
    """3-D [P1+FB]^3: the plain prolongation is bubble-corrected, and HipCG(transfer=False) must restrict with ITS transpose (the
    device transfer with gamma = 0, robust restriction on) -- the non-robust restriction is the transpose of the plain nodal
    interpolation, another matrix.  The restatement (P and P.T) converges in 51 iterations at gamma = 1e4."""
    from alfi_amd import hip
    its, rn, true, bn = run_cg(ctx, "3d", 1e4, transfer=False)
    ref = R.solve("3d", 1e4, "patch", False)[0]
    print("graddiv 3d plain transfers", its, ref)
    assert ref < R.MAX_IT and abs(its - ref) <= 1, (its, ref)
    assert rn <= 1e-8 * bn * (1 + 1e-2)
    # adjointness at gamma = 0: (P xc) . rf == xc . (restrict rf) with the robust restriction, to rounding
    lv, tr = R.hierarchy("3d", 1e4)
    mg = hip.Multigrid(ctx, lv, tr, 2, robust_restriction=True)
    try:
        T, (Lc, Lf) = mg.transfers[0], lv
        T.update(tr[0].nu, 0.0)
        xc, rf = seeded(Lc.n, Lc.bc_dofs, 1), seeded(Lf.n, Lf.bc_dofs, 2)
        dxf, drc = ctx.vec(Lf.n), ctx.vec(Lc.n)
        T.prolong(ctx.vec(xc), dxf)
        T.restrict(ctx.vec(rf), drc, robust=True)
        lhs, rhs = dxf.get() @ rf, xc @ drc.get()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
        P = tr[0].P.to_scipy()
        assert relerr(dxf.get(), np.where(np.isin(np.arange(Lf.n), Lf.bc_dofs), 0.0, P @ xc)) < 1e-13
    finally:
        mg.close()


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_graddiv_experiment_jacobi_is_not_robust(ctx, case):
    its = run_cg(ctx, case, 1e4, smoother="jacobi")[0]
    assert its > 100, its


# ---- 9. macro stars ------------------------------------------------------------------------------------------------------------
def test_graddiv_experiment_macro_star_patches(ctx):
    its, rn, true, bn = run_cg(ctx, "sv", 1e4, patch="macro")
    ref = R.solve("sv", 1e4)[0]
    print("graddiv macro", its, ref)
    assert abs(its - ref) <= 1, (its, ref)
    assert rn <= 1e-8 * bn * (1 + 1e-2)


# ---- 10. refusals and state ------------------------------------------------------------------------------------------------------
def test_bad_chebyshev_arguments_leave_x_untouched(ctx, device_mg):
    from alfi_amd import hip
    dl = device_mg("2d", 1e4).levels[-1]
    x0 = np.random.default_rng(3).standard_normal(dl.n)
    db, dx = ctx.vec(x0[::-1].copy()), ctx.vec(x0)
    for k, emin, emax in ((2, 0.0, 1.0), (2, -1.0, 1.0), (2, 1.0, 1.0), (2, 2.0, 1.0), (0, 0.3, 3.0), (2, float("nan"), 3.0)):
        with pytest.raises(hip.AlfiHipError, match="error -2"):            # ALFI_E_ARG
            dl.smooth_chebyshev(k, emin, emax, db, dx)
        assert np.array_equal(dx.get(), x0)
    with pytest.raises(hip.AlfiHipError, match="error -2"):
        dl.arnoldi(31, dx)
    with pytest.raises(hip.AlfiHipError, match="error -2"):
        device_mg("2d", 1e4).set_smoother("chebyshev", [(0.3, 3.0), (3.0, 0.3)])


def test_partitioned_levels_are_refused(ctx):
    """One rank, in-process: a level marked as partitioned and distributed (alfi_level_set_partition, as alfi_amd.dist does)."""
    from alfi_amd import hip
    A, bc = tridiagonal(8, 2, "flat")
    lvl = hip.Level(ctx, A, bc)
    lvl.set_partition(A.nbrows, True, np.zeros(0, dtype=np.int32), None, None, 0)
    mg = hip.Multigrid.__new__(hip.Multigrid)
    hip.Multigrid._from_device_levels(mg, ctx, [lvl], [], 2, False)
    x0 = np.arange(lvl.n, dtype=np.float64)
    db, dx = ctx.vec(lvl.n), ctx.vec(x0)
    calls = [lambda: lvl.set_jacobi(True), lambda: lvl.smooth_chebyshev(2, 0.3, 3.0, db, dx), lambda: lvl.arnoldi(3, dx),
             lambda: mg.set_smoother("chebyshev", []), lambda: mg.set_cycle_type("w"), lambda: mg.cg(db, dx)]
    try:
        for call in calls:
            with pytest.raises(hip.AlfiHipError, match="error -2.*partitioned"):
                call()
        assert np.array_equal(dx.get(), x0)
    finally:
        mg.close()
        lvl.close()


def test_switch_to_chebyshev_under_graph_replay_needs_no_allocation_in_the_cycle(ctx, device_mg):
    """Graphs on, two FGMRES cycles on one pair of buffers (the second one is captured), then Chebyshev / W on the SAME pair of a
    hierarchy that has never run the Chebyshev smoother: the re-capture must find the smoother's workspace in place
    (alfi_mg_set_smoother allocates it; an allocation inside a capturing cycle is an error).  Bit for bit the eager result."""
    from alfi_amd import hip
    lv, tr = R.hierarchy("2d", 1e4)
    rmg, ref_mg = R.multigrid("2d", 1e4), device_mg("2d", 1e4)
    b = seeded(lv[-1].n, lv[-1].bc_dofs, 11)

    def sequence(mg):
        db, dx = ctx.vec(b), ctx.vec(lv[-1].n)
        out = []
        for _ in range(2):
            mg.vcycle(db, dx)
            out.append(dx.get())
        mg.set_smoother("chebyshev", rmg.bounds[1:])
        mg.set_cycle_type("w")
        for _ in range(2):
            mg.vcycle(db, dx)
            out.append(dx.get())
        mg.set_smoother("fgmres")
        mg.set_cycle_type("v")
        return out
    eager = sequence(ref_mg)
    fresh = hip.Multigrid(ctx, lv, tr, 2, robust_restriction=True)
    ctx.set_graph(True)
    try:
        replayed = sequence(fresh)
    finally:
        ctx.set_graph(False)
        fresh.close()
    for i, (a, e) in enumerate(zip(replayed, eager)):
        assert np.array_equal(a, e), i
    assert relerr(eager[3], eager[2]) > 1e-9


def test_default_cycle_is_restored_bit_for_bit_and_graphs_replay_the_w_cycle(ctx, device_mg):
    lv, _ = R.hierarchy("2d", 1e4)
    rmg, dmg = R.multigrid("2d", 1e4), device_mg("2d", 1e4)
    b = seeded(lv[-1].n, lv[-1].bc_dofs, 9)
    db, dx = ctx.vec(b), ctx.vec(lv[-1].n)
    dmg.vcycle(db, dx)
    default = dx.get()
    # three consecutive W / Chebyshev cycles on one pair of buffers: eager, then with graphs on (the first call of a pair runs
    # eagerly, the second captures and replays, the third replays)
    dmg.set_smoother("chebyshev", rmg.bounds[1:])
    dmg.set_cycle_type("w")
    eager = []
    dx.zero()
    for _ in range(3):
        dmg.vcycle(db, dx)
        eager.append(dx.get())
    ctx.set_graph(True)
    try:
        db2, dx2 = ctx.vec(b), ctx.vec(lv[-1].n)
        for i in range(3):
            dmg.vcycle(db2, dx2)
            assert np.array_equal(dx2.get(), eager[i]), i
    finally:
        ctx.set_graph(False)
    assert relerr(eager[1], eager[0]) > 1e-6                   # the iterate moves: the comparison above is not vacuous
    dmg.set_smoother("fgmres")
    dmg.set_cycle_type("v")
    dx.zero()
    dmg.vcycle(db, dx)
    assert np.array_equal(dx.get(), default)
