"""Vertex-star patch factors condensed by the library itself (alfi_patches_find_groups + the automatic policy of
alfi_patches_factor, forced here with Context.set_condense_min_bytes(0)) against dense inverses on the same operator, against
the oracle, and through the diagnostics the full-size tests use (patch_inverse, patch_check, set_multiplicative).  -m gpu.

Shapes: ldc3d [P2+FB]^3, Re 1000, one hierarchy N = 2 / 4 / 8.  N = 4: 125 patches, 27 full stars of 153 dofs and every
boundary shape (3 / 9 / 21 / 33 / 57 dofs); N = 8: 729 patches.  Launches of fewer than 1024 patches take the chunked form of
the condensed apply, larger ones a workgroup per patch: the N = 8 patch set listed twice (1458 patches) runs the latter.
Tolerances: condensed against the oracle 1e-7 and against dense 1e-8 in the max norm relative to the reference
(tests/test_gpu_condensed.py); cycles 1e-5 (tests/test_gpu_parity.py: CYCLE_TOL)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CYCLE_TOL = 1e-5
K = 4


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def hier():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)


@pytest.fixture(scope="module")
def cctx():
    """every level condenses where it finds groups"""
    from alfi_amd import hip
    c = hip.Context(0)
    c.set_condense_min_bytes(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dctx():
    """the default threshold: these small levels keep dense inverses"""
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _level(ctx, L, patch_ptr=None, patch_dofs=None):
    from alfi_amd import hip
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(L.patch_ptr if patch_ptr is None else patch_ptr, L.patch_dofs if patch_dofs is None else patch_dofs)
    return dl


def _patch_matrix(L, p):
    dofs = L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]]
    return dofs, L.A.to_scipy().tocsr()[dofs][:, dofs].toarray()


def test_find_groups_on_the_device_level(cctx, dctx, hier):
    from alfi_amd import _hostlib
    L = hier[0][1]                                                            # N = 4
    dl = _level(cctx, L)
    g = dl.find_patch_groups()
    assert np.array_equal(g, dl.find_patch_groups())                          # two identical calls, identical labels
    assert np.array_equal(g, _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs))
    sizes = np.diff(L.patch_ptr)
    assert set(sizes.tolist()) == {3, 9, 21, 33, 57, 153}
    for p, n in enumerate(sizes):
        lab = g[L.patch_ptr[p]:L.patch_ptr[p + 1]]
        grp = sorted(np.bincount(lab[lab >= 0]).tolist()) if (lab >= 0).any() else []
        assert grp == {153: [15] * 6, 57: [15] * 2}.get(int(n), []), (p, n, grp)
        assert (lab < 0).sum() == {153: 63, 57: 27}.get(int(n), int(n))
    dl.set_patch_groups(g)                                                    # validated: groups mutually uncoupled
    dl.factor()
    assert dl.condensed() == 1
    dl.close()
    # the full stars alone: 6 (16 15 + 28 15 + 16 27) + 63 64 = 10 584 doubles against 153 154 = 23 562 with the even leading
    # dimensions: 0.449
    full = np.flatnonzero(sizes == 153)
    pp = np.concatenate([[0], np.cumsum(sizes[full])])
    pd = np.concatenate([L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]] for p in full])
    out = {}
    for name, ctx in (("condensed", cctx), ("dense", dctx)):
        d = _level(ctx, L, pp, pd)
        d.factor()
        out[name] = d.factor_bytes()
        assert d.condensed() == (2 if name == "condensed" else 0)
        d.close()
    print("153-dof stars: condensed %d bytes, dense %d: %.3f" % (out["condensed"], out["dense"], out["condensed"] / out["dense"]))
    assert out["condensed"] <= 0.46 * out["dense"]


@pytest.mark.parametrize("name", ["b", "a"])
def test_the_device_level_plans_with_the_code_the_host_library_exports(dctx, name):
    """csrc/patch_plan.h once in each library: the level's factor bytes and wavefront count are those of the host plan of the
    same inputs (tests/patch_plan_cases.py: b = this file's N = 4 level as a hierarchy of its own, a = 2-D Scott-Vogelius)."""
    from tests.patch_plan_cases import case, plans
    L, groups, iterset = case(name)
    pl = plans(name)
    dl = _level(dctx, L)
    dl.set_patch_groups(groups)
    assert dl.condensed() == 1
    assert dl.factor_bytes() == 8 * (pl["cond"]["mat_doubles"] + pl["cond"]["sinv_doubles"])
    dl.set_patch_groups(None)                                                  # sweeps read dense inverses
    assert dl.set_multiplicative(iterset, True) == len(pl["sweep"]["wave_ptr"]) - 1
    dl.close()


@pytest.mark.parametrize("shape", ["N4", "N8", "N8-twice"])
def test_condensed_apply_equals_dense_apply(cctx, dctx, hier, shape):
    from oracle import alfi_oracle as O
    L = hier[0][1 if shape == "N4" else 2]
    pp, pd = L.patch_ptr, L.patch_dofs
    if shape == "N8-twice":                  # 1458 patches: the workgroup-per-patch kernels of the large levels
        pp = np.concatenate([pp, pp[1:] + pp[-1]])
        pd = np.concatenate([pd, pd])
    x = np.random.default_rng(0).standard_normal(L.n)                          # Dirichlet entries non-zero on purpose
    out = {}
    for mode, ctx in (("dense", dctx), ("condensed", cctx)):
        dl = _level(ctx, L, pp, pd)
        dl.factor()
        assert dl.condensed() == (2 if mode == "condensed" else 0)
        worst, flagged, repaired, after = dl.patch_check()
        print(shape, mode, "probe worst %.3e flagged %d repaired %d" % (worst, flagged, repaired))
        assert 0.0 <= worst < 1e-6 and flagged == repaired
        dx, dy = ctx.vec(x), ctx.vec(L.n)
        dl.patch_apply(dx, dy)
        out[mode] = (dy.get(), dl.factor_bytes())
        dl.patch_apply(dx, dy)
        assert np.array_equal(dy.get(), out[mode][0])                           # bitwise reproducible
        assert np.array_equal(out[mode][0][L.bc_dofs], x[L.bc_dofs])           # Dirichlet entries copied exactly
        dl.close()
    ref = O.PatchSmoother(L.A.to_scipy().tocsr(), pp, pd, L.bc_dofs).apply(x)
    print(shape, "dense %.2e condensed %.2e against the oracle, condensed against dense %.2e, bytes %d / %d"
          % (relerr(out["dense"][0], ref), relerr(out["condensed"][0], ref), relerr(out["condensed"][0], out["dense"][0]),
             out["condensed"][1], out["dense"][1]))
    assert relerr(out["condensed"][0], ref) < 1e-7
    assert relerr(out["condensed"][0], out["dense"][0]) < 1e-8
    assert out["condensed"][1] < 0.55 * out["dense"][1]


def test_patch_inverse_of_a_condensed_level(cctx, hier):
    L = hier[0][1]
    dl = _level(cctx, L)
    dl.factor()
    assert dl.condensed() == 2
    x = np.random.default_rng(3).standard_normal(L.n)
    dx, dy = cctx.vec(x), cctx.vec(L.n)
    dl.patch_apply(dx, dy)
    Mx = dy.get()
    sizes = np.diff(L.patch_ptr)
    holders = {}                                                              # patch -> its dense inverse

    def inverse(p):
        if p not in holders:
            holders[p] = dl.patch_inverse(int(p), int(sizes[p]))
        return holders[p]

    for n in sorted(set(sizes.tolist())):
        for p in np.flatnonzero(sizes == n)[:2]:
            dofs, Ap = _patch_matrix(L, p)
            X = inverse(p)
            res = np.abs(X @ Ap - np.eye(n)).max()
            print("patch %d (%d dofs): |X A - I| %.3e, cond %.3e" % (p, n, res, np.linalg.cond(Ap)))
            assert res < 1e-8 * np.linalg.cond(Ap), (p, res)
            # the apply at one dof of the patch = the sum over the patches holding it of their row of the inverse times x there
            d = dofs[len(dofs) // 2]
            val = 0.0
            for q in range(len(sizes)):
                qd = L.patch_dofs[L.patch_ptr[q]:L.patch_ptr[q + 1]]
                row = np.flatnonzero(qd == d)
                if row.size:
                    val += inverse(q)[row[0]] @ x[qd]
            assert abs(Mx[d] - val) < 1e-9 * max(abs(val), np.abs(Mx).max() * 1e-3), (p, d, Mx[d], val)
    dl.close()


def test_multiplicative_sweeps_send_a_found_condensation_back_to_dense(cctx, dctx, hier):
    from alfi_amd import hip
    L = hier[0][1]
    npatch = len(L.patch_ptr) - 1
    it = np.arange(npatch)
    x = np.random.default_rng(5).standard_normal(L.n)
    dl = _level(cctx, L)
    dl.factor()
    assert dl.condensed() == 2
    small = dl.factor_bytes()
    dl.set_multiplicative(it, True)                                            # succeeds: back to dense inverses, factored again
    assert dl.condensed() == 0 and dl.factor_bytes() > small
    ref = _level(dctx, L)                                                      # never condensed
    ref.set_multiplicative(it, True)
    ref.factor()
    assert ref.condensed() == 0 and dl.factor_bytes() == ref.factor_bytes()
    dx, dy, rx, ry = cctx.vec(x), cctx.vec(L.n), dctx.vec(x), dctx.vec(L.n)
    dl.patch_apply(dx, dy)
    ref.patch_apply(rx, ry)
    assert np.array_equal(dy.get(), ry.get())
    dl.factor()                                                                # stays dense at the next factorisation
    assert dl.condensed() == 0
    dl.patch_apply(dx, dy)
    assert np.array_equal(dy.get(), ry.get())
    dl.close()
    ref.close()
    own = _level(cctx, L)                                                      # the caller's groups: still an error
    own.set_patch_groups(own.find_patch_groups())
    own.factor()
    with pytest.raises(hip.AlfiHipError, match="dense patch inverses"):
        own.set_multiplicative(it, True)
    own.close()


def test_vcycles_with_every_smoothed_level_condensed(cctx, dctx, hier):
    from alfi_amd import hip
    from oracle import alfi_oracle as O
    lv, tr = hier
    L = lv[-1]
    b = np.random.default_rng(8).standard_normal(L.n)
    b[L.bc_dofs] = 0.0
    hist, first = {}, {}
    for mode, ctx in (("dense", dctx), ("condensed", cctx)):
        mg = hip.Multigrid(ctx, lv, tr, K, robust_restriction=True)
        assert [d.condensed() for d in mg.levels[1:]] == [2 if mode == "condensed" else 0] * 2
        assert hip.condense_patches(L) == (mode == "condensed")
        db, du, dr = ctx.vec(b), ctx.vec(L.n), ctx.vec(L.n)
        h = []
        for i in range(3):
            mg.vcycle(db, du)
            if i == 0:
                first[mode] = du.get()
            mg.levels[-1].residual(db, du, dr)
            h.append(np.linalg.norm(dr.get()))
        hist[mode] = np.array(h)
        mg.close()
    print("residual histories", hist, "largest relative difference %.3e" % np.abs(hist["condensed"] / hist["dense"] - 1.0).max())
    assert (np.abs(hist["condensed"] - hist["dense"]) < 1e-6 * hist["dense"]).all()
    ref = O.build_oracle_mg(lv, tr, K, schoeberl_restriction=True).vcycle(len(lv) - 1, b, np.zeros(L.n))
    print("first V-cycle against the oracle: condensed %.3e dense %.3e" % (relerr(first["condensed"], ref), relerr(first["dense"], ref)))
    assert relerr(first["condensed"], ref) < CYCLE_TOL


def test_a_burman_level_never_keeps_found_groups(cctx, dctx):
    """Burman levels are out of scope for the condensed factors (the facet term couples macro interiors, PCPATCH's facet rule
    changes the patch matrices).  With the threshold at 0: a level that declares its facet-coupled sparsity
    (set_facet_blocks) never looks for groups; a level that is told only later, by set_patch_facet_correction AFTER its first
    factorisation -- the order of the Newton solver -- and had found groups in the facet-coupled sparsity goes back to dense
    inverses there, factors with a non-zero Burman weight, and holds the bits of a level that was never condensed."""
    from alfi_amd import hip
    from alfi_amd.burman import patch_facet_corrections
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import BSR, TwoDimLidDrivenCavityProblem
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 2, 2, discretisation="sv", stabilisation_type="burman",
                              stabilisation_weight=5e-3, device_assembly=True)
    try:
        d = s.problem.dim
        u = np.random.default_rng(5).standard_normal(s.n_u)
        u[s.levels[-1].bc_dofs] = 0.0
        s.nu = 0.05
        s._device_states(u)
        L, st, obj = s.levels[-1], s._dstate[-1], s.hmg.pc_objs[-1]
        assert L.facet_coupling and not obj.condensed and s.hmg.mg.levels[-1].condensed() == 0
        A = BSR(L.A.nbrows, L.A.nbcols, d, L.A.rowptr, L.A.colidx, s.level_values(L, st.get().reshape(-1, d), 1.0, True))
        beta, scale = L.facet_beta
        assert scale != 0.0
        corr = patch_facet_corrections(L.V, L.facets, obj.patch_ptr, obj.patch_dofs)
        pp, pd, nf, bc = obj.patch_ptr, obj.patch_dofs, L.facets.nf, L.bc_dofs
    finally:
        s.close()
    x = np.random.default_rng(6).standard_normal(A.nbrows * d)
    out = {}
    for mode, ctx in (("late", cctx), ("declared", cctx), ("never", dctx)):
        dl = hip.Level(ctx, A, bc)
        if mode == "declared":
            dl.set_facet_blocks(True)
        dl.set_patches(pp, pd)
        dl.factor()
        if mode == "late":
            assert dl.condensed() == 2                  # nothing told the level yet: it found groups in this sparsity
            small = dl.factor_bytes()
        else:
            assert dl.condensed() == 0
        dl.set_patch_facet_correction(nf, *corr)
        assert dl.condensed() == 0
        dl.set_facet_beta(beta, scale)
        dl.factor()                                     # (condensed factors with a Burman weight would be an error here)
        assert dl.condensed() == 0
        if mode == "late":
            assert dl.factor_bytes() > small
        worst, flagged, repaired, _ = dl.patch_check()
        assert 0.0 <= worst < 1e-6 and flagged == repaired
        dx, dy = ctx.vec(x), ctx.vec(len(x))
        dl.patch_apply(dx, dy)
        out[mode] = (dy.get(), dl.factor_bytes(), dl.patch_inverse(0, int(pp[1] - pp[0])))
        dl.close()
    for mode in ("late", "declared"):
        assert np.array_equal(out[mode][0], out["never"][0]) and out[mode][1] == out["never"][1]
        assert np.array_equal(out[mode][2], out["never"][2])
