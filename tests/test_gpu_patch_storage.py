"""Single-precision storage of dense patch inverses (alfi_patches_set_storage; hip.Level.set_patch_storage and the front ends'
patch_factor_dtype="f32"): the stored values are float32, every product and sum of the apply FP64.  -m gpu.

Error model: for stored values fl32(inv(A_p)) and FP64 arithmetic, |(apply_f32 - apply_f64)_i| <= 2^-24 (|inv(A_p)| |x|)_i summed
over the patches that hold dof i, plus FP64 round-off.  The model is derived, not measured; the tests use it as it stands
(factor 1.01, plus 1e-13 of the largest entry for the FP64 round-off of either apply).

Shapes: ldc3d on the 2 x 2 x 2 base mesh refined once (N = 4, 125 patches): [P2+FB]^3 (stars of 153 dofs, boundary shapes 3 / 9 /
21 / 33 / 57: 8 waves per patch) and [P1+FB]^3 (stars of 111 dofs: 4 waves per patch); synthetic dof sets of 33 .. 160 dofs on the
[P2+FB]^3 operator (every residue mod 4, both sides of the 64- and 128-dof boundaries between the kernels of 1, 4 and 8 waves, the
last piece of every width)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
K = 4
# synthetic patch sizes per kernel (waves per patch), the patch count of each level not a multiple of 4
SIZES = {1: [33, 34, 35, 36, 63, 64, 33], 4: [65, 66, 67, 111, 127, 128, 36], 8: [129, 130, 131, 153, 157, 158, 159, 160, 64]}


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def p2():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 2, Re=1000.0)


@pytest.fixture(scope="module")
def p1():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 1, Re=10.0)


@pytest.fixture(scope="module")
def ctx():
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cctx():
    """every FP64 level condenses where it finds groups"""
    from alfi_amd import hip
    c = hip.Context(0)
    c.set_condense_min_bytes(0)
    yield c
    c.close()


def _level(ctx, L, ptr, dofs, dtype=None, dense=False):
    from alfi_amd import hip
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(ptr, dofs)
    if dense:
        dl.set_patch_groups(None)
    if dtype is not None:
        dl.set_patch_storage(dtype)
    dl.factor()
    return dl


def _apply(ctx, dl, x):
    dx, dy = ctx.vec(x), ctx.vec(len(x))
    dl.patch_apply(dx, dy)
    return dy.get()


def _host_apply(dl, L, ptr, dofs, x):
    """(sum_p inv_p x_p, sum_p |inv_p| |x_p|) with the inverses the level returns; Dirichlet entries copied"""
    y, bound = np.zeros(L.n), np.zeros(L.n)
    for p in range(len(ptr) - 1):
        d = dofs[ptr[p]:ptr[p + 1]]
        inv = dl.patch_inverse(p, len(d))
        y[d] += inv @ x[d]
        bound[d] += np.abs(inv) @ np.abs(x[d])
    y[L.bc_dofs] = x[L.bc_dofs]
    return y, bound


def _check_b_c(ctx, f32, f64, L, ptr, dofs, x, label):
    """(b) the FP32 level's apply is the FP64 product of ITS stored values with x; (c) it differs from the FP64 level's apply
    within the error model."""
    y32, y64 = _apply(ctx, f32, x), _apply(ctx, f64, x)
    own, bound32 = _host_apply(f32, L, ptr, dofs, x)
    big = np.abs(own).max()
    eb = np.abs(y32 - own)
    print("%s: (b) worst |apply - host product| / bound %.3e" % (label, (eb / (1e-13 * bound32 + 1e-13 * big)).max()))
    assert np.all(eb <= 1e-13 * bound32 + 1e-13 * big)
    _, bound64 = _host_apply(f64, L, ptr, dofs, x)
    ec = np.abs(y32 - y64)
    lim = 1.01 * U24 * bound64 + 1e-13 * big
    print("%s: (c) worst |f32 - f64| / bound %.3f, relative max-norm difference %.3e" % (label, (ec / lim).max(), relerr(y32, y64)))
    assert np.all(ec <= lim)
    return y32


@pytest.mark.parametrize("waves", sorted(SIZES))
def test_synthetic_patch_sets(ctx, p2, waves):
    L = p2[0][-1]
    rng = np.random.default_rng(waves)
    free = np.setdiff1d(np.arange(L.n), L.bc_dofs)
    ptr, dofs = [0], []
    for sz in SIZES[waves]:
        start = int(rng.integers(0, len(free) - sz))
        dofs.append(free[start:start + sz])                 # a window of consecutive free dofs: ascending, coupled
        ptr.append(ptr[-1] + sz)
    ptr, dofs = np.array(ptr, dtype=np.int64), np.concatenate(dofs).astype(np.int32)
    assert (len(ptr) - 1) % 4 != 0
    f32, f64 = _level(ctx, L, ptr, dofs, "f32"), _level(ctx, L, ptr, dofs, dense=True)
    try:
        assert f32.patch_storage_dtype() == "f32" and f64.patch_storage_dtype() == "f64"
        assert f32.condensed() == 0 and f32.factor_bytes() < 0.55 * f64.factor_bytes()
        # (a) the stored values are the FP64 inverse of the twin -- the same deterministic factorisation -- rounded to nearest
        for p, sz in enumerate(SIZES[waves]):
            a, b = f32.patch_inverse(p, sz), f64.patch_inverse(p, sz)
            assert np.array_equal(a, np.float32(b).astype(np.float64)), (p, sz)
        x = rng.standard_normal(L.n)
        y = _check_b_c(ctx, f32, f64, L, ptr, dofs, x, "%d wave(s) per patch" % waves)
        assert np.array_equal(y, _apply(ctx, f32, x))       # (d) bitwise reproducible
        # two range launches with an odd split (and the empty ranges at either end): a patch's result does not depend on the
        # launch it is computed in and the dof-wise sum runs in a fixed order, so the full-range result bit for bit
        npatch = len(ptr) - 1
        for split in (3, npatch - 2, 0, npatch):
            dx, dy = ctx.vec(x), ctx.vec(L.n)
            f32.patch_apply_split(split, dx, dy)
            assert np.array_equal(dy.get(), y), split
        # the probe's figures are those of the FP64 inverse
        assert f32.patch_check() == f64.patch_check()
    finally:
        f32.close()
        f64.close()


def test_p2_stars_do_not_condense_and_take_half_the_bytes(cctx, ctx, p2):
    from alfi_amd.dist import DistMultigrid
    lv, tr = p2
    L = lv[-1]
    assert set(np.diff(L.patch_ptr).tolist()) == {3, 9, 21, 33, 57, 153} and len(L.patch_ptr) - 1 == 125
    f32, twin = _level(cctx, L, L.patch_ptr, L.patch_dofs, "f32"), _level(cctx, L, L.patch_ptr, L.patch_dofs)
    dense = _level(ctx, L, L.patch_ptr, L.patch_dofs, dense=True)
    try:
        assert twin.condensed() == 2 and f32.condensed() == 0 and dense.condensed() == 0
        assert f32.patch_storage_dtype() == "f32"
        print("factor bytes: f32 %d, condensed f64 %d, dense f64 %d" % (f32.factor_bytes(), twin.factor_bytes(), dense.factor_bytes()))
        assert f32.factor_bytes() < 0.55 * dense.factor_bytes()
        x = np.random.default_rng(5).standard_normal(L.n)
        y = _check_b_c(cctx, f32, dense, L, L.patch_ptr, L.patch_dofs, x, "[P2+FB]^3 stars")
        worst, flagged, repaired, _ = f32.patch_check()
        assert 0.0 <= worst < 1e-6 and flagged == repaired
    finally:
        for d in (f32, twin, dense):
            d.close()
    # the range launches as a partitioned level issues them: a one-rank forced partition with the overlapped exchange, no ghosts,
    # so the interior ranges are [0, 62) and [62, 125) and the boundary range is empty
    dmg = DistMultigrid(lv, tr, K, solo=(0, 1), min_dofs=1, force_distributed=True, overlap=True, overlap_min_dofs=0,
                        patch_factor_dtype="f32")
    try:
        assert dmg.overlap_levels == [1] and dmg.patch_storage_dtypes()[1] == "f32" and dmg.patch_storage()[1][0] == 0
        fin = dmg.local_levels[1]
        assert fin.npatch_int == 125 and fin.patch_factor_dtype == "f32"
        dx, dy = dmg.local_vec(x), dmg.local_vec()
        dmg.levels[1].patch_apply(dx, dy)
        yr = np.empty(L.n)
        yr[fin.part.own_dofs()] = dmg.owned(dy)
        print("ranges [0, 62) + [62, 125) against the full range: %.3e" % relerr(yr, y))
        assert relerr(yr, y) < 1e-13
    finally:
        dmg.close()


# One V(4,4) cycle / one full cycle of the oracle (oracle/alfi_oracle.py: build_oracle_mg(lv, tr, 4) on this hierarchy, right-hand
# side default_rng(0).standard_normal with the Dirichlet entries zeroed) with every patch inverse rounded to float32 and widened
# again, against the same cycle with the FP64 inverses, relative max-norm difference on the CPU:
ORACLE_V, ORACLE_F = 4.869e-06, 6.585e-06
V_BOUND, F_BOUND = 10 * ORACLE_V, 10 * ORACLE_F


def test_p1_stars_and_cycles(ctx, p1):
    from alfi_amd import hip
    lv, tr = p1
    L = lv[-1]
    assert np.diff(L.patch_ptr).max() == 111
    f32, f64 = _level(ctx, L, L.patch_ptr, L.patch_dofs, "f32"), _level(ctx, L, L.patch_ptr, L.patch_dofs, dense=True)
    try:
        _check_b_c(ctx, f32, f64, L, L.patch_ptr, L.patch_dofs, np.random.default_rng(6).standard_normal(L.n), "[P1+FB]^3 stars")
    finally:
        f32.close()
        f64.close()
    b = np.random.default_rng(0).standard_normal(L.n)
    b[L.bc_dofs] = 0.0
    out = {}
    for dtype in (None, "f32"):
        mg = hip.Multigrid(ctx, lv, tr, K, patch_factor_dtype=dtype)
        assert [d.patch_storage_dtype() for d in mg.levels[1:]] == [dtype or "f64"]
        assert lv[-1].patch_factor_dtype == (dtype or "f64")
        db, dx = ctx.vec(b), ctx.vec(L.n)
        mg.vcycle(db, dx)
        v = dx.get()
        mg.fcycle(db, dx)
        out[dtype] = (v, dx.get())
        mg.close()
    ev, ef = relerr(out["f32"][0], out[None][0]), relerr(out["f32"][1], out[None][1])
    print("V(4,4) cycle f32 against f64 %.3e (oracle %.3e), full cycle %.3e (oracle %.3e)" % (ev, ORACLE_V, ef, ORACLE_F))
    assert ev < V_BOUND and ef < F_BOUND


def _outer_cases():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    return {"ldc2d-re10": (lambda: TwoDimLidDrivenCavityProblem(8), 2, 2, 10.0),
            "ldc2d-re1000": (lambda: TwoDimLidDrivenCavityProblem(8), 2, 2, 1000.0),
            "ldc3d-p1fb-re10": (lambda: ThreeDimLidDrivenCavityProblem(2), 1, 1, 10.0),
            "ldc3d-p2fb-re1000": (lambda: ThreeDimLidDrivenCavityProblem(2), 2, 1, 1000.0)}


@pytest.mark.parametrize("case", ["ldc2d-re10", "ldc2d-re1000", "ldc3d-p1fb-re10", "ldc3d-p2fb-re1000"])
def test_outer_solve(case):
    import alfi_amd
    from alfi_amd import hip
    from alfi_amd.problem import build_hierarchy, build_pressure_coupling
    mk, ke, nref, Re = _outer_cases()[case]
    prob = mk()
    lv, tr = build_hierarchy(prob, nref, ke, Re=Re, gamma=1e4)
    L = lv[-1]
    B, _ = build_pressure_coupling(L)
    params = alfi_amd.outer_solver(prob.dim, alfi_amd.fieldsplit_0_mg(alfi_amd.mg_levels_solver(prob.dim, smoothing=4)))
    params["ksp_rtol"] = 1e-9
    b = np.random.default_rng(2).standard_normal(L.n)
    b[L.bc_dofs] = 0.0
    res = {}
    ctx = hip.Context(0)
    try:
        for dtype in (None, "f32"):
            s = alfi_amd.HipOuterSolver(ctx, lv, tr, params, patch_factor_dtype=dtype)
            u, p, its, rn = s.solve(b)
            res[dtype] = (u, p, its, rn, [l.patch_factor_dtype for l in lv[1:]], s.rtol, s.atol)
            s.saddle.close()
            s.hmg.mg.close()
    finally:
        ctx.close()
    (u0, p0, its0, rn0, dt0, rtol, atol), (u1, p1, its1, rn1, dt1, _, _) = res[None], res["f32"]
    print("%s: iterations f64 %d / f32 %d, residual %.3e / %.3e, |B u| %.3e / %.3e, storage %s"
          % (case, its0, its1, rn0, rn1, np.abs(B @ u0).max(), np.abs(B @ u1).max(), dt1))
    assert set(dt0) == {"f64"}
    assert abs(its1 - its0) <= 1
    # The final TRUE residual within the solver's own tolerance.  The solver stops on FGMRES's recurrence residual; where the
    # true residual of the FP64 solve itself ends above the tolerance (the recurrence's round-off, which the storage of the
    # patch inverses does not touch) the FP32 solve may not end above that.
    # Measured (tolerance | FP64 | FP32): ldc2d Re 10 8.89e-8 | 1.351e-8 | 1.351e-8; ldc2d Re 1000 8.89e-8 | 1.305e-7 | 1.305e-7 (the
    # 2-D levels keep FP64: bitwise); ldc3d [P1+FB]^3 Re 10 4.54e-8 | 2.229e-8 | 2.228e-8; [P2+FB]^3 Re 1000 5.60e-8 | 3.689e-8 | 3.804e-8.
    tol = max(rtol * np.linalg.norm(b), atol)
    print("%s: tolerance %.3e, true residual f64 %.3e, f32 %.3e" % (case, tol, rn0, rn1))
    assert rn1 <= max(tol, rn0)
    assert np.abs(B @ u1).max() <= 10 * max(np.abs(B @ u0).max(), 1e-300)
    if prob.dim == 2:
        # every level's patches have <= 32 dofs: refused, FP64 kept, nothing changes
        assert set(dt1) == {"f64"}
        assert np.array_equal(u1, u0) and np.array_equal(p1, p0) and its1 == its0
    else:
        assert set(dt1) == {"f32"}


def test_newton_with_device_assembly():
    from alfi_amd.nssolver import HipNavierStokesSolver, run_solver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem
    res, seen, krylov = {}, [], {None: [], "f32": []}
    for dtype in (None, "f32"):
        s = HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 2, patch_factor_dtype=dtype, device_assembly=True)
        try:
            solve = s.saddle.solve

            def counted(*a, _solve=solve, _its=krylov[dtype], **kw):
                r = _solve(*a, **kw)
                _its.append(r[0])
                return r
            s.saddle.solve = counted
            if dtype:
                factor = s._factor_levels

                def noted():
                    factor()
                    seen.append([(dl.patch_storage_dtype(), dl.condensed(), dl.patch_check()) for dl in s.hmg.mg.levels[1:]])
                s._factor_levels = noted
            res[dtype] = run_solver(s, [10, 100])
            assert s.device_assembly
        finally:
            s.close()
    assert len(seen) >= sum(res["f32"][re]["nonlinear_iter"] for re in (10, 100))
    for refresh in seen:
        for dt, mode, (worst, flagged, repaired, _) in refresh:
            assert dt == "f32" and mode == 0
            assert 0.0 <= worst < 1e-6 and flagged == repaired
    for re in (10, 100):
        a, b = res["f32"][re], res[None][re]
        print("Re %d: Newton %d / %d, Krylov %s / %s" % (re, a["nonlinear_iter"], b["nonlinear_iter"], a["linear_iter"], b["linear_iter"]))
        assert a["converged"] and b["converged"]
        assert a["nonlinear_iter"] == b["nonlinear_iter"]
    print("Krylov iterations per Newton step: f32 %s, f64 %s" % (krylov["f32"], krylov[None]))
    assert len(krylov["f32"]) == len(krylov[None]) == sum(res[None][re]["nonlinear_iter"] for re in (10, 100))
    assert all(abs(x - y) <= 1 for x, y in zip(krylov["f32"], krylov[None]))


def test_canonical_elimination_order(ctx, p2):
    """alfi_patches_set_canonical_order: an FP32 level eliminates in the caller's order and stores the inverse in the order of
    patch_dofs.  The identity order changes nothing, bit for bit; the reversed order gives another rounding of the same inverse
    (FP64 round-off: the probe of this level stays below 1e-8, so 1e-6 of the largest entry bounds two eliminations' difference
    with two decimal digits to spare, plus one float32 ulp where an entry crosses a rounding boundary) and a level whose apply is
    still the FP64 product of its stored values; an FP64 level ignores the order; a non-permutation is refused."""
    from alfi_amd import hip
    L = p2[0][-1]
    ptr, dofs = np.asarray(L.patch_ptr), L.patch_dofs
    sizes = np.diff(ptr)
    ident = np.concatenate([np.arange(n) for n in sizes]).astype(np.int32)
    rev = np.concatenate([np.arange(n)[::-1] for n in sizes]).astype(np.int32)
    x = np.random.default_rng(9).standard_normal(L.n)
    plain, f64 = _level(ctx, L, ptr, dofs, "f32"), _level(ctx, L, ptr, dofs, dense=True)
    lev = {}
    try:
        for name, rank in (("ident", ident), ("rev", rev)):
            dl = hip.Level(ctx, L.A, L.bc_dofs)
            dl.set_patches(ptr, dofs)
            dl.set_patch_storage("f32")
            dl.set_patch_canonical_order(rank)
            dl.factor()
            lev[name] = dl
        full = int(np.argmax(sizes))
        a, b, c = (d.patch_inverse(full, 153) for d in (plain, lev["ident"], lev["rev"]))
        assert np.array_equal(a, b) and np.array_equal(_apply(ctx, plain, x), _apply(ctx, lev["ident"], x))
        print("reversed elimination order against ascending: inverse %.3e of the largest entry" % relerr(c, a))
        assert not np.array_equal(a, c) and np.abs(c - a).max() < (1e-6 + 2.0 ** -23) * np.abs(a).max()
        _check_b_c(ctx, lev["rev"], f64, L, ptr, dofs, x, "reversed elimination order")
        worst, flagged, repaired, _ = lev["rev"].patch_check()
        assert 0.0 <= worst < 1e-6 and flagged == repaired
        # FP64 storage: the order is not used
        y64 = _apply(ctx, f64, x)
        f64.set_patch_canonical_order(rev)
        f64.factor()
        assert np.array_equal(_apply(ctx, f64, x), y64)
        bad = ident.copy()
        bad[ptr[full] + 1] = bad[ptr[full]]
        assert "permutation" in _refused(lambda: plain.set_patch_canonical_order(bad), hip.E_ARG)
        plain.set_patch_canonical_order(None)
    finally:
        for d in [plain, f64] + list(lev.values()):
            d.close()


def _refused(fn, code):
    from alfi_amd import hip
    with pytest.raises(hip.AlfiHipError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    text = str(e.value).split(":", 1)[1].strip()
    assert len(text) > 10
    return text


def test_refusals(ctx, p2):
    from alfi_amd import hip
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, build_hierarchy
    L = p2[0][-1]
    x = np.random.default_rng(8).standard_normal(L.n)

    def fresh():
        dl = hip.Level(ctx, L.A, L.bc_dofs)
        dl.set_patches(L.patch_ptr, L.patch_dofs)
        return dl

    def works_in_f64(dl, ref=None):
        dl.factor()
        assert dl.patch_storage_dtype() == "f64"
        y = _apply(ctx, dl, x)
        assert np.isfinite(y).all() and (ref is None or relerr(y, ref) < 1e-8)
        return y
    dl = fresh()
    dl.set_patch_groups(None)
    ref = works_in_f64(dl)
    dl.close()
    with pytest.raises(ValueError):
        fresh().set_patch_storage("f16")
    # --- asked of a level that has no FP32 form: ALFI_E_ARG, the level stays as it was
    # small 2-D stars (the interleaved copy)
    lv2, _ = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 1, 2, Re=10.0)
    L2 = lv2[-1]
    assert np.diff(L2.patch_ptr).max() <= 32
    d2 = hip.Level(ctx, L2.A, L2.bc_dofs)
    d2.set_patches(L2.patch_ptr, L2.patch_dofs)
    assert "32" in _refused(lambda: d2.set_patch_storage("f32"), hip.E_ARG)
    d2.factor()
    assert d2.patch_storage_dtype() == "f64"
    d2.close()
    # a patch above 160 dofs
    free = np.setdiff1d(np.arange(L.n), L.bc_dofs)
    big = hip.Level(ctx, L.A, L.bc_dofs)
    big.set_patches(np.array([0, 40, 40 + 162]), np.concatenate([free[:40], free[100:262]]).astype(np.int32))
    assert "160" in _refused(lambda: big.set_patch_storage("f32"), hip.E_ARG)
    big.factor()
    assert big.patch_storage_dtype() == "f64"
    big.close()
    # caller-supplied groups
    dl = fresh()
    dl.set_patch_groups(dl.find_patch_groups())
    assert "groups" in _refused(lambda: dl.set_patch_storage("f32"), hip.E_ARG)
    works_in_f64(dl, ref)
    assert dl.condensed() == 1
    dl.close()
    # multiplicative sweeps
    dl = fresh()
    dl.factor()
    dl.set_multiplicative(np.arange(len(L.patch_ptr) - 1), False)
    assert "multiplicative" in _refused(lambda: dl.set_patch_storage("f32"), hip.E_ARG)
    dl.set_multiplicative(None, False)
    works_in_f64(dl, ref)
    dl.close()
    # a facet correction (empty lists: the rule is set, it corrects nothing)
    dl = fresh()
    nrow = int(L.patch_ptr[-1]) // L.bs
    dl.set_patch_facet_correction(1, np.zeros(nrow + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32),
                                  np.zeros(0))
    assert "facet" in _refused(lambda: dl.set_patch_storage("f32"), hip.E_ARG)
    works_in_f64(dl, ref)
    dl.close()
    # --- the other direction, on an FP32 level: ALFI_E_STATE, the level stays FP32; back to FP64 on request
    dl = fresh()
    dl.set_patch_storage("f32")
    assert dl.patch_storage_dtype() == "f64"                 # the NEXT factorisation obeys
    assert "FP32" in _refused(lambda: dl.set_multiplicative(np.arange(5), False), hip.E_STATE)
    assert "FP32" in _refused(lambda: dl.set_patch_groups(np.full(int(L.patch_ptr[-1]), -1, dtype=np.int32)), hip.E_STATE)
    assert "FP32" in _refused(lambda: dl.set_patch_facet_correction(1, np.zeros(nrow + 1, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                                                    np.zeros(0, dtype=np.int32), np.zeros(0)), hip.E_STATE)
    dl.factor()
    assert dl.patch_storage_dtype() == "f32" and dl.condensed() == 0
    y32 = _apply(ctx, dl, x)
    assert 0 < relerr(y32, ref) < 1e-6
    for fn in (lambda: dl.set_multiplicative(np.arange(5), False),
               lambda: dl.set_patch_groups(np.full(int(L.patch_ptr[-1]), -1, dtype=np.int32))):
        _refused(fn, hip.E_STATE)
    assert np.array_equal(_apply(ctx, dl, x), y32)
    dl.set_patch_storage("f64")
    assert dl.patch_storage_dtype() == "f32" and np.array_equal(_apply(ctx, dl, x), y32)    # until the next factorisation
    works_in_f64(dl, ref)
    assert dl.set_multiplicative(np.arange(len(L.patch_ptr) - 1), False) >= 1                # and everything is allowed again
    dl.close()
