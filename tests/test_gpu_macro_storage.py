"""Single-precision storage of dense MACRO-STAR inverses, Burman levels included (alfi_patches_set_macro_storage;
hip.Level.set_macro_patch_storage and the front ends' macro_factor_dtype="f32"): big_apply_kernel<float, NT>, the factorisation in patch
ranges through the context's work buffer (alfi_ctx_set_f32_work_bytes), and the facet rule on FP32 levels.  -m gpu.

Error model (tests/test_gpu_patch_storage.py): for stored values fl32(inv(A_p)) and FP64 arithmetic,
    (b) |apply - host product of the stored values| <= 1e-13 bound + 1e-13 big,
    (c) |f32 - f64|                                 <= 1.01 2^-24 bound + 1e-13 big,
bound_i = sum over the patches holding dof i of (|inv(A_p)| |x|)_i, big = the largest entry of the result.  Derived, not measured.

Shapes: windows of consecutive free dofs on the [P2+FB]^3 N = 4 operator at Re 1000 (161 .. 513 dofs: every residue mod 4, both
sides of the 128-row piece boundary, one patch below 160 inside a big level; with the 513-dof patch two workgroups share a patch,
without it one does); the 27 macro stars of 3-D [P3]^3 on the 1 x 1 x 1 base mesh refined once (150 .. 1599 dofs, four
workgroups per patch); the two Burman cases of tests/test_gpu_burman.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SIZES = {2: [161, 162, 163, 164, 255, 256, 257, 385, 513, 150], 1: [161, 162, 163, 164, 255, 256, 257, 385, 150]}


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def p2():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 2, Re=1000.0)


@pytest.fixture(scope="module")
def sv3():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem
    from alfi_amd.sv import build_sv_hierarchy
    return build_sv_hierarchy(ThreeDimLidDrivenCavityProblem(1), 1, 3, Re=100.0, gamma=1e4)


@pytest.fixture(scope="module")
def ctx():
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _windows(L, sizes, seed):
    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(L.n), L.bc_dofs)
    ptr, dofs = [0], []
    for sz in sizes:
        start = int(rng.integers(0, len(free) - sz))
        dofs.append(free[start:start + sz])                 # a window of consecutive free dofs: ascending, coupled
        ptr.append(ptr[-1] + sz)
    return np.array(ptr, dtype=np.int64), np.concatenate(dofs).astype(np.int32)


def _level(ctx, L, ptr, dofs, dtype=None):
    """dense inverses (no groups, no search for any), FP64 or asked for FP32 through the macro call"""
    from alfi_amd import hip
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(ptr, dofs)
    dl.set_patch_groups(None)
    if dtype is not None:
        dl.set_macro_patch_storage(dtype)
    dl.factor()
    return dl


def _apply(ctx, dl, x):
    dx, dy = ctx.vec(x), ctx.vec(len(x))
    dl.patch_apply(dx, dy)
    return dy.get()


def _inverses(dl, ptr):
    return [dl.patch_inverse(p, int(ptr[p + 1] - ptr[p])) for p in range(len(ptr) - 1)]


def _host_apply(invs, L, ptr, dofs, x):
    """(sum_p inv_p x_p, sum_p |inv_p| |x_p|); Dirichlet entries copied"""
    y, bound = np.zeros(L.n), np.zeros(L.n)
    for p, inv in enumerate(invs):
        d = dofs[ptr[p]:ptr[p + 1]]
        y[d] += inv @ x[d]
        bound[d] += np.abs(inv) @ np.abs(x[d])
    y[L.bc_dofs] = x[L.bc_dofs]
    return y, bound


def _check_b(y32, invs32, L, ptr, dofs, x, label):
    own, bound32 = _host_apply(invs32, L, ptr, dofs, x)
    big = np.abs(own).max()
    eb = np.abs(y32 - own)
    print("%s: (b) worst |apply - host product| / bound %.3e" % (label, (eb / (1e-13 * bound32 + 1e-13 * big)).max()))
    assert np.all(eb <= 1e-13 * bound32 + 1e-13 * big)
    return big


def _check_a_b_c(ctx, f32, f64, L, ptr, dofs, x, label):
    """(a) the stored values are float32 of the FP64 twin's -- the same deterministic factorisation -- exactly; (b); (c)"""
    i32, i64 = _inverses(f32, ptr), _inverses(f64, ptr)
    for p, (a, b) in enumerate(zip(i32, i64)):
        assert np.array_equal(a, np.float32(b).astype(np.float64)), (label, p, a.shape)
    y32, y64 = _apply(ctx, f32, x), _apply(ctx, f64, x)
    big = _check_b(y32, i32, L, ptr, dofs, x, label)
    _, bound64 = _host_apply(i64, L, ptr, dofs, x)
    ec = np.abs(y32 - y64)
    lim = 1.01 * U24 * bound64 + 1e-13 * big
    print("%s: (c) worst |f32 - f64| / bound %.3f, relative max-norm difference %.3e" % (label, (ec / lim).max(), relerr(y32, y64)))
    assert np.all(ec <= lim)
    return y32, y64


@pytest.mark.parametrize("split", sorted(SIZES))
def test_synthetic_big_patch_sets(ctx, p2, split):
    L = p2[0][-1]
    sizes = SIZES[split]
    ptr, dofs = _windows(L, sizes, split)
    npatch = len(ptr) - 1
    assert npatch % 4 != 0 and min(sizes) < 160 < max(sizes) and ((max(sizes) + 127) // 128 + 3) // 4 == split
    f32, f64 = _level(ctx, L, ptr, dofs, "f32"), _level(ctx, L, ptr, dofs)
    try:
        assert f32.patch_storage_dtype() == "f32" and f64.patch_storage_dtype() == "f64"
        assert f32.condensed() == 0 and f32.factor_bytes() < 0.55 * f64.factor_bytes()
        x = np.random.default_rng(10 + split).standard_normal(L.n)
        y, _ = _check_a_b_c(ctx, f32, f64, L, ptr, dofs, x, "%d workgroup(s) per patch" % split)
        assert np.array_equal(y, _apply(ctx, f32, x))       # bitwise reproducible
        # two range launches with an odd split (and the empty ranges at either end): the full-range result bit for bit
        for cut in (3, npatch - 3, 0, npatch):
            dx, dy = ctx.vec(x), ctx.vec(L.n)
            f32.patch_apply_split(cut, dx, dy)
            assert np.array_equal(dy.get(), y), cut
        # the probe's figures are those of the FP64 inverses
        assert f32.patch_check() == f64.patch_check()
    finally:
        f32.close()
        f64.close()


def test_ranges_do_not_change_a_bit(p2):
    """One patch per range, several, one range for the level: the same stored values, the same apply, the same probe figures; the
    context's work buffer never exceeds max(cap, the largest patch) and goes with the context's last FP32 level."""
    from alfi_amd import _hostlib, hip
    L = p2[0][-1]
    ptr, dofs = _windows(L, SIZES[2], 2)
    lay = _hostlib.plan_patch_layout(L.n, ptr, dofs)
    pbytes = 8 * np.diff(lay["inv_ptr"])
    largest, level_bytes = int(pbytes.max()), int(pbytes.sum())
    middle = level_bytes // 4
    assert 3 * int(pbytes.min()) < middle < largest          # ranges of several patches, and one patch above the cap
    x = np.random.default_rng(3).standard_normal(L.n)
    c = hip.Context(0)
    levels, ref = [], None
    try:
        with pytest.raises(hip.AlfiHipError) as e:
            c.set_f32_work_bytes(0)
        assert e.value.code == hip.E_ARG
        assert c.f32_work_bytes() == 0
        twin = _level(c, L, ptr, dofs)
        levels.append(twin)
        for cap in (1, middle, 4 * level_bytes):
            c.set_f32_work_bytes(cap)
            dl = _level(c, L, ptr, dofs, "f32")
            levels.append(dl)
            held = c.f32_work_bytes()
            print("cap %d bytes: work buffer %d bytes (largest patch %d, level %d)" % (cap, held, largest, level_bytes))
            assert 0 < held <= max(cap, largest)
            got = (_inverses(dl, ptr), _apply(c, dl, x), dl.patch_check(), dl.factor_bytes())
            if ref is None:
                ref = got
                for a, b in zip(ref[0], _inverses(twin, ptr)):
                    assert np.array_equal(a, np.float32(b).astype(np.float64))
                assert got[2] == twin.patch_check()
            else:
                assert all(np.array_equal(a, b) for a, b in zip(got[0], ref[0])), cap
                assert np.array_equal(got[1], ref[1]) and got[2] == ref[2] and got[3] == ref[3], cap
        # the work buffer is not the level's: the levels' bytes are the floats
        assert ref[3] < 0.55 * twin.factor_bytes()
        for dl in levels:
            dl.close()
        levels = []
        assert c.f32_work_bytes() == 0
    finally:
        for dl in levels:
            dl.close()
        c.close()


def test_p3_macro_stars(ctx, sv3):
    lv, _ = sv3
    L = lv[-1]
    sizes = np.diff(L.patch_ptr)
    assert len(sizes) == 27 and sizes.min() == 150 and sizes.max() == 1599
    f32, f64 = _level(ctx, L, L.patch_ptr, L.patch_dofs, "f32"), _level(ctx, L, L.patch_ptr, L.patch_dofs)
    try:
        assert f32.patch_storage_dtype() == "f32" and f32.condensed() == 0 and f64.condensed() == 0
        assert f32.factor_bytes() < 0.55 * f64.factor_bytes()
        x = np.random.default_rng(11).standard_normal(L.n)
        y32, y64 = _check_a_b_c(ctx, f32, f64, L, np.asarray(L.patch_ptr), L.patch_dofs, x, "[P3]^3 macro stars")
        # Nothing lands outside a patch's own staging slots (the last patch has 150 = 2 mod 4 dofs: its pad rows would fall
        # behind the buffer, those of the others into the next patch's first slots): every Dirichlet-free dof -- the sum of
        # its staged values -- is within the error model of the twin (checked above), and every dof no patch holds is zero
        free = np.setdiff1d(np.arange(L.n), L.bc_dofs)
        held = np.zeros(L.n, dtype=bool)
        held[L.patch_dofs] = True
        assert any(int(n) % 4 in (1, 2) for n in sizes) and np.array_equal(y32[free][~held[free]], y64[free][~held[free]])
        assert np.array_equal(y32, _apply(ctx, f32, x))
        assert f32.patch_check() == f64.patch_check()
    finally:
        f32.close()
        f64.close()


BURMAN = [pytest.param("2d", 2, 2, id="2d-P2"), pytest.param("3d", 1, 3, id="3d-P3")]


def _burman_solver(dim, nref, k, **kw):
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    prob = TwoDimLidDrivenCavityProblem(2) if dim == "2d" else ThreeDimLidDrivenCavityProblem(1)
    return HipNavierStokesSolver(prob, nref, k, discretisation="sv", stabilisation_type="burman", stabilisation_weight=5e-3,
                                 device_assembly=True, **kw)


@pytest.mark.parametrize("dim,nref,k", BURMAN)
def test_burman_levels(dim, nref, k):
    """After a refresh at a random state every smoothed level holds float32 of the inverse of the facet-rule matrix (the
    construction of test_patch_inverses_follow_the_pcpatch_facet_rule), and applies what it holds."""
    from alfi_amd.burman import patch_facet_corrections
    from alfi_amd.problem import BSR
    s = _burman_solver(dim, nref, k)
    try:
        assert [dl.patch_storage_dtype() for dl in s.hmg.mg.levels[1:]] == ["f64"] * (len(s.levels) - 1)
        assert [L.patch_factor_dtype for L in s.levels[1:]] == ["f64"] * (len(s.levels) - 1)
    finally:
        s.close()
    s = _burman_solver(dim, nref, k, macro_factor_dtype="f32")
    try:
        d = s.problem.dim
        u = np.random.default_rng(5).standard_normal(s.n_u)
        u[s.levels[-1].bc_dofs] = 0.0
        s.nu = 0.05
        s._device_states(u)
        big = False
        for L, dl, st, obj in zip(s.levels, s.hmg.mg.levels, s._dstate, s.hmg.pc_objs):
            if obj is None:
                continue
            assert not obj.condensed
            dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
            dl.factor()
            assert dl.patch_storage_dtype() == "f32" and L.patch_factor_dtype == "f32" and dl.condensed() == 0
            big = big or int(np.diff(obj.patch_ptr).max()) > 160
            worst, flagged, repaired, _ = dl.patch_check()
            assert 0.0 <= worst and flagged == repaired
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
                assert np.array_equal(X, np.float32(X).astype(np.float64))          # stored floats, widened
                ref = np.linalg.inv(Ap)
                ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
                assert np.all(np.abs(X - ref) <= 1e-8 * np.abs(ref).max() + ulp), (L.level, p)
            assert ncorr > 0
            pp = np.asarray(obj.patch_ptr)
            x = np.random.default_rng(6).standard_normal(L.n)
            _check_b(_apply(s.ctx, dl, x), _inverses(dl, pp), L, pp, obj.patch_dofs, x, "Burman level %d" % L.level)
        assert big == (dim == "3d")           # the 2-D levels take the small-patch path, the 3-D finest one the big one
    finally:
        s.close()


def test_newton_2d_burman():
    """Reynolds continuation 10 -> 100 on 2-D SV-P2 with Burman weight 5e-3, FP32 against FP64 storage."""
    from alfi_amd.nssolver import run_solver
    res = [10.0, 100.0]
    out, krylov = {}, {None: [], "f32": []}
    for dtype in (None, "f32"):
        s = _burman_solver("2d", 2, 2, macro_factor_dtype=dtype)
        try:
            solve = s.saddle.solve

            def counted(*a, _solve=solve, _its=krylov[dtype], **kw):
                r = _solve(*a, **kw)
                _its.append(r[0])
                return r
            s.saddle.solve = counted
            info = run_solver(s, res)
            out[dtype] = (s.u.copy(), s.p.copy(), info, [L.patch_factor_dtype for L in s.levels[1:]])
        finally:
            s.close()
    (u32, p32, i32, dt32), (_, _, i64, dt64) = out["f32"], out[None]
    assert set(dt32) == {"f32"} and set(dt64) == {"f64"}
    for re in res:
        print("Re %g: Newton f32 %d / f64 %d, Krylov f32 %s / f64 %s"
              % (re, i32[re]["nonlinear_iter"], i64[re]["nonlinear_iter"], i32[re]["linear_iter"], i64[re]["linear_iter"]))
        assert i32[re]["converged"] and i64[re]["converged"]
        assert i32[re]["nonlinear_iter"] == i64[re]["nonlinear_iter"]
    print("Krylov iterations per solve: f32 %s, f64 %s" % (krylov["f32"], krylov[None]))
    assert len(krylov["f32"]) == len(krylov[None])
    assert all(abs(a - b) <= 1 for a, b in zip(krylov["f32"], krylov[None]))
    # the converged state is a root of the host residual, Burman term included
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 2, 2, discretisation="sv", stabilisation_type="burman",
                              stabilisation_weight=5e-3, device_assembly=False)
    try:
        s.nu = s.char_L * s.char_U / res[-1]
        Fu, Fp = s.residual(u32, p32, 1.0)
        F0u, F0p = s.residual(np.zeros_like(u32) + s.u, np.zeros_like(p32), 1.0)
        assert np.sqrt(Fu @ Fu + Fp @ Fp) < 1e-5 * np.sqrt(F0u @ F0u + F0p @ F0p)
    finally:
        s.close()


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
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, build_hierarchy
    L = p2[0][-1]
    x = np.random.default_rng(8).standard_normal(L.n)
    nrow = int(L.patch_ptr[-1]) // L.bs
    no_facets = (1, np.zeros(nrow + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))

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
        fresh().set_macro_patch_storage("f16")
    with pytest.raises(ValueError):
        HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 1, 2, patch_factor_dtype="f32", macro_factor_dtype="f32")
    with pytest.raises(ValueError):
        hip.check_factor_dtypes(None, "f16")
    # --- ALFI_E_ARG, the level stays as it was and works in FP64
    # no patches
    d0 = hip.Level(ctx, L.A, L.bc_dofs)
    d0.set_patches(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    assert "no patches" in _refused(lambda: d0.set_macro_patch_storage("f32"), hip.E_ARG)
    d0.close()
    # small 2-D stars (the interleaved copy)
    lv2, _ = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 1, 2, Re=10.0)
    L2 = lv2[-1]
    assert np.diff(L2.patch_ptr).max() <= 32
    d2 = hip.Level(ctx, L2.A, L2.bc_dofs)
    d2.set_patches(L2.patch_ptr, L2.patch_dofs)
    assert "32" in _refused(lambda: d2.set_macro_patch_storage("f32"), hip.E_ARG)
    d2.factor()
    assert d2.patch_storage_dtype() == "f64"
    d2.close()
    # caller-supplied groups
    dl = fresh()
    dl.set_patch_groups(dl.find_patch_groups())
    assert "groups" in _refused(lambda: dl.set_macro_patch_storage("f32"), hip.E_ARG)
    works_in_f64(dl, ref)
    assert dl.condensed() == 1
    dl.close()
    # multiplicative sweeps
    dl = fresh()
    dl.factor()
    dl.set_multiplicative(np.arange(len(L.patch_ptr) - 1), False)
    assert "multiplicative" in _refused(lambda: dl.set_macro_patch_storage("f32"), hip.E_ARG)
    dl.set_multiplicative(None, False)
    works_in_f64(dl, ref)
    dl.close()
    # --- what the star call refuses and this one accepts: a facet correction before the request (empty lists: it corrects
    # nothing) and a patch above 160 dofs
    dl = fresh()
    dl.set_patch_facet_correction(*no_facets)
    dl.set_macro_patch_storage("f32")
    dl.factor()
    assert dl.patch_storage_dtype() == "f32" and 0 < relerr(_apply(ctx, dl, x), ref) < 1e-6
    dl.close()
    free = np.setdiff1d(np.arange(L.n), L.bc_dofs)
    big = hip.Level(ctx, L.A, L.bc_dofs)
    big.set_patches(np.array([0, 40, 40 + 162]), np.concatenate([free[:40], free[100:262]]).astype(np.int32))
    big.set_macro_patch_storage("f32")
    big.factor()
    assert big.patch_storage_dtype() == "f32"
    big.close()
    # --- on a level asked through this call: ALFI_E_STATE for sweeps and groups, the level stays FP32; a facet correction after
    # the request is accepted and marks the level unfactored; back to FP64 on request, at the next factorisation
    dl = fresh()
    dl.set_macro_patch_storage("f32")
    assert dl.patch_storage_dtype() == "f64"                 # the NEXT factorisation obeys
    assert "FP32" in _refused(lambda: dl.set_multiplicative(np.arange(5), False), hip.E_STATE)
    assert "FP32" in _refused(lambda: dl.set_patch_groups(np.full(int(L.patch_ptr[-1]), -1, dtype=np.int32)), hip.E_STATE)
    dl.factor()
    assert dl.patch_storage_dtype() == "f32" and dl.condensed() == 0
    y32 = _apply(ctx, dl, x)
    assert 0 < relerr(y32, ref) < 1e-6
    for fn in (lambda: dl.set_multiplicative(np.arange(5), False),
               lambda: dl.set_patch_groups(np.full(int(L.patch_ptr[-1]), -1, dtype=np.int32))):
        _refused(fn, hip.E_STATE)
    assert np.array_equal(_apply(ctx, dl, x), y32)
    dl.set_patch_facet_correction(*no_facets)
    _refused(lambda: dl.patch_apply(ctx.vec(x), ctx.vec(L.n)), hip.E_STATE)          # unfactored
    dl.factor()
    assert dl.patch_storage_dtype() == "f32" and np.array_equal(_apply(ctx, dl, x), y32)
    dl.set_macro_patch_storage("f64")
    assert dl.patch_storage_dtype() == "f32" and np.array_equal(_apply(ctx, dl, x), y32)    # until the next factorisation
    works_in_f64(dl, ref)
    dl.set_patches(L.patch_ptr, L.patch_dofs)                # a new patch set starts in FP64
    dl.set_macro_patch_storage("f32")
    dl.set_patches(L.patch_ptr, L.patch_dofs)
    works_in_f64(dl)
    assert dl.set_multiplicative(np.arange(len(L.patch_ptr) - 1), False) >= 1                # and everything is allowed again
    dl.close()


def test_partitioned_levels_take_the_request(ctx, sv3, monkeypatch):
    """A one-rank forced partition of the [P3]^3 hierarchy with ALFI_CONDENSE=0: the rank's finest level takes FP32 and its
    apply -- range launches -- is the serial FP32 level's."""
    from alfi_amd.dist import DistMultigrid
    monkeypatch.setenv("ALFI_CONDENSE", "0")
    lv, tr = sv3
    L = lv[-1]
    x = np.random.default_rng(12).standard_normal(L.n)
    f32 = _level(ctx, L, L.patch_ptr, L.patch_dofs, "f32")
    try:
        y = _apply(ctx, f32, x)
    finally:
        f32.close()
    with pytest.raises(ValueError):
        DistMultigrid(lv, tr, 4, solo=(0, 1), min_dofs=1, force_distributed=True, patch_factor_dtype="f32", macro_factor_dtype="f32")
    dmg = DistMultigrid(lv, tr, 4, solo=(0, 1), min_dofs=1, force_distributed=True, macro_factor_dtype="f32")
    try:
        assert dmg.patch_storage_dtypes()[-1] == "f32" and dmg.patch_storage()[-1][0] == 0
        fin = dmg.local_levels[-1]
        assert fin.patch_factor_dtype == "f32"
        dx, dy = dmg.local_vec(x), dmg.local_vec()
        dmg.levels[-1].patch_apply(dx, dy)
        yr = np.empty(L.n)
        yr[fin.part.own_dofs()] = dmg.owned(dy)
        print("partitioned FP32 macro-star level against the serial one: %.3e" % relerr(yr, y))
        assert relerr(yr, y) < 1e-13
    finally:
        dmg.close()
