"""The block form of the four-launch smoother iteration (csrc/kernels_block_fused.hip; hip.Level.smooth_block on levels where
``smooth_block_mode(k) == 2``).  -m gpu

No tolerance anywhere: column c of ``smooth_block`` equals ``smooth`` on column c BIT FOR BIT, three ways -- with the block
fused form on, with ``Context.set_block_fused(False)`` (these levels loop whole smoother calls, every other block kernel on) and
with ``Context.set_block_kernels(False)`` -- for ncol 1 .. 5 (a chunk of four plus one), a gapped column list with a wider
leading dimension and a sentinel column that stays untouched.  ``smooth_block_mode`` says which way a level goes, so every test
asserts that the path it means to test really ran.

Levels.  The interleaved copy, every G class: the small levels of tests/invert_cases.py (288 dofs, caps 8, 14, 16, 24, 32 -> G 4,
7, 8, 12, 16, patch counts a multiple neither of 64 / G nor of a workgroup's share, sizes 1 .. cap).  The product with dots,
every lanes-per-row class: banded operators of 1003 block rows (tests/block_fused_cases.py; bs 3: 3009 dofs, an odd length for the
paired BLAS-1 loads) with windows of consecutive nodes as patches.  Grid stride: 70 001 block rows of bs 2 (the product's loop
runs twice, 1024 dot partials, 35 norm partials).  Dense stars: the 1003-patch levels of tests/test_gpu_block_rhs.py, one per
waves-per-patch class.  A level that keeps looping: four patches, one of 161 dofs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from tests import block_fused_cases as fc
from tests import invert_cases as ic

SENTINEL = -7.25
WAYS = (("fused", True, True), ("looped", True, False), ("kernels off", False, True))
NPATCH = 1003
CLASSES = {1: (33, 47, 64), 4: (65, 111, 127, 128), 8: (129, 153, 160)}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_block_kernels(True)
    c.set_block_fused(True)
    c.close()


def _way(ctx, kernels, fused):
    ctx.set_block_kernels(kernels)
    ctx.set_block_fused(fused)


def _level(ctx, A, bc, ptr, dofs, pou=False, dtype=None):
    dl = hip.Level(ctx, A, np.asarray(bc, dtype=np.int32))
    dl.set_patches(ptr, dofs)
    dl.set_patch_groups(None)
    if dtype is not None:
        dl.set_patch_storage(dtype)
    if pou:
        dl.set_partition_of_unity(True)
    dl.factor()
    return dl


def _wide(n, extra):
    return ((n + 1) & ~1) + extra


def _single(ctx, dl, k, B, X0, guess):
    ref = np.empty_like(X0)
    for c in range(B.shape[1]):
        db, dx = ctx.vec(B[:, c]), ctx.vec(X0[:, c])
        dl.smooth(k, db, dx, nonzero_guess=guess)
        ref[:, c] = dx.get()
    return ref


def _check(ctx, dl, seed, ks, mode, B=None, X0=None, ncols=(1, 2, 3, 4, 5)):
    """smooth_block against smooth, bitwise, the three ways; mode: what smooth_block_mode reports with everything on"""
    n = dl.n
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, 5)) if B is None else B
    X0 = rng.standard_normal((n, 5)) if X0 is None else X0
    try:
        for k in ks:
            _way(ctx, True, True)
            assert dl.smooth_block_mode(k) == mode, k
            assert not dl.smooth_block_lockstep(k)                 # the old query: "the general path in lockstep" only
            for guess in (False, True):
                ref = _single(ctx, dl, k, B, X0, guess)
                assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
                for name, kernels, fused in WAYS:
                    _way(ctx, kernels, fused)
                    assert dl.smooth_block_mode(k) == (mode if name == "fused" else 0), (k, name)
                    for ncol in ncols:
                        dB, dX = ctx.mat(B[:, :ncol]), ctx.mat(X0[:, :ncol])
                        dl.smooth_block(k, dB, dX, nonzero_guess=guess)
                        assert np.array_equal(dX.get(), ref[:, :ncol]), (k, guess, name, ncol)
                        assert np.array_equal(dB.get(), B[:, :ncol])
                    ld = _wide(n, 6)
                    Xs = X0[:, :4].copy()
                    Xs[:, 1] = SENTINEL
                    dX = ctx.mat(Xs, ld=ld)
                    dl.smooth_block(k, ctx.mat(B[:, :4], ld=_wide(n, 2)), dX, nonzero_guess=guess, cols=[0, 2, 3])
                    got = dX.get()
                    assert np.array_equal(got[:, [0, 2, 3]], ref[:, [0, 2, 3]]) and np.all(got[:, 1] == SENTINEL), (k, guess, name)
                    assert np.all(dX._buf.get().reshape(4, ld)[:, n:] == 0.0)        # nothing written between n and ld
    finally:
        _way(ctx, True, True)


# ---- the interleaved copy: every G class ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 14, 16, 24, 32])
@pytest.mark.parametrize("bs", [2, 3])
def test_every_lane_class_of_the_interleaved_apply(ctx, bs, cap):
    sizes = ic.levels()[cap]
    pw = 64 // ic.il_lanes(cap)
    assert len(sizes) % pw != 0 and len(sizes) % (4 * pw) != 0 and set(sizes) == set(range(1, cap + 1))
    dl = _level(ctx, ic.operator(bs), [], *ic.patch_arrays(sizes))
    try:
        assert not dl.patch_apply_block_batched() and dl.patch_apply_block_width() == 0     # the block apply itself still loops
        assert dl.smooth_block_mode(16) == 1 and dl.smooth_block_lockstep(16)               # k + 1 > 16: the general path
        _check(ctx, dl, 100 * bs + cap, (1, 2, 10, 15), 2)
    finally:
        dl.close()


# ---- the product with dots: every lanes-per-row class ---------------------------------------------------------------------------------
def _banded(ctx, nb, half, bs, count, pou=False, seed=5):
    A = fc.banded_operator(nb, half, bs, seed)
    nodes = 7 if bs == 2 else 5                                    # 14 / 15 dofs: the interleaved copy
    return _level(ctx, A, np.arange(0, 4 * bs), *fc.window_patches(nb, bs, nodes, count, seed + 1), pou=pou)


@pytest.mark.parametrize("bs,half", sorted(fc.BANDS))
def test_every_lane_class_of_the_product_with_dots(ctx, bs, half):
    dl = _banded(ctx, fc.NB, half, bs, 301)
    try:
        assert dl.n == bs * fc.NB
        _check(ctx, dl, 10 * half + bs, (2, 15), 2)                 # 3 and 16 dot vectors at the end: instantiations of 4 and 16
    finally:
        dl.close()


def test_grid_stride_and_many_partials(ctx):
    dl = _banded(ctx, fc.NB_STRIDE, 2, 2, 3001)
    try:
        assert dl.n == 2 * fc.NB_STRIDE > fc.SMALL_N
        _check(ctx, dl, 33, (2,), 2, ncols=(1, 3, 4, 5))
    finally:
        dl.close()


# ---- edge columns -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["il", "band"])
def test_zero_and_identical_columns_with_partition_of_unity(ctx, kind):
    if kind == "il":
        dl = _level(ctx, ic.operator(2), [], *ic.patch_arrays(ic.levels()[14]), pou=True)
    else:
        dl = _banded(ctx, fc.NB, 5, 3, 301, pou=True)
    try:
        n = dl.n
        rng = np.random.default_rng(44)
        B = rng.standard_normal((n, 5))
        B[:, 1] = 0.0                       # a zero right-hand side among non-zero ones
        B[:, 3] = B[:, 0]                   # two identical columns
        X0 = rng.standard_normal((n, 5))
        X0[:, 3] = X0[:, 0]
        _check(ctx, dl, 45, (3,), 2, B=B, X0=X0)
        for guess in (False, True):
            dX = ctx.mat(X0[:, :4])
            dl.smooth_block(3, ctx.mat(B[:, :4]), dX, nonzero_guess=guess)
            got = dX.get()
            assert np.array_equal(got[:, 3], got[:, 0])
            if not guess:
                assert np.all(got[:, 1] == 0.0) and not np.signbit(got[:, 1]).any()
        # all columns zero: f = 0 everywhere, exact zeros
        dX = ctx.mat(X0[:, :3])
        dl.smooth_block(3, ctx.mat(np.zeros((n, 3))), dX, nonzero_guess=False)
        assert np.all(dX.get() == 0.0)
    finally:
        dl.close()


# ---- dense stars of small levels, and a level that keeps looping ------------------------------------------------------------------------
@pytest.mark.parametrize("waves,dtype", [(1, "f64"), (4, "f64"), (8, "f64"), (4, "f32")])
def test_dense_star_small_levels(ctx, waves, dtype):
    s = CLASSES[waves]
    sizes = [s[i % len(s)] for i in range(NPATCH)]
    dl = _level(ctx, ic.operator(3), [], *ic.patch_arrays(sizes), dtype=None if dtype == "f64" else dtype)
    try:
        assert dl.patch_storage_dtype() == dtype and dl.patch_apply_block_width() == 4
        _check(ctx, dl, 60 + waves, (1, 10), 2)
    finally:
        dl.close()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_macro_star_levels_in_pieces(ctx, name):
    """the levels of tests/block_big_cases.py (8 patches, 2736 dofs): width 4 is one piece; width 3 takes four columns as 3 + 1 and
    width 2 takes three as 2 + 1 -- the one-column piece goes through the single apply into the level's own staging buffer"""
    from tests import block_big_cases as bc
    dl = _level(ctx, bc.operator(), [], *bc.patch_arrays(bc.LEVELS[name]))
    try:
        assert dl.condensed() == 0 and dl.patch_apply_block_width() == bc.EXPECTED[name][1] == {"A": 4, "B": 3, "C": 2}[name]
        _check(ctx, dl, 75, (3,), 2)
    finally:
        dl.close()


def test_a_level_of_few_macro_stars_keeps_looping(ctx):
    dl = _level(ctx, ic.operator(3), [], *ic.patch_arrays((40, 161, 100, 77)))
    try:
        assert not dl.patch_apply_block_batched()
        _check(ctx, dl, 70, (1, 10), 0)
    finally:
        dl.close()


# ---- launches per iteration do not depend on the number of columns -----------------------------------------------------------------------
def test_launch_counts_are_those_of_one_column(ctx):
    dl = _level(ctx, ic.operator(2), [], *ic.patch_arrays(ic.levels()[14]))
    classes = ("PATCH_APPLY", "PATCH_SCATTER", "MATMULT")
    try:
        n, k = dl.n, 6
        B = np.random.default_rng(80).standard_normal((n, 4))
        ctx.prof_enable(True)

        def counts(fn):
            ctx.prof_reset()
            fn()
            ctx.sync()
            got = ctx.prof_get(dl.id)
            return {c: got[c][1] for c in classes}

        one = counts(lambda: dl.smooth(k, ctx.vec(B[:, 0]), ctx.vec(n), nonzero_guess=False))
        assert one == {c: k for c in classes}, one
        _way(ctx, True, True)
        assert dl.smooth_block_mode(k) == 2
        assert counts(lambda: dl.smooth_block(k, ctx.mat(B), ctx.mat(n, 4), nonzero_guess=False)) == one
        _way(ctx, True, False)
        assert dl.smooth_block_mode(k) == 0
        assert counts(lambda: dl.smooth_block(k, ctx.mat(B), ctx.mat(n, 4), nonzero_guess=False)) == {c: 4 * k for c in classes}
    finally:
        ctx.prof_enable(False)
        _way(ctx, True, True)
        dl.close()


# ---- workspaces across a new patch set, a refactorisation and new operator values ------------------------------------------------------
def test_workspaces_follow_the_level(ctx):
    A = ic.operator(3)
    dl = _level(ctx, A, [], *ic.patch_arrays(ic.levels()[14]))
    try:
        _check(ctx, dl, 90, (4,), 2, ncols=(4,))
        dl.set_patches(*ic.patch_arrays(ic.levels()[32]))          # another staging length, another lane class
        dl.set_patch_groups(None)
        dl.factor()
        _check(ctx, dl, 91, (4,), 2, ncols=(2, 4))
        dl.update_values(1.25 * A.vals)
        dl.factor()
        _check(ctx, dl, 92, (6,), 2, ncols=(3, 4))                 # a larger k too: the Krylov workspace is allocated again
    finally:
        dl.close()


# ---- hierarchies ----------------------------------------------------------------------------------------------------------------------------
def test_block_cycles_of_a_2d_hierarchy(ctx):
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, build_hierarchy
    lv, tr = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 1, 2, Re=100.0)
    mg = hip.Multigrid(ctx, lv, tr, 2)
    try:
        assert len(mg.levels) >= 2 and all(L.smooth_block_mode(2) == 2 for L in mg.levels[1:])
        n = lv[-1].n
        B = np.random.default_rng(12).standard_normal((n, 5))
        B[lv[-1].bc_dofs] = 0.0
        refv, reff = np.empty_like(B), np.empty_like(B)
        for c in range(5):
            db, dx = ctx.vec(B[:, c]), ctx.vec(n)
            mg.vcycle(db, dx)
            refv[:, c] = dx.get()
            mg.fcycle(db, dx)
            reff[:, c] = dx.get()
        for name, kernels, fused in WAYS:
            _way(ctx, kernels, fused)
            dB, dX = ctx.mat(B), ctx.mat(n, 5)
            mg.vcycle_block(dB, dX)
            assert np.array_equal(dX.get(), refv), name
            mg.fcycle_block(dB, dX)
            assert np.array_equal(dX.get(), reff), name
            dX = ctx.mat(np.full((n, 5), SENTINEL), ld=_wide(n, 4))
            mg.fcycle_block(dB, dX, cols=[4, 0, 2])
            got = dX.get()
            assert np.array_equal(got[:, [0, 2, 4]], reff[:, [0, 2, 4]]) and np.all(got[:, [1, 3]] == SENTINEL), name
    finally:
        _way(ctx, True, True)
        mg.close()


def test_adjoint_list_of_a_2d_solver():
    from alfi_amd.adjoint import LinearFunctional, LoadFunctional
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem

    def weight(x):
        w = np.zeros_like(x)
        w[:, 0] = np.cos(0.5 * np.pi * x[:, 1])
        w[:, 1] = 1.0 + x[:, 0] * x[:, 1]
        return w

    def force(x):
        f = np.zeros_like(x)
        f[:, 0] = np.sin(np.pi * x[:, 1]) + 0.5 * x[:, 0] * x[:, 0]
        f[:, 1] = np.sin(np.pi * x[:, 0]) + 0.5 * x[:, 1] * x[:, 1]
        return f

    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2)
    try:
        _, info = s.solve(10.0)
        assert info["converged"]
        g_p = np.random.default_rng(5).standard_normal(s.n_p) + 0.2
        Js = [LoadFunctional(weight), LinearFunctional(LoadFunctional(force).gradient(s, s.u, s.p)[0], g_p), LoadFunctional(force)]
        single = []
        for J in Js:
            z, inf = s.solve_adjoint(J, rtol=1e-10, atol=0.0)
            assert inf["converged"] and inf["linear_iter"] > 0
            single.append((z[0].copy(), z[1].copy(), inf["linear_iter"]))
        for fused in (True, False):
            s.ctx.set_block_fused(fused)
            k = s.hmg.mg.k
            assert all(L.smooth_block_mode(k) == (2 if fused else 0) for L in s.hmg.mg.levels[1:])
            z, inf = s.solve_adjoint(Js, rtol=1e-10, atol=0.0)
            for i in range(3):
                assert np.array_equal(z[i][0], single[i][0]) and np.array_equal(z[i][1], single[i][1]), (fused, i)
            assert inf["linear_iter"] == [t[2] for t in single]
    finally:
        s.ctx.set_block_fused(True)
        s.close()
