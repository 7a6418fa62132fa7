"""Block right-hand sides (alfi_*_block; hip.Level.patch_apply_block / spmv_block / residual_block / smooth_block,
hip.Multigrid.vcycle_block / fcycle_block).  -m gpu

The contract needs no tolerance: column c of every block result equals the single-vector call on column c BIT FOR BIT, whether
the level batches (one launch streams the stored values once for up to four columns) or loops, and with the batched kernels
switched off (Context.set_block_kernels).  ``patch_apply_block_batched`` / ``spmv_block_batched`` say which way a level goes, so
every test asserts that the path it means to test really ran.

Levels.  Dense stars: the synthetic levels of tests/invert_cases.py (a 288-dof operator, patch n = the fixed dof subset D_n), 1003
patches each -- above the 1000 below which the single apply takes its few-patches detours -- with the sizes of one
waves-per-patch class per level: {33, 47, 64} one wave, {65, 111, 127, 128} four, {129, 153, 160} eight (odd n = a pad row,
single-digit row pieces, a full 128-row piece plus a remainder).  Looped applies: every patch <= 24 dofs (the interleaved copy), one
patch above 160 dofs (macro stars' kernel), the condensed [P2+FB]^3 stars of ldc3d.  Products: the dense synthetic operators
(bs 3: 9216 blocks = 144 value groups, 96 blocks per row, 48 whole-row chunks; bs 2: 20 736 blocks) and, for the carry and
fix-up launch, operators whose first block row is longer than a chunk of 256 blocks (3 .. 4 chunks, under the 1024 blocks from
which the product de-duplicates its columns and loops).  Smoother, general path: a banded bs-3 operator of 50 100 dofs with 33
blocks per row (above the 50 000 dofs / 32 blocks up to which the single smoother takes its four-launch iteration) with 1100
windows of 111 consecutive dofs as patches; the four-launch path: the synthetic 288-dof level (``smooth_block_lockstep`` says
which of the two a level takes).  Outer solve and adjoints: the Newton solvers of tests/test_gpu_adjoint.py after a converged
forward solve -- Saddle.mult_block / precond_block / solve_block against one call per column, solve_adjoint of a list of
functionals against one solve_adjoint per functional; a one-rank forced partition for the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from alfi_amd.problem import BSR
from tests import invert_cases as ic

NPATCH = 1003
CLASSES = {1: (33, 47, 64), 4: (65, 111, 127, 128), 8: (129, 153, 160)}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_block_kernels(True)
    c.close()


def _synthetic(ctx, bs, sizes, dtype=None, pou=False):
    dl = hip.Level(ctx, ic.operator(bs), np.zeros(0, dtype=np.int32))
    dl.set_patches(*ic.patch_arrays(sizes))
    dl.set_patch_groups(None)
    if dtype is not None:
        dl.set_patch_storage(dtype)
    if pou:
        dl.set_partition_of_unity(True)
    dl.factor()
    return dl


def _class_sizes(waves):
    s = CLASSES[waves]
    return [s[i % len(s)] for i in range(NPATCH)]


def _single_columns(ctx, fn, X, *more):
    """fn(x, [b, ...], y) column by column on device vectors -> (n, ncol) array"""
    out = np.empty_like(X)
    for c in range(X.shape[1]):
        dy = ctx.vec(X.shape[0])
        fn(*([ctx.vec(M[:, c]) for M in (X,) + more] + [dy]))
        out[:, c] = dy.get()
    return out


SENTINEL = -7.25


def _wide(n, extra):
    """a leading dimension above the default one: n rounded up to even, plus an even extra"""
    return ((n + 1) & ~1) + extra


def _check_block_apply(ctx, dl, rng, want_batched):
    """patch_apply_block against patch_apply, bitwise: ncol 1 .. 5, a gapped list with a wider leading dimension"""
    n = dl.n
    assert dl.patch_apply_block_batched() == want_batched
    X = rng.standard_normal((n, 5))
    ref = _single_columns(ctx, dl.patch_apply, X)
    for ncol in (1, 2, 3, 4, 5):
        dX, dY = ctx.mat(X[:, :ncol]), ctx.mat(n, ncol)
        dl.patch_apply_block(dX, dY)
        assert np.array_equal(dY.get(), ref[:, :ncol]), ncol
        assert np.array_equal(dX.get(), X[:, :ncol])                   # x is not modified
    ld = _wide(n, 6)
    dX, dY = ctx.mat(X[:, :4], ld=ld), ctx.mat(np.full((n, 4), SENTINEL), ld=ld)
    dl.patch_apply_block(dX, dY, cols=[0, 2, 3])
    Y = dY.get()
    assert np.array_equal(Y[:, [0, 2, 3]], ref[:, [0, 2, 3]]) and np.all(Y[:, 1] == SENTINEL)
    assert np.all(dY._buf.get().reshape(4, ld)[:, n:] == 0.0)       # nothing written between n and ld
    dl.patch_apply_block(dX, dY, cols=[3, 1])                          # any order
    Y = dY.get()
    assert np.array_equal(Y[:, [1, 3]], ref[:, [1, 3]])
    return X, ref


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("waves", sorted(CLASSES))
def test_block_apply_of_dense_stars_is_the_single_apply(ctx, waves, dtype):
    sizes = _class_sizes(waves)
    dl = _synthetic(ctx, 3, sizes, None if dtype == "f64" else dtype)
    try:
        assert dl.patch_storage_dtype() == dtype and dl.condensed() == 0
        X, ref = _check_block_apply(ctx, dl, np.random.default_rng(waves), True)
        # the same bits with the batched kernels switched off
        ctx.set_block_kernels(False)
        assert not dl.patch_apply_block_batched()
        dX, dY = ctx.mat(X), ctx.mat(dl.n, 5)
        dl.patch_apply_block(dX, dY)
        assert np.array_equal(dY.get(), ref)
        ctx.set_block_kernels(True)
        assert dl.patch_apply_block_batched()
        # and against NumPy, at the tolerance tests/test_gpu_parity.py has for alfi_patch_apply (1e-7 of the max-norm)
        inv = {m: dl.patch_inverse(sizes.index(m), m) for m in set(sizes)}
        host = np.zeros_like(X)
        for m in sizes:
            host[ic.dofs(m)] += inv[m] @ X[ic.dofs(m)]
        assert np.abs(ref - host).max() < 1e-7 * np.abs(host).max()
    finally:
        ctx.set_block_kernels(True)
        dl.close()


def test_block_apply_with_partition_of_unity(ctx):
    dl = _synthetic(ctx, 2, _class_sizes(4), pou=True)
    plain = _synthetic(ctx, 2, _class_sizes(4))
    try:
        X, ref = _check_block_apply(ctx, dl, np.random.default_rng(11), True)
        dY = ctx.mat(dl.n, 5)
        plain.patch_apply_block(ctx.mat(X), dY)
        assert not np.array_equal(dY.get(), ref)                       # the flag did something
    finally:
        dl.close()
        plain.close()


def test_looped_applies_are_the_single_apply(ctx):
    """the interleaved copy (every patch <= 24 dofs), a level with a patch above 160 dofs, 200 patches above 64 dofs (the macro
    stars' kernel): batched == 0, same bits"""
    for sizes in (ic.levels()[24], (40, 161, 100, 77), _class_sizes(8)[:200]):
        dl = _synthetic(ctx, 3, list(sizes))
        try:
            _check_block_apply(ctx, dl, np.random.default_rng(len(sizes)), False)
        finally:
            dl.close()


def test_few_patches_above_256_batch_with_eight_waves(ctx):
    """257 .. 1000 patches above 64 dofs: the single apply gives every patch eight waves whatever its size, and so does the block"""
    dl = _synthetic(ctx, 3, _class_sizes(4)[:300])
    try:
        _check_block_apply(ctx, dl, np.random.default_rng(3), True)
    finally:
        dl.close()


def test_condensed_level_loops(ctx):
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    lv, _ = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 2, Re=1000.0)
    L = lv[-1]
    cctx = hip.Context(0)
    cctx.set_condense_min_bytes(0)
    dl = hip.Level(cctx, L.A, L.bc_dofs)
    try:
        dl.set_patches(L.patch_ptr, L.patch_dofs)
        dl.factor()
        assert dl.condensed() == 2
        _check_block_apply(cctx, dl, np.random.default_rng(4), False)
    finally:
        dl.close()
        cctx.close()


# ---- products -----------------------------------------------------------------------------------------------------------------------
def _long_first_row(bs, seed):
    """block rows: row 0 with 300 blocks (longer than a chunk of 256), then 200 rows of 3 blocks: 900 blocks = 4 chunks"""
    rng = np.random.default_rng(seed)
    nb = 300
    rows = [np.arange(nb)] + [np.sort(rng.choice(nb, 3, replace=False)) for _ in range(200)] + [np.array([i]) for i in range(201, nb)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colidx = np.concatenate(rows).astype(np.int32)
    return BSR(nb, nb, bs, rowptr, colidx, rng.standard_normal((len(colidx), bs, bs)))


@pytest.mark.parametrize("bs", [2, 3])
@pytest.mark.parametrize("kind", ["whole-row chunks", "carry and fix-up"])
def test_block_product_and_residual_are_the_single_ones(ctx, bs, kind):
    A = ic.operator(bs) if kind == "whole-row chunks" else _long_first_row(bs, bs)
    assert A.nnzb > 256
    dl = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
    try:
        n = dl.n
        assert dl.spmv_block_batched()
        rng = np.random.default_rng(bs)
        X, B = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
        y = _single_columns(ctx, dl.spmv, X)
        r = _single_columns(ctx, lambda x, b, out: dl.residual(b, x, out), X, B)
        S = A.to_scipy()
        assert np.abs(y - S @ X).max() < 1e-13 * np.abs(S @ X).max()
        for on in (True, False):
            ctx.set_block_kernels(on)
            assert dl.spmv_block_batched() == on
            for ncol in (1, 2, 3, 4, 5):
                dX, dB, dY = ctx.mat(X[:, :ncol]), ctx.mat(B[:, :ncol]), ctx.mat(n, ncol)
                dl.spmv_block(dX, dY)
                assert np.array_equal(dY.get(), y[:, :ncol]), (on, ncol)
                dl.residual_block(dB, dX, dY)
                assert np.array_equal(dY.get(), r[:, :ncol]), (on, ncol)
            dX, dB = ctx.mat(X[:, :4], ld=_wide(n, 6)), ctx.mat(B[:, :4], ld=_wide(n, 2))
            dY = ctx.mat(np.full((n, 4), SENTINEL), ld=_wide(n, 4))
            dl.residual_block(dB, dX, dY, cols=[0, 2, 3])
            Y = dY.get()
            assert np.array_equal(Y[:, [0, 2, 3]], r[:, [0, 2, 3]]) and np.all(Y[:, 1] == SENTINEL)
            dl.spmv_block(dX, dY, cols=[1, 3])
            assert np.array_equal(dY.get()[:, [1, 3]], y[:, [1, 3]])
    finally:
        ctx.set_block_kernels(True)
        dl.close()


# ---- smoother -------------------------------------------------------------------------------------------------------------------------
def _banded_level(ctx):
    """16 700 block rows of bs 3 (50 100 dofs), block columns i - 16 .. i + 16, diagonally dominant; patches: 1100 windows of 37
    consecutive nodes (111 dofs)"""
    nb, half, bs = 16700, 16, 3
    rng = np.random.default_rng(77)
    cols = np.arange(nb)[:, None] + np.arange(-half, half + 1)[None, :]
    ok = (cols >= 0) & (cols < nb)
    rowptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int32)
    colidx = cols[ok].astype(np.int32)
    vals = 0.05 * rng.standard_normal((len(colidx), bs, bs))
    diag = colidx == np.repeat(np.arange(nb), ok.sum(axis=1))
    vals[diag] += 4.0 * np.eye(bs)
    A = BSR(nb, nb, bs, rowptr, colidx, vals)
    bc = np.arange(0, 30, dtype=np.int32)
    dl = hip.Level(ctx, A, bc)
    starts = np.sort(rng.integers(10, nb - 37, 1100))
    ptr = (111 * np.arange(1101)).astype(np.int64)
    dofs = (3 * starts[:, None] + np.arange(111)[None, :]).ravel().astype(np.int32)
    dl.set_patches(ptr, dofs)
    dl.set_patch_groups(None)
    dl.factor()
    return dl


@pytest.fixture(scope="module")
def banded(ctx):
    dl = _banded_level(ctx)
    yield dl
    dl.close()


def _check_smoother(ctx, dl, seed):
    n = dl.n
    rng = np.random.default_rng(seed)
    B, X0 = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
    for k in (1, 10):
        for guess in (False, True):
            ref = np.empty((n, 5))
            for c in range(5):
                db, dx = ctx.vec(B[:, c]), ctx.vec(X0[:, c])
                dl.smooth(k, db, dx, nonzero_guess=guess)
                ref[:, c] = dx.get()
            for on in (True, False):
                ctx.set_block_kernels(on)
                dB, dX = ctx.mat(B), ctx.mat(X0)
                dl.smooth_block(k, dB, dX, nonzero_guess=guess)
                assert np.array_equal(dX.get(), ref), (k, guess, on)
                dX = ctx.mat(X0[:, :4], ld=_wide(n, 2))
                dl.smooth_block(k, ctx.mat(B[:, :4]), dX, nonzero_guess=guess, cols=[0, 2, 3])
                got = dX.get()
                assert np.array_equal(got[:, [0, 2, 3]], ref[:, [0, 2, 3]]) and np.array_equal(got[:, 1], X0[:, 1]), (k, guess, on)
            ctx.set_block_kernels(True)
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0


def test_block_smoother_general_path(ctx, banded):
    assert banded.patch_apply_block_batched() and banded.spmv_block_batched()
    assert banded.smooth_block_lockstep(1) and banded.smooth_block_lockstep(10)      # not the loop over whole smoother calls
    _check_block_apply(ctx, banded, np.random.default_rng(8), True)        # Dirichlet rows: y[bc] = x[bc] in every column
    _check_smoother(ctx, banded, 9)


def test_block_smoother_on_a_level_of_the_four_launch_iteration(ctx):
    dl = _synthetic(ctx, 3, _class_sizes(4))
    try:
        assert not dl.smooth_block_lockstep(1) and not dl.smooth_block_lockstep(10)
        assert dl.smooth_block_lockstep(16)          # k + 1 > 16: the single call leaves the four-launch iteration
        _check_smoother(ctx, dl, 10)
    finally:
        dl.close()


# ---- cycles ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ldc3d", "ldc2d"])
def test_block_cycles_are_the_single_cycles(ctx, case):
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem, build_hierarchy
    prob = ThreeDimLidDrivenCavityProblem(2) if case == "ldc3d" else TwoDimLidDrivenCavityProblem(4)
    lv, tr = build_hierarchy(prob, 1, 2, Re=100.0)
    mg = hip.Multigrid(ctx, lv, tr, 2)
    try:
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
        for on in (True, False):
            ctx.set_block_kernels(on)
            dB, dX = ctx.mat(B), ctx.mat(n, 5)
            mg.vcycle_block(dB, dX)
            assert np.array_equal(dX.get(), refv), (case, on)
            mg.fcycle_block(dB, dX)
            assert np.array_equal(dX.get(), reff), (case, on)
            dX = ctx.mat(np.full((n, 5), SENTINEL), ld=_wide(n, 4))
            mg.fcycle_block(dB, dX, cols=[4, 0, 2])
            got = dX.get()
            assert np.array_equal(got[:, [0, 2, 4]], reff[:, [0, 2, 4]]) and np.all(got[:, [1, 3]] == SENTINEL)
    finally:
        ctx.set_block_kernels(True)
        mg.close()


def test_mat_apply_of_the_plug_ins_is_apply_per_column(ctx):
    """HipPatchPC.matApply / HipMG.matApply (PETSc's PCMatApply shape: dense host matrices, one column per right-hand side)"""
    import alfi_amd
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    lv, tr = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 1, Re=100.0)
    mg = alfi_amd.HipMG(ctx, lv, tr, alfi_amd.fieldsplit_0_mg(alfi_amd.mg_levels_solver(3, smoothing=3)))
    try:
        n = lv[-1].n
        X = np.random.default_rng(14).standard_normal((n, 3))
        X[lv[-1].bc_dofs] = 0.0
        Y, Z = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
        mg.pc_objs[-1].matApply(mg.pcs[-1], X, Y)
        mg.matApply(X, Z)
        for c in range(3):
            y, z = np.zeros(n), np.zeros(n)
            mg.pc_objs[-1].apply(mg.pcs[-1], X[:, c].copy(), y)
            mg.apply(X[:, c].copy(), z)
            assert np.array_equal(Y[:, c], y) and np.array_equal(Z[:, c], z), c
        with pytest.raises(ValueError):
            mg.matApply(X, X)
        with pytest.raises(ValueError):
            mg.pc_objs[-1].matApply(mg.pcs[-1], X, np.zeros((n, 2)))
    finally:
        mg.mg.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(hip.AlfiHipError) as e:
        fn()
    assert e.value.code == hip.E_ARG, str(e.value)


def test_refusals_leave_everything_untouched(ctx):
    dl = _synthetic(ctx, 3, _class_sizes(1)[:40])
    try:
        n = dl.n
        X = np.random.default_rng(13).standard_normal((n, 4))
        dX, dY = ctx.mat(X), ctx.mat(np.full((n, 4), SENTINEL))
        lib, h = ctx.lib, dl.h
        i32 = lambda *a: np.array(a, dtype=np.int32)
        calls = {
            "ncol 0": lambda c: lib.alfi_patch_apply_block(h, 0, None, 4, dX.ptr, dX.ld, dY.ptr, dY.ld),
            "ncol > nx": lambda c: lib.alfi_patch_apply_block(h, 5, None, 4, dX.ptr, dX.ld, dY.ptr, dY.ld),
            "odd ldx": lambda c: lib.alfi_patch_apply_block(h, 2, None, 2, dX.ptr, dX.ld + 1, dY.ptr, dY.ld),
            "ldy < n": lambda c: lib.alfi_patch_apply_block(h, 2, None, 2, dX.ptr, dX.ld, dY.ptr, n - 2),
            "column 4 of 4": lambda c: lib.alfi_patch_apply_block(h, 2, hip._ptr(c), 4, dX.ptr, dX.ld, dY.ptr, dY.ld),
            "X is Y": lambda c: lib.alfi_patch_apply_block(h, 2, None, 4, dX.ptr, dX.ld, dX.ptr, dX.ld),
            "spmv X is Y": lambda c: lib.alfi_spmv_block(h, 2, None, 4, dX.ptr, dX.ld, dX.ptr, dX.ld),
            "residual ldr": lambda c: lib.alfi_residual_block(h, 2, None, 4, dX.ptr, dX.ld, dX.ptr, dX.ld, dY.ptr, dY.ld + 1),
            "smoother b is x": lambda c: lib.alfi_smooth_fgmres_block(h, 2, 2, None, 4, dX.ptr, dX.ld, dX.ptr, dX.ld, 1),
        }
        bad = i32(1, 4)
        for name, call in calls.items():
            assert call(bad) == hip.E_ARG, name
        assert lib.alfi_patch_apply_block(h, 2, hip._ptr(i32(1, 1)), 4, dX.ptr, dX.ld, dY.ptr, dY.ld) == hip.E_ARG   # listed twice
        assert lib.alfi_patch_apply_block(h, 2, hip._ptr(i32(-1, 1)), 4, dX.ptr, dX.ld, dY.ptr, dY.ld) == hip.E_ARG
        assert np.array_equal(dX.get(), X) and np.all(dY.get() == SENTINEL)
        # the Python wrappers raise the same code
        _refused(lambda: dl.patch_apply_block(dX, dY, cols=[0, 4]))
        _refused(lambda: dl.patch_apply_block(dX, dX))
        _refused(lambda: dl.patch_apply_block(dX, dY, cols=[]))
        # the level still applies, in blocks and singly
        ref = _single_columns(ctx, dl.patch_apply, X)
        dl.patch_apply_block(dX, dY)
        assert np.array_equal(dY.get(), ref)
    finally:
        dl.close()
    # a partitioned level (one rank, every node owned, no neighbour): every block entry point refuses, the single call works
    dl = hip.Level(ctx, ic.operator(3), np.zeros(0, dtype=np.int32))
    try:
        assert dl.spmv_block_batched()
        y = _single_columns(ctx, dl.spmv, X)
        dl.set_partition(n // 3, False, np.zeros(0, dtype=np.int32), None, None, 0)
        dY = ctx.mat(np.full((n, 4), SENTINEL))
        for fn in (lambda: dl.patch_apply_block(dX, dY), lambda: dl.spmv_block(dX, dY), lambda: dl.residual_block(dX, dX, dY),
                   lambda: dl.smooth_block(2, dX, dY)):
            _refused(fn)
        assert np.all(dY.get() == SENTINEL) and not dl.patch_apply_block_batched() and not dl.spmv_block_batched()
        assert np.array_equal(_single_columns(ctx, dl.spmv, X), y)
    finally:
        dl.close()


# ---- outer solve and adjoints -----------------------------------------------------------------------------------------------------------
def _ns_solver(case, **kw):
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    if case == "pkp0-2d":
        return HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2, **kw)
    if case == "pkp0-3d-k1":
        return HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 1, **kw)
    assert case == "sv-2d-burman"
    return HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(2), 2, 2, discretisation="sv", stabilisation_type="burman",
                                 stabilisation_weight=5e-3, **kw)


def _weight(x):
    w = np.zeros_like(x)
    w[:, 0] = np.cos(0.5 * np.pi * x[:, 1])
    w[:, 1] = 1.0 + x[:, 0] * x[:, 1]
    return w


def _force(x):
    d = x.shape[1]
    f = np.zeros_like(x)
    for i in range(d):
        f[:, i] = np.sin(np.pi * x[:, (i + 1) % d]) + 0.5 * x[:, i] * x[:, (i + 2) % d]
    return f


@pytest.mark.parametrize("case", ["pkp0-2d", "pkp0-3d-k1"])
def test_saddle_block_calls_are_the_single_calls(case):
    """Saddle.mult_block / precond_block / solve_block on the operators of a converged Newton step.  Right-hand sides of
    different difficulty: a random one, a copy of it scaled by 1e-4 (the absolute tolerance then asks for three digits only), a
    second random one, a zero column and a fifth column (a second chunk).  Iterations, true residual norms and solutions are
    those of one ``solve`` per column, bit for bit; with restart 4 (restarts are crossed where a column needs more than four
    iterations) and with max_it one below the slowest column's count (the limit is met) too."""
    s = _ns_solver(case)
    try:
        _, info = s.solve(10.0)
        assert info["converged"]
        sad, ctx, n, nu = s.saddle, s.ctx, s.n_u + s.n_p, s.n_u
        rng = np.random.default_rng(21)
        B = rng.standard_normal((n, 5))
        B[s.levels[-1].bc_dofs] = 0.0
        B[nu:] -= B[nu:].mean(axis=0)
        B[:, 1] = 1e-4 * B[:, 0]
        B[:, 3] = 0.0
        # products and preconditioner applications
        ym, yp = np.empty_like(B), np.empty_like(B)
        for c in range(5):
            dx, dy = ctx.vec(B[:, c]), ctx.vec(n)
            sad.mult(dx, dy)
            ym[:, c] = dy.get()
            sad.precond(dx, dy)
            yp[:, c] = dy.get()
        for on in (True, False):
            ctx.set_block_kernels(on)
            dB, dY = ctx.mat(B), ctx.mat(n, 5)
            sad.mult_block(dB, dY)
            assert np.array_equal(dY.get(), ym), on
            sad.precond_block(dB, dY)
            assert np.array_equal(dY.get(), yp), on
            dY = ctx.mat(np.full((n, 5), SENTINEL), ld=_wide(n, 2))
            sad.precond_block(dB, dY, cols=[4, 0, 2])
            got = dY.get()
            assert np.array_equal(got[:, [0, 2, 4]], yp[:, [0, 2, 4]]) and np.all(got[:, [1, 3]] == SENTINEL)
        ctx.set_block_kernels(True)
        # solves
        atol = 1e-7 * np.linalg.norm(B[:, 0])
        slowest = None
        for restart, max_it in ((30, 200), (4, 200), (4, None)):
            max_it = slowest - 1 if max_it is None else max_it
            ref = []
            for c in range(5):
                db, dx = ctx.vec(B[:, c]), ctx.vec(n)
                its, rn = sad.solve(db, dx, 1e-6, atol, max_it, restart)
                ref.append((its, rn, dx.get()))
            assert ref[3][0] == 0 and np.all(ref[3][2] == 0.0)                      # the zero column
            if max_it == 200:
                assert len({r[0] for r in ref[:3]}) > 1, [r[0] for r in ref]         # the columns converge at different iterations
                assert ref[1][0] < ref[0][0]
                slowest = max(r[0] for r in ref)
                assert slowest >= 2
            else:
                assert max(r[0] for r in ref) == max_it
            for on in (True, False):
                ctx.set_block_kernels(on)
                dB, dX = ctx.mat(B), ctx.mat(np.full((n, 5), SENTINEL))
                its, rn = sad.solve_block(dB, dX, 1e-6, atol, max_it, restart)
                X = dX.get()
                assert its == [r[0] for r in ref], (restart, max_it, on, its)
                assert rn == [r[1] for r in ref], (restart, max_it, on)
                for c in range(5):
                    assert np.array_equal(X[:, c], ref[c][2]), (restart, max_it, on, c)
            ctx.set_block_kernels(True)
            dX = ctx.mat(np.full((n, 5), SENTINEL), ld=_wide(n, 4))
            its, rn = sad.solve_block(ctx.mat(B), dX, 1e-6, atol, max_it, restart, cols=[2, 1])
            X = dX.get()
            assert its == [ref[2][0], ref[1][0]] and rn == [ref[2][1], ref[1][1]]
            assert np.array_equal(X[:, 2], ref[2][2]) and np.array_equal(X[:, 1], ref[1][2]) and np.all(X[:, [0, 3, 4]] == SENTINEL)
        # refusals: ALFI_E_ARG, nothing written
        dB, dX = ctx.mat(B), ctx.mat(np.full((n, 5), SENTINEL))
        lib, h = ctx.lib, sad.h
        its, rn = np.zeros(5, dtype=np.int32), np.zeros(5)
        args = (1e-6, atol, 10, 30, hip._ptr(its), hip._ptr(rn))
        assert lib.alfi_saddle_solve_block(h, 0, None, 5, dB.ptr, dB.ld, dX.ptr, dX.ld, *args) == hip.E_ARG
        assert lib.alfi_saddle_solve_block(h, 2, None, 5, dB.ptr, dB.ld + 1, dX.ptr, dX.ld, *args) == hip.E_ARG
        assert lib.alfi_saddle_solve_block(h, 2, None, 5, dB.ptr, dB.ld, dX.ptr, n - 2, *args) == hip.E_ARG
        assert lib.alfi_saddle_solve_block(h, 2, hip._ptr(np.array([0, 5], dtype=np.int32)), 5, dB.ptr, dB.ld, dX.ptr, dX.ld,
                                           *args) == hip.E_ARG
        assert lib.alfi_saddle_solve_block(h, 2, None, 5, dB.ptr, dB.ld, dB.ptr, dB.ld, *args) == hip.E_ARG
        assert lib.alfi_saddle_solve_block(h, 2, None, 5, dB.ptr, dB.ld, dX.ptr, dX.ld, 1e-6, atol, 10, 0, hip._ptr(its),
                                           hip._ptr(rn)) == hip.E_ARG
        assert lib.alfi_saddle_mult_block(h, 2, None, 5, dB.ptr, dB.ld, dB.ptr, dB.ld) == hip.E_ARG
        assert lib.alfi_saddle_precond_block(h, 6, None, 5, dB.ptr, dB.ld, dX.ptr, dX.ld) == hip.E_ARG
        assert np.all(dX.get() == SENTINEL) and np.array_equal(dB.get(), B)
    finally:
        s.ctx.set_block_kernels(True)
        s.close()


@pytest.mark.parametrize("case", ["pkp0-2d", "sv-2d-burman"])
def test_adjoint_of_a_list_of_functionals(case):
    """solve_adjoint([J1, J2, J3]): every z_adj[i] and its counts bitwise those of solve_adjoint(Ji); refresh, transpose and
    factor times are reported once; a single functional keeps its types."""
    from alfi_amd.adjoint import LinearFunctional, LoadFunctional, gradient
    s = _ns_solver(case)
    try:
        for re in (10.0, 50.0):
            _, info = s.solve(re)
            assert info["converged"]
        g_p = np.random.default_rng(5).standard_normal(s.n_p) + 0.2
        Js = [LoadFunctional(_weight), LinearFunctional(LoadFunctional(_force).gradient(s, s.u, s.p)[0], g_p), LoadFunctional(_force)]
        single = []
        for J in Js:
            z, inf = s.solve_adjoint(J, rtol=1e-10, atol=0.0)
            assert isinstance(z, tuple) and isinstance(inf["linear_iter"], int) and isinstance(inf["converged"], bool)
            assert inf["converged"] and inf["linear_iter"] > 0
            single.append((z[0].copy(), z[1].copy(), inf))
        z, inf = s.solve_adjoint(Js, rtol=1e-10, atol=0.0)
        assert isinstance(z, list) and len(z) == 3 and z is s.z_adj
        for i in range(3):
            assert np.array_equal(z[i][0], single[i][0]) and np.array_equal(z[i][1], single[i][1]), (case, i)
            assert abs(s.vol @ z[i][1]) <= 1e-12 * np.abs(z[i][1]).max() * s.area
        assert inf["linear_iter"] == [t[2]["linear_iter"] for t in single]
        assert inf["residual_norm"] == [t[2]["residual_norm"] for t in single]
        assert inf["rhs_norm"] == [t[2]["rhs_norm"] for t in single]
        assert inf["converged"] == [True, True, True]
        for key in ("refresh_s", "transpose_s", "factor_s", "solve_s", "time"):
            assert isinstance(inf[key], float), key                       # one pass, reported once
        v = np.random.default_rng(6).standard_normal(s.n_u + s.n_p)
        assert gradient(s, v, index=1) == float(single[1][0] @ v[:s.n_u] + single[1][1] @ v[s.n_u:])
        with pytest.raises(ValueError):
            gradient(s, v)
        z1, _ = s.solve_adjoint(Js[0], rtol=1e-10, atol=0.0)             # a single functional again: a tuple again
        assert isinstance(z1, tuple) and np.array_equal(z1[0], single[0][0])
        assert gradient(s, v) == float(single[0][0] @ v[:s.n_u] + single[0][1] @ v[s.n_u:])
        with pytest.raises(ValueError):
            gradient(s, v, index=0)
    finally:
        s.close()


def test_adjoint_list_leaves_no_trace():
    """Continuation 10 -> 100 with a three-functional adjoint solve after every step: the same states, bit for bit, and the same
    Newton / Krylov counts as without (tests/test_gpu_adjoint.py: test_adjoint_leaves_no_trace for one functional)."""
    from alfi_amd.adjoint import LoadFunctional
    runs = []
    for with_adjoint in (False, True):
        s = _ns_solver("pkp0-2d")
        try:
            out = []
            for re in (10.0, 100.0):
                _, info = s.solve(re)
                out.append((s.u.copy(), s.p.copy(), info["linear_iter"], info["nonlinear_iter"]))
                if with_adjoint:
                    s.solve_adjoint([LoadFunctional(_weight), LoadFunctional(_force), LoadFunctional(_weight)])
            runs.append(out)
        finally:
            s.close()
    for a, b in zip(*runs):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2:] == b[2:]


def test_partitioned_saddle_and_hierarchy_refuse_block_calls():
    """A one-rank forced partition (DistMultigrid + DistSaddle, as tests/test_gpu_patch_storage.py sets one up): the saddle's
    and the hierarchy's block entry points return ALFI_E_ARG and write nothing."""
    from alfi_amd.dist import DistMultigrid, DistSaddle
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, build_hierarchy, build_pressure_coupling
    lv, tr = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 1, 2, Re=10.0)
    L = lv[-1]
    dmg = DistMultigrid(lv, tr, 2, solo=(0, 1), min_dofs=1, force_distributed=True)
    B, vol = build_pressure_coupling(L)
    sad = DistSaddle(dmg, B, vol, L.V.cell_nodes, L.nu, L.gamma, remove_constant_nullspace=True)
    try:
        ctx, n = sad.sad.ctx, sad.n
        dB, dX = ctx.mat(np.ones((n, 2))), ctx.mat(np.full((n, 2), SENTINEL))
        for fn in (lambda: sad.sad.solve_block(dB, dX), lambda: sad.sad.mult_block(dB, dX), lambda: sad.sad.precond_block(dB, dX)):
            _refused(fn)
        assert np.all(dX.get() == SENTINEL)
        nf = dmg.mg.levels[-1].n
        dB, dX = ctx.mat(np.ones((nf, 2))), ctx.mat(np.full((nf, 2), SENTINEL))
        for fn in (lambda: dmg.mg.vcycle_block(dB, dX), lambda: dmg.mg.fcycle_block(dB, dX)):
            _refused(fn)
        assert np.all(dX.get() == SENTINEL)
    finally:
        sad.close()
        dmg.close()
