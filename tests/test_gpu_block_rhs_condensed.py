"""Block right-hand sides on CONDENSED patch levels (hip.Level.patch_apply_block and what is built on it).  -m gpu

The contract of tests/test_gpu_block_rhs.py, with no tolerance: column c of a block apply equals the single-vector apply on
column c BIT FOR BIT -- batched (kernels_block_cond.hip: one stream of X_g, B_g, W_g and inv(Sigma) for 2 .. 4 columns), in
pieces narrower than a chunk (Context.set_block_lds_bytes), looped (fewer than 1024 patches: the chunked form of the apply), and
with the batched kernels switched off.  Every case asserts ``condensed() != 0`` and the ``patch_apply_block_width()`` that the
width rule gives on the HOST plan of the same inputs (alfi_amd._hostlib.plan_condensed: the widest NV of 4, 3, 2 with
NV x max(lds_front, lds_back) <= budget; tests/block_cond_cases.py), and which waves-per-patch class (1 / 2 / 4 / 8 by the plan's
max_pairs) it exercises.

Levels, every one of at least 1024 patches unless it says otherwise (the patch list repeated: a repeated patch is a patch):
  * ldc3d [P2+FB]^3 N = 8 vertex stars listed twice (1458 patches, groups found by the library): 84 row pairs, 2 waves, width 4;
    with budgets of 3 x, 2 x, 1 x the level's LDS per column the widths 3, 2, 0;
  * its 57-dof boundary stars alone (16 row pairs): 1 wave;
  * Scott-Vogelius macro stars with the generator's groups: 2-D [P2]^2 (24 pairs: 1 wave), 3-D [P2]^3 (192 pairs: 4 waves) and,
    for 8 waves, 3-D [P3]^3 without its one interior star of 1599 dofs (336 pairs; 16 792 bytes of LDS per column: width 3 in
    64 KiB) -- with that star the level needs 32 968 bytes per column, two columns do not fit and it loops: asserted too;
  * the 1458 patches less one ... and 1023 of them: width 0."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import _hostlib, hip
from tests.block_cond_cases import DEFAULT_LDS_BUDGET, expected_width, lds_per_column, repeat_patches, waves_per_patch
from tests.test_gpu_block_rhs import SENTINEL, _check_block_apply, _single_columns, _wide


@pytest.fixture(scope="module")
def hier():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)


@pytest.fixture(scope="module")
def cctx():
    """every level condenses where it finds groups"""
    c = hip.Context(0)
    c.set_condense_min_bytes(0)
    yield c
    c.set_block_kernels(True)
    c.close()


@pytest.fixture(scope="module")
def stars(hier):
    """(host level N = 8, labels the host library finds, patch_ptr / patch_dofs / labels of the set listed twice, its host plan)"""
    L = hier[0][2]
    g = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)
    pp, pd, gg = repeat_patches(L.patch_ptr, L.patch_dofs, g, 2 * (len(L.patch_ptr) - 1))
    assert len(pp) - 1 == 1458
    return L, g, pp, pd, gg, _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, pp, pd, gg)


def _level(ctx, L, pp, pd, groups=None, pou=False):
    """groups None: the library finds them itself at factor time (cctx)"""
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(pp, pd)
    if groups is not None:
        dl.set_patch_groups(groups)
    if pou:
        dl.set_partition_of_unity(True)
    dl.factor()
    return dl


def _same_bits(ctx, dl, X, ref):
    """ncol 1 .. 5 and a gapped list, against the reference of the single apply"""
    n = dl.n
    for ncol in (1, 2, 3, 4, 5):
        dX, dY = ctx.mat(X[:, :ncol]), ctx.mat(n, ncol)
        dl.patch_apply_block(dX, dY)
        assert np.array_equal(dY.get(), ref[:, :ncol]), ncol
    ld = _wide(n, 6)
    dX, dY = ctx.mat(X[:, :4], ld=ld), ctx.mat(np.full((n, 4), SENTINEL), ld=ld)
    dl.patch_apply_block(dX, dY, cols=[3, 0, 2])
    Y = dY.get()
    assert np.array_equal(Y[:, [0, 2, 3]], ref[:, [0, 2, 3]]) and np.all(Y[:, 1] == SENTINEL)
    assert np.all(dY._buf.get().reshape(4, ld)[:, n:] == 0.0)


def test_vertex_stars_with_library_found_groups(cctx, stars):
    L, g, pp, pd, gg, plan = stars
    assert waves_per_patch(plan) == 2 and expected_width(plan, npatch=1458) == 4
    per = lds_per_column(plan)
    dl = _level(cctx, L, pp, pd)
    try:
        assert dl.condensed() == 2
        assert dl.patch_apply_block_batched()                          # on the parent a condensed level loops
        assert dl.patch_apply_block_width() == 4
        X, ref = _check_block_apply(cctx, dl, np.random.default_rng(41), True)
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
        for k, width in ((3, 3), (2, 2), (1, 0)):
            cctx.set_block_lds_bytes(k * per)
            assert dl.patch_apply_block_width() == width == expected_width(plan, k * per)
            assert dl.patch_apply_block_batched() == (width >= 2)
            _same_bits(cctx, dl, X, ref)
        cctx.set_block_lds_bytes(3 * per - 1)                          # one byte less than three columns need
        assert dl.patch_apply_block_width() == 2
        cctx.set_block_lds_bytes(0)
        assert dl.patch_apply_block_width() == 0
        cctx.set_block_lds_bytes(DEFAULT_LDS_BUDGET)
        assert dl.patch_apply_block_width() == 4
        cctx.set_block_kernels(False)
        assert dl.patch_apply_block_width() == 0 and not dl.patch_apply_block_batched()
        _same_bits(cctx, dl, X, ref)
        cctx.set_block_kernels(True)
        assert dl.patch_apply_block_width() == 4
        # a budget above the device's limit is clamped, never an error; the width stays 4
        cctx.set_block_lds_bytes(1 << 40)
        assert dl.patch_apply_block_width() == 4
    finally:
        cctx.set_block_lds_bytes(DEFAULT_LDS_BUDGET)
        cctx.set_block_kernels(True)
        dl.close()


def test_dense_levels_report_width_four(cctx):
    from tests.test_gpu_block_rhs import _class_sizes, _synthetic
    dl = _synthetic(cctx, 3, _class_sizes(4))
    looped = _synthetic(cctx, 3, _class_sizes(8)[:200])
    try:
        assert dl.condensed() == 0 and dl.patch_apply_block_batched() and dl.patch_apply_block_width() == 4
        assert not looped.patch_apply_block_batched() and looped.patch_apply_block_width() == 0
        cctx.set_block_lds_bytes(0)                                    # the budget is the condensed levels' alone
        assert dl.patch_apply_block_width() == 4
    finally:
        cctx.set_block_lds_bytes(DEFAULT_LDS_BUDGET)
        dl.close()
        looped.close()


def test_one_wave_per_patch(cctx, stars):
    """the 57-dof boundary stars alone (two groups of 15, a skeleton of 27), repeated to 1030 patches"""
    L, g = stars[0], stars[1]
    sizes = np.diff(L.patch_ptr)
    sel = np.flatnonzero(sizes == 57)
    spp = np.concatenate([[0], np.cumsum(sizes[sel])]).astype(np.int64)
    take = lambda a: np.concatenate([a[L.patch_ptr[p]:L.patch_ptr[p + 1]] for p in sel]).astype(np.int32)
    pp, pd, gg = repeat_patches(spp, take(L.patch_dofs), take(g), 1030)
    plan = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, pp, pd, gg)
    assert plan["max_pairs"] <= 64 and waves_per_patch(plan) == 1 and expected_width(plan, npatch=1030) == 4
    dl = _level(cctx, L, pp, pd)
    try:
        assert dl.condensed() == 2 and dl.patch_apply_block_width() == 4
        _check_block_apply(cctx, dl, np.random.default_rng(42), True)
    finally:
        dl.close()


SV_CASES = {"2d-P2": (1, 4), "3d-P2": (4, 4), "3d-P3-faces": (8, 3), "3d-P3": (8, 0)}      # waves per patch, width


@pytest.mark.parametrize("case", sorted(SV_CASES))
def test_macro_stars_with_caller_supplied_groups(case):
    """the Scott-Vogelius levels of tests/test_gpu_condensed.py, their patch lists (and groups) repeated to 1024 patches"""
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    from alfi_amd.sv import build_sv_hierarchy
    prob, nref, k = {"2d-P2": (TwoDimLidDrivenCavityProblem(2), 2, 2), "3d-P2": (ThreeDimLidDrivenCavityProblem(1), 1, 2),
                     "3d-P3": (ThreeDimLidDrivenCavityProblem(1), 1, 3), "3d-P3-faces": (ThreeDimLidDrivenCavityProblem(1), 1, 3)}[case]
    lv, _ = build_sv_hierarchy(prob, nref, k, Re=100.0)
    L = lv[-1]
    pp, pd, g = np.asarray(L.patch_ptr, dtype=np.int64), np.asarray(L.patch_dofs), np.asarray(L.patch_groups, dtype=np.int32)
    if case.startswith("3d-P3"):
        # "faces": without the interior star of 1599 dofs the largest patch has 837 (the 150-dof corner stars seven times each:
        # the case factors in seconds); "3d-P3": that star and 127 copies of a corner star, so that the level that does not fit
        # two columns factors in seconds as well (8 stars of 1599 dofs among 1024 patches)
        sizes = np.diff(pp)
        if case == "3d-P3-faces":
            sel = np.concatenate([np.flatnonzero(sizes <= 837), np.repeat(np.flatnonzero(sizes == 150), 6)])
        else:
            sel = np.concatenate([np.flatnonzero(sizes == 1599)[:1], np.repeat(np.flatnonzero(sizes == 150)[:1], 127)])
        take = lambda a: np.concatenate([a[pp[p]:pp[p + 1]] for p in sel])
        pp, pd, g = np.concatenate([[0], np.cumsum(sizes[sel])]).astype(np.int64), take(pd), take(g)
    pp, pd, g = repeat_patches(pp, pd, g, 1024)
    plan = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, pp, pd, g)
    waves, width = SV_CASES[case]
    assert waves_per_patch(plan) == waves and expected_width(plan, npatch=1024) == width, (plan["max_pairs"], lds_per_column(plan))
    ctx = hip.Context(0)
    dl = _level(ctx, L, pp, pd, g)
    try:
        assert dl.condensed() == 1 and dl.patch_apply_block_width() == width
        X, ref = _check_block_apply(ctx, dl, np.random.default_rng(43), width >= 2)
        if width == 0:         # ... and with room for two columns (the device gives a workgroup more than 64 KiB) it batches
            ctx.set_block_lds_bytes(2 * lds_per_column(plan))
            if dl.patch_apply_block_width() == 2:
                _same_bits(ctx, dl, X, ref)
    finally:
        dl.close()
        ctx.close()


@pytest.mark.parametrize("npatch", [1457, 1023])
def test_levels_below_the_per_patch_threshold_loop(cctx, stars, npatch):
    """one patch dropped: 1457 still batches; 1023 patches take the chunked form of the single apply, and the block call loops"""
    L, g, pp, pd, gg, plan = stars
    pp, pd = pp[:npatch + 1], pd[:pp[npatch]]
    want = 4 if npatch >= 1024 else 0
    assert expected_width(plan, npatch=npatch) == want
    dl = _level(cctx, L, pp, pd)
    try:
        assert dl.condensed() == 2 and dl.patch_apply_block_width() == want
        _check_block_apply(cctx, dl, np.random.default_rng(44), want >= 2)
    finally:
        dl.close()


def test_partition_of_unity(cctx, stars):
    L, g, pp, pd, gg, plan = stars
    dl, plain = _level(cctx, L, pp, pd, pou=True), _level(cctx, L, pp, pd)
    try:
        assert dl.condensed() == 2 and dl.patch_apply_block_width() == 4
        X, ref = _check_block_apply(cctx, dl, np.random.default_rng(45), True)
        dY = cctx.mat(dl.n, 5)
        plain.patch_apply_block(cctx.mat(X), dY)
        assert not np.array_equal(dY.get(), ref)                       # the flag did something
    finally:
        dl.close()
        plain.close()


def test_new_patch_set_and_refactorisation(cctx, stars):
    """alfi_patches_set frees the per-column scratch of the block apply (its slots are sized by the old set), the next block
    apply grows it again; a refactorisation keeps it"""
    L, g, pp, pd, gg, plan = stars
    dl = _level(cctx, L, pp[:1101], pd[:pp[1100]])                     # 1100 patches first
    try:
        assert dl.condensed() == 2 and dl.patch_apply_block_width() == 4
        rng = np.random.default_rng(46)
        _check_block_apply(cctx, dl, rng, True)
        dl.set_patches(pp, pd)                                         # a larger set: longer slots
        dl.factor()
        assert dl.condensed() == 2 and dl.patch_apply_block_width() == 4
        X, ref = _check_block_apply(cctx, dl, rng, True)
        dl.factor()                                                    # a refactorisation of the same set
        assert dl.patch_apply_block_width() == 4
        _same_bits(cctx, dl, X, ref)
        dl.set_patches(pp[:1025], pd[:pp[1024]])                       # a smaller set again
        dl.factor()
        _check_block_apply(cctx, dl, rng, True)
        dl.set_patch_groups(None)                                      # and dense inverses on the same level: the dense batch
        dl.factor()
        assert dl.condensed() == 0 and dl.patch_apply_block_width() == 4
        _check_block_apply(cctx, dl, rng, True)
    finally:
        dl.close()


def test_smoother_in_lockstep_and_two_level_cycles(cctx, hier, stars):
    """On the 1458-patch level the block smoother runs in lockstep from k = 16 on (below, this level of 34 323 dofs takes the
    four-launch iteration and whole smoother calls loop) and equals the single smoother per column; a two-level hierarchy N = 4
    / N = 8 with 16 smoothing steps: vcycle_block / fcycle_block equal the single cycles per column."""
    L, g, pp, pd, gg, plan = stars
    dl = _level(cctx, L, pp, pd)
    try:
        n = dl.n
        assert dl.patch_apply_block_width() == 4 and dl.smooth_block_lockstep(16) and not dl.smooth_block_lockstep(2)
        rng = np.random.default_rng(47)
        B, X0 = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
        for k, guess in ((16, True), (16, False), (2, True)):
            ref = np.empty((n, 5))
            for c in range(5):
                db, dx = cctx.vec(B[:, c]), cctx.vec(X0[:, c])
                dl.smooth(k, db, dx, nonzero_guess=guess)
                ref[:, c] = dx.get()
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
            for on in (True, False):
                cctx.set_block_kernels(on)
                dB, dX = cctx.mat(B), cctx.mat(X0)
                dl.smooth_block(k, dB, dX, nonzero_guess=guess)
                assert np.array_equal(dX.get(), ref), (k, guess, on)
            cctx.set_block_kernels(True)
            dX = cctx.mat(X0[:, :4], ld=_wide(n, 2))
            dl.smooth_block(k, cctx.mat(B[:, :4]), dX, nonzero_guess=guess, cols=[0, 2, 3])
            got = dX.get()
            assert np.array_equal(got[:, [0, 2, 3]], ref[:, [0, 2, 3]]) and np.array_equal(got[:, 1], X0[:, 1]), (k, guess)
    finally:
        cctx.set_block_kernels(True)
        dl.close()
    lv, tr = hier
    coarse, fine = copy.copy(lv[1]), copy.copy(lv[2])
    coarse.level, fine.level = 0, 1
    fine.patch_ptr, fine.patch_dofs = pp, pd
    mg = hip.Multigrid(cctx, [coarse, fine], [tr[1]], 16)
    try:
        top = mg.levels[-1]
        assert top.condensed() == 2 and top.patch_apply_block_width() == 4 and top.smooth_block_lockstep(16)
        n = top.n
        B = np.random.default_rng(48).standard_normal((n, 5))
        B[L.bc_dofs] = 0.0
        refv, reff = np.empty_like(B), np.empty_like(B)
        for c in range(5):
            db, dx = cctx.vec(B[:, c]), cctx.vec(n)
            mg.vcycle(db, dx)
            refv[:, c] = dx.get()
            mg.fcycle(db, dx)
            reff[:, c] = dx.get()
        assert np.isfinite(refv).all() and np.isfinite(reff).all() and np.abs(reff).max() > 0.0
        for on in (True, False):
            cctx.set_block_kernels(on)
            dB, dX = cctx.mat(B), cctx.mat(n, 5)
            mg.vcycle_block(dB, dX)
            assert np.array_equal(dX.get(), refv), on
            mg.fcycle_block(dB, dX)
            assert np.array_equal(dX.get(), reff), on
        cctx.set_block_kernels(True)
        dX = cctx.mat(np.full((n, 5), SENTINEL), ld=_wide(n, 4))
        mg.fcycle_block(cctx.mat(B), dX, cols=[4, 0, 2])
        got = dX.get()
        assert np.array_equal(got[:, [0, 2, 4]], reff[:, [0, 2, 4]]) and np.all(got[:, [1, 3]] == SENTINEL)
    finally:
        cctx.set_block_kernels(True)
        mg.close()
