"""Block right-hand sides on levels of dense MACRO-STAR inverses (patches above 160 dofs; kernels_block_big.hip).  -m gpu

The contract of tests/test_gpu_block_rhs.py, with no tolerance: column c of a block apply equals the single-vector apply on
column c BIT FOR BIT -- batched (one stream of the stored inverses for 2 .. 4 columns), in pieces narrower than a chunk
(Context.set_block_lds_bytes), looped (fewer than 8 patches), and with the batched kernels switched off.  Every case asserts the
``patch_apply_block_width()`` of the width rule (csrc/block_cols.h: the widest NV of 4, 3, 2 with NV x 8 x the largest patch
rounded up to even <= the budget), restated in tests/block_big_cases.py.

Levels (tests/block_big_cases.py: a dense 2736-dof operator of block size 3, sorted random dof subsets as patches, 8 .. 12
patches each), one per ``big_split`` (workgroups per patch of the single launcher) and per width class of the 64 KiB budget:

    level  sizes include                          big_split  width at 64 KiB  width 4 above 64 KiB
    D      161 162 163 191-193 255-257 512        1          4
    E      513 640 641                            2          4
    F      1153 1154 1155                         3          4
    A      2047 2048                              4          4
    B      2049                                   5          3                yes (the attribute path of the launcher)
    C      2731                                   6          2                yes

and the real thing: the 27 macro stars (150 .. 1599 dofs) of the 3-D [P3]^3 Scott-Vogelius level with dense inverses, for the
smoother in lockstep and two-level block cycles."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from tests import block_big_cases as bc
from tests.test_gpu_block_rhs import _check_block_apply
from tests.test_gpu_block_rhs_condensed import _same_bits


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_block_kernels(True)
    c.set_block_lds_bytes(bc.DEFAULT_LDS_BUDGET)
    c.close()


def _level(ctx, sizes, macro_dtype=None, pou=False):
    dl = hip.Level(ctx, bc.operator(), np.zeros(0, dtype=np.int32))
    dl.set_patches(*bc.patch_arrays(sizes))
    dl.set_patch_groups(None)
    if macro_dtype is not None:
        dl.set_macro_patch_storage(macro_dtype)
    if pou:
        dl.set_partition_of_unity(True)
    dl.factor()
    return dl


def test_the_levels_are_what_the_table_says():
    for name, sizes in bc.LEVELS.items():
        assert 8 <= len(sizes) <= 16 and max(sizes) > 160
        assert sum(8 * n * ((n + 1) & ~1) for n in sizes) < 0.1e9, name          # well under 0.3 GB of inverses
        assert (bc.big_split(len(sizes), max(sizes)), bc.block_big_width(max(sizes))) == bc.EXPECTED[name], name
    assert {n % 4 for n in bc.LEVELS["D"]} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", sorted(bc.LEVELS))
def test_block_apply_of_macro_stars_is_the_single_apply(ctx, name):
    sizes = bc.LEVELS[name]
    max_np, width = max(sizes), bc.EXPECTED[name][1]
    dl = _level(ctx, sizes)
    try:
        assert dl.patch_storage_dtype() == "f64" and dl.condensed() == 0
        assert dl.patch_apply_block_width() == width                   # on the parent: 0, dense macro stars loop
        X, ref = _check_block_apply(ctx, dl, np.random.default_rng(len(name) + max_np), True)
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
        if width < 4:                                                  # a budget that fits four columns: above 64 KiB
            need = bc.block_big_lds(max_np, 4)
            assert need > bc.DEFAULT_LDS_BUDGET
            ctx.set_block_lds_bytes(need)
            assert dl.patch_apply_block_width() == 4
            _same_bits(ctx, dl, X, ref)
            ctx.set_block_lds_bytes(need - 1)
            assert dl.patch_apply_block_width() == 3
            _same_bits(ctx, dl, X, ref)
            ctx.set_block_lds_bytes(bc.DEFAULT_LDS_BUDGET)
            assert dl.patch_apply_block_width() == width
        if name == "D":
            one = bc.block_big_lds(512, 1)
            for budget, w in ((3 * one, 3), (2 * one, 2), (2 * one - 1, 0), (0, 0)):
                ctx.set_block_lds_bytes(budget)
                assert dl.patch_apply_block_width() == w and dl.patch_apply_block_batched() == (w >= 2), budget
                _same_bits(ctx, dl, X, ref)
            ctx.set_block_lds_bytes(bc.DEFAULT_LDS_BUDGET)
            # against NumPy, at the tolerance tests/test_gpu_parity.py has for alfi_patch_apply (1e-7 of the max-norm)
            host = np.zeros_like(X)
            for p, m in enumerate(sizes):
                host[bc.dofs(m)] += dl.patch_inverse(p, m) @ X[bc.dofs(m)]
            assert np.abs(ref - host).max() < 1e-7 * np.abs(host).max()
        # the same bits with the batched kernels switched off
        ctx.set_block_kernels(False)
        assert dl.patch_apply_block_width() == 0 and not dl.patch_apply_block_batched()
        _same_bits(ctx, dl, X, ref)
        ctx.set_block_kernels(True)
        assert dl.patch_apply_block_width() == width
    finally:
        ctx.set_block_kernels(True)
        ctx.set_block_lds_bytes(bc.DEFAULT_LDS_BUDGET)
        dl.close()


@pytest.mark.parametrize("name", ["D", "F"])
def test_fp32_macro_storage(ctx, name):
    """the single-precision copy (guarded stores: a pad row's sum is never written): the width of FP64, the bits of the FP32
    single apply"""
    sizes = bc.LEVELS[name]
    dl = _level(ctx, sizes, macro_dtype="f32")
    try:
        assert dl.patch_storage_dtype() == "f32" and dl.condensed() == 0
        assert dl.patch_apply_block_width() == bc.EXPECTED[name][1]
        X, ref = _check_block_apply(ctx, dl, np.random.default_rng(61 + len(sizes)), True)
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
        ctx.set_block_kernels(False)
        assert dl.patch_apply_block_width() == 0
        _same_bits(ctx, dl, X, ref)
    finally:
        ctx.set_block_kernels(True)
        dl.close()


def test_partition_of_unity(ctx):
    dl, plain = _level(ctx, bc.LEVELS["E"], pou=True), _level(ctx, bc.LEVELS["E"])
    try:
        assert dl.patch_apply_block_width() == 4
        X, ref = _check_block_apply(ctx, dl, np.random.default_rng(62), True)
        dY = ctx.mat(dl.n, 5)
        plain.patch_apply_block(ctx.mat(X), dY)
        assert not np.array_equal(dY.get(), ref)                       # the flag did something
    finally:
        dl.close()
        plain.close()


def test_seven_patches_loop(ctx):
    """one patch below BIG_BLOCK_MIN_PATCHES: width 0, same bits"""
    sizes = bc.LEVELS["D"][:7]
    assert max(sizes) > 160
    dl = _level(ctx, sizes)
    try:
        assert dl.patch_apply_block_width() == 0
        _check_block_apply(ctx, dl, np.random.default_rng(63), False)
    finally:
        dl.close()
    dl = _level(ctx, bc.LEVELS["D"][:8])
    try:
        assert dl.patch_apply_block_width() == 4
        _check_block_apply(ctx, dl, np.random.default_rng(64), True)
    finally:
        dl.close()


def test_new_patch_set_and_refactorisation(ctx):
    """alfi_patches_set frees the staging slots of the block apply (sized by the old set), the next block apply grows them again;
    a refactorisation keeps them"""
    dl = _level(ctx, bc.LEVELS["E"])
    try:
        rng = np.random.default_rng(65)
        assert dl.patch_apply_block_width() == 4
        _check_block_apply(ctx, dl, rng, True)
        dl.set_patches(*bc.patch_arrays(bc.LEVELS["F"]))               # longer staging slots
        dl.set_patch_groups(None)
        dl.factor()
        assert dl.patch_apply_block_width() == 4
        X, ref = _check_block_apply(ctx, dl, rng, True)
        dl.factor()                                                    # a refactorisation of the same set
        assert dl.patch_apply_block_width() == 4
        _same_bits(ctx, dl, X, ref)
        dl.set_patches(*bc.patch_arrays(bc.SMALL_STARS))               # small stars on the same level: the dense batch
        dl.set_patch_groups(None)
        dl.factor()
        assert dl.patch_apply_block_width() == 4
        _check_block_apply(ctx, dl, rng, True)
    finally:
        dl.close()


def test_real_macro_stars_smoother_and_two_level_cycles(ctx):
    """The 27 macro stars (150 .. 1599 dofs, big_split 4) of the 3-D [P3]^3 Scott-Vogelius level with DENSE inverses: width 4; the
    block smoother in lockstep (k = 16: the single call leaves its four-launch iteration) and vcycle_block / fcycle_block of the
    two-level hierarchy equal the single calls per column, kernels on and off."""
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem
    from alfi_amd.sv import build_sv_hierarchy
    lv, tr = build_sv_hierarchy(ThreeDimLidDrivenCavityProblem(1), 1, 3, Re=100.0)
    fine = copy.copy(lv[1])
    fine.patch_groups = None                                           # dense inverses (27 stars: far below the level's own policy)
    sizes = np.diff(fine.patch_ptr)
    assert len(sizes) == 27 and sizes.min() == 150 and sizes.max() == 1599 and bc.big_split(27, 1599) == 4
    k = 16
    mg = hip.Multigrid(ctx, [lv[0], fine], tr, k)
    try:
        top = mg.levels[-1]
        n = top.n
        assert top.condensed() == 0 and top.patch_apply_block_width() == 4 and top.smooth_block_lockstep(k)
        rng = np.random.default_rng(66)
        _check_block_apply(ctx, top, rng, True)
        B, X0 = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
        B[fine.bc_dofs] = 0.0
        X0[fine.bc_dofs] = 0.0
        for guess in (True, False):
            ref = np.empty((n, 5))
            for c in range(5):
                db, dx = ctx.vec(B[:, c]), ctx.vec(X0[:, c])
                top.smooth(k, db, dx, nonzero_guess=guess)
                ref[:, c] = dx.get()
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
            for on in (True, False):
                ctx.set_block_kernels(on)
                dB, dX = ctx.mat(B), ctx.mat(X0)
                top.smooth_block(k, dB, dX, nonzero_guess=guess)
                assert np.array_equal(dX.get(), ref), (guess, on)
            ctx.set_block_kernels(True)
        refv, reff = np.empty_like(B), np.empty_like(B)
        for c in range(5):
            db, dx = ctx.vec(B[:, c]), ctx.vec(n)
            mg.vcycle(db, dx)
            refv[:, c] = dx.get()
            mg.fcycle(db, dx)
            reff[:, c] = dx.get()
        assert np.isfinite(refv).all() and np.isfinite(reff).all() and np.abs(reff).max() > 0.0
        for on in (True, False):
            ctx.set_block_kernels(on)
            dB, dX = ctx.mat(B), ctx.mat(n, 5)
            mg.vcycle_block(dB, dX)
            assert np.array_equal(dX.get(), refv), on
            mg.fcycle_block(dB, dX)
            assert np.array_equal(dX.get(), reff), on
    finally:
        ctx.set_block_kernels(True)
        mg.close()
