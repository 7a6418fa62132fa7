"""cond_sigma_kernel requests the first block of a wave's rows of inv(Sigma) before the Schur right-hand side is in LDS
(big_block_prefetch / big_block_finish) where the skeleton is small enough for the block to fit in one batch of loads.  The sums
must stay those of big_rows to the bit.  -m gpu.

The reference is the chunked form of the condensed apply (cond_gsigma_kernel: big_rows after the barrier, untouched), which
launches of fewer than 1024 patches take: patch_apply_split cuts a level of >= 1024 patches into two such launches, the full
range is ONE launch of the workgroup-per-patch kernels, and the dof-wise sum behind both is the same kernel over the same staging
slots -- equal staged values give equal bits.

Shapes: tests/test_gpu_star_condense.py's N = 8 level of ldc3d [P2+FB]^3 (729 patches: 3 / 9 / 21 / 33 dofs without a group,
57-dof stars with a skeleton of 27 = blocks of 16 | 8 + 4 rows, 153-dof stars with a skeleton of 63 = four blocks of 16 rows, the
pad row in the last) listed twice and four times; 2-D Scott-Vogelius macro stars with the generator's groups, [P2]^2 (skeletons
of <= 14: blocks of 8, 4, 2 rows) and [P3]^2, 25 patches listed 41 times."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def repeated(L, times, groups=None):
    """the level's patch set (and its group labels) listed ``times`` times"""
    pp, pd = np.asarray(L.patch_ptr, dtype=np.int64), np.asarray(L.patch_dofs, dtype=np.int32)
    ptr = np.concatenate([[0]] + [pp[1:] + i * pp[-1] for i in range(times)])
    return ptr, np.tile(pd, times), None if groups is None else np.tile(np.asarray(groups, dtype=np.int32), times)


@pytest.fixture(scope="module")
def cctx():
    """every level condenses where it finds groups"""
    from alfi_amd import hip
    c = hip.Context(0)
    c.set_condense_min_bytes(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def star_level():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)[0][2]


def applies(ctx, L, pp, pd, groups, splits, seed):
    """the full-range apply (twice: reproducible) and the apply split at each of ``splits``"""
    from alfi_amd import hip
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(pp, pd)
    if groups is not None:
        dl.set_patch_groups(groups)
    dl.factor()
    assert dl.condensed() == (2 if groups is None else 1)
    x = np.random.default_rng(seed).standard_normal(L.n)
    dx, dy = ctx.vec(x), ctx.vec(L.n)
    dl.patch_apply(dx, dy)
    full = dy.get()
    dl.patch_apply(dx, dy)
    assert np.array_equal(dy.get(), full)
    out = []
    for sp in splits:
        dl.patch_apply_split(sp, dx, dy)
        out.append(dy.get())
    dl.close()
    assert np.isfinite(full).all() and np.abs(full).max() > 0.0
    return full, out


def test_vertex_stars_one_large_launch_equals_two_chunked_launches(cctx, star_level):
    pp, pd, _ = repeated(star_level, 2)                                        # 1458 patches
    full, (halves, uneven) = applies(cctx, star_level, pp, pd, None, (729, 500), 0)
    assert np.array_equal(halves, full)                                         # 729 | 729: both in the chunked form
    assert np.array_equal(uneven, full)                                         # 500 | 958


def test_vertex_stars_two_large_range_launches_equal_the_ordered_full_range(cctx, star_level):
    """2916 patches split at 1459: both ranges take the workgroup-per-patch kernels in the natural order, the full range walks
    the patches largest first"""
    pp, pd, _ = repeated(star_level, 4)
    full, (split,) = applies(cctx, star_level, pp, pd, None, (1459,), 1)
    assert np.array_equal(split, full)


@pytest.mark.parametrize("k", [2, 3])
def test_small_macro_stars_of_the_caller(cctx, k):
    from alfi_amd import _hostlib
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem
    from alfi_amd.sv import build_sv_hierarchy
    lv, _ = build_sv_hierarchy(TwoDimLidDrivenCavityProblem(2), 1, k, Re=10.0)
    L = lv[-1]
    pl = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs, np.asarray(L.patch_groups, dtype=np.int32))
    print("[P%d]^2 macro stars: %d patches of up to %d dofs, max_s %d, max_pairs %d"
          % (k, len(L.patch_ptr) - 1, int(np.diff(L.patch_ptr).max()), pl["max_s"], pl["max_pairs"]))
    times = -(-1025 // (len(L.patch_ptr) - 1))
    pp, pd, groups = repeated(L, times, L.patch_groups)
    npatch = len(pp) - 1
    assert npatch >= 1024
    full, (split,) = applies(cctx, L, pp, pd, groups, (npatch // 2,), 2)
    assert np.array_equal(split, full)
