"""The tail launch of the condensed apply (csrc/cond_layout.h: cond_tail; cond_tail_kernel): the Schur solve and the back
substitution of a patch in one workgroup of 256 threads -- a wave's rows of inv(Sigma) and a quarter of a row pair of W per lane
requested at kernel entry, y_S through LDS, a row pair's W sum one chain through four lanes.  The sums must stay those of
cond_sigma_kernel + cond_back_kernel to the bit.  -m gpu.

The reference for bits is the chunked form of the condensed apply (cond_gfront / cond_gsigma / cond_gback, untouched), which
launches of fewer than 1024 patches take: patch_apply_split cuts a level of >= 1024 patches into two such launches, the full range
is ONE launch of the workgroup-per-patch kernels (tests/test_gpu_sigma_ahead.py has the argument).  Which tail a level takes is
the rule of cond_layout.h, restated here on the host plan; the rule itself is checked by tests/test_cond_tail_rule.py.

Shapes: the N = 8 level of ldc3d [P2+FB]^3 (729 patches: 3 / 9 / 21 / 33 dofs without a group, 57-dof stars with two groups of
15 and a skeleton of 27 = a block of 16 rows | pieces of 8 + 4, 153-dof stars with six groups and a skeleton of 63 = four blocks of
16) listed twice and four times; synthetic levels of 1025 disjoint "arrowhead" patches with caller-supplied groups at the rule's
bounds: 8 / 16 / 32 and 9 / 27 coupled skeleton entries (one, two, four quarters full; a part-filled second and fourth), 34 and 33
(not taken), 64 and 65 row pairs of X / W, skeletons of 62 / 64 (taken: every piece of 8, 4, 2 rows behind whole 16s, the pieces
of 64, 32 and 16 rows) and 66 entries (not taken), a group of one node and a patch without a group beside full patches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_cond_ahead import _shape, arrowhead_level
from tests.test_gpu_sigma_ahead import applies, repeated


def maxima(plan):
    """(max_xpairs, max_sc, max_s) of CondPlan (csrc/patch_plan.h) from the tables of a host plan: most row pairs of X / W in a
    patch, most coupled skeleton entries of a group, the largest skeleton"""
    return int(np.diff(plan["xp_ptr"]).max()), int(np.asarray(plan["g_sc"]).max()), int(plan["max_s"])


def takes_tail(plan):
    """cond_tail (csrc/cond_layout.h) on a host plan"""
    max_xpairs, max_sc, max_s = maxima(plan)
    return max_xpairs <= 64 and max_sc <= 32 and max_s <= 64


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


def test_vertex_stars_take_the_tail_launch_and_keep_the_bits(cctx, star_level):
    from alfi_amd import _hostlib
    L = star_level
    sizes = set(np.diff(L.patch_ptr).tolist())
    assert len(L.patch_ptr) - 1 == 729 and {3, 9, 21, 33, 57, 153} <= sizes
    g = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)
    pp, pd, gg = repeated(L, 2, g)                                              # 1458 patches
    plan = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, pp, pd, gg)
    print("vertex stars: max_xpairs %d, max_sc %d, max_s %d" % maxima(plan))
    assert maxima(plan) == (48, 27, 63) and takes_tail(plan)
    full, (halves, uneven) = applies(cctx, L, pp, pd, None, (729, 500), 0)      # (applies: twice the same bits, condensed() == 2)
    assert np.array_equal(halves, full)                                         # 729 | 729: both in the chunked form
    assert np.array_equal(uneven, full)                                         # 500 | 958
    pp, pd, _ = repeated(L, 4)
    full, (split,) = applies(cctx, L, pp, pd, None, (1459,), 1)                 # two per-patch launches, the second at p0 > 0
    assert np.array_equal(split, full)


# ---- synthetic levels: disjoint patches, caller-supplied groups (tests/test_gpu_cond_ahead.py: arrowhead_level) ----------------
_SMALL = [_shape([8, 7], [8, 9], 9), _shape([], [], 4), _shape([1], [1], 1)]     # full patch, no group, a group of one node
# name -> (bs, shapes, tail launch expected, (max_xpairs, max_sc, max_s) with None = not asserted)
LEVELS = {
    # W of 8 / 16 / 32 / 2 columns: one, two, four quarters exactly full; beside them a patch without a group and a one-node group
    "bs2-sc8-16-32": (2, [_shape([4, 8, 7, 1], [4, 8, 16, 1], 16)] + _SMALL, True, (None, 32, 32)),
    # 9 / 27 / 3 columns: a part-filled second and fourth quarter, odd groups (15: the pad row)
    "bs3-sc9-27": (3, [_shape([5, 5, 1], [3, 9, 1], 9), _shape([], [], 2), _shape([1], [1], 2)], True, (None, 27, 27)),
    # a column more than the four quarters hold: the three launches
    "bs2-sc34": (2, [_shape([8, 7], [17, 4], 17)] + _SMALL, False, (None, 34, 34)),
    "bs3-sc33": (3, [_shape([5, 4], [11, 3], 11), _shape([], [], 2)], False, (None, 33, 33)),
    # a group of 18 entries: the front kernel in its loop form (tests/test_gpu_cond_ahead.py), the tail launch behind it
    "bs2-m18": (2, [_shape([9, 8], [8, 9], 9)] + _SMALL, True, (None, 18, 18)),
    # 8 groups of 16 entries = 64 row pairs of X / W: a quartet for every pair of the 256 lanes ...
    "pairs-64": (2, [_shape([8] * 8, [2] * 8, 6)] + _SMALL * 8, True, (64, None, None)),
    # ... and one pair more
    "pairs-65": (2, [_shape([8] * 8 + [1], [2] * 8 + [1], 6)] + _SMALL * 8, False, (65, None, None)),
    # skeletons of 62 (32 + 16 | 8 + 4 + 2 in the last wave), 48 (32 + 16) and 10 (8 + 2) rows
    "s-62": (2, [_shape([7, 8], [9, 16], 31), _shape([8], [12], 24), _shape([3], [5], 5)] + _SMALL, True, (None, 32, 62)),
    # 64 (one piece of 64 rows), 44 (32 + 8 + 4) and 14 (8 + 4 + 2)
    "s-64": (2, [_shape([7, 8], [16, 9], 32), _shape([8], [11], 22), _shape([3], [7], 7)] + _SMALL, True, (None, 32, 64)),
    # 66: two chunks of the sigma launch
    "s-66": (2, [_shape([7, 8], [9, 16], 33)] + _SMALL, False, (None, 32, 66)),
    # odd skeletons: 63 (the pad row in the fourth block of 16), 45 (32 + 8 + 4 + 2, the pad row in the piece of 2), 3
    "bs3-s63": (3, [_shape([5, 5], [9, 4], 21), _shape([4], [5], 15), _shape([1], [1], 1), _shape([], [], 2)], True,
                (None, 27, 63)),
}


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_caller_supplied_groups_at_the_dispatch_bounds(cctx, name):
    from alfi_amd import _hostlib, hip
    bs, shapes, tail, (max_xpairs, max_sc, max_s) = LEVELS[name]
    npatch = 1025
    A, pp, pd, groups = arrowhead_level(bs, shapes, npatch, sorted(LEVELS).index(name))
    plan = _hostlib.plan_condensed(bs, A.rowptr, A.colidx, pp, pd, groups)
    print("%s: %d dofs, max_xpairs %d, max_sc %d, max_s %d" % ((name, A.nbrows * bs) + maxima(plan)))
    assert takes_tail(plan) == tail
    for got, want in zip(maxima(plan), (max_xpairs, max_sc, max_s)):
        assert want is None or got == want, (maxima(plan), (max_xpairs, max_sc, max_s))
    n = A.nbrows * bs
    dl = hip.Level(cctx, A, np.zeros(0, dtype=np.int32))
    dl.set_patches(pp, pd)
    dl.set_patch_groups(groups)
    dl.factor()
    assert dl.condensed() == 1
    x = np.random.default_rng(100).standard_normal(n)
    dx, dy = cctx.vec(x), cctx.vec(n)
    dl.patch_apply(dx, dy)
    full = dy.get()
    dl.patch_apply(dx, dy)
    assert np.array_equal(dy.get(), full)              # the same input, the same bits
    for cut in (npatch // 2, 3):                       # both ranges chunked: 512 | 513 and 3 | 1022
        dl.patch_apply_split(cut, dx, dy)
        assert np.array_equal(dy.get(), full), cut
    dl.close()
    # the patches are disjoint: the apply is a solve per patch
    S = A.to_scipy().tocsr()
    ref = np.zeros(n)
    for p in range(npatch):
        dofs = pd[pp[p]:pp[p + 1]]
        ref[dofs] = np.linalg.solve(S[dofs][:, dofs].toarray(), x[dofs])
    err = np.abs(full - ref).max() / np.abs(ref).max()
    print("%s: against numpy.linalg.solve per patch %.2e" % (name, err))
    assert err < 1e-9                                  # (tests/test_gpu_cond_ahead.py, tests/test_gpu_condensed.py)
