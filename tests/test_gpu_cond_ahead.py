"""The early-load form of cond_front_kernel (csrc/cond_layout.h: cond_ahead): a lane requests its tables and its whole row pair of
X or B at kernel entry, the X and the B pairs of a patch in different waves.  The sums must stay those of the loop form to the
bit.  -m gpu.

The reference for bits is the chunked form of the condensed apply (cond_gfront / cond_gsigma / cond_gback, untouched), which
launches of fewer than 1024 patches take: patch_apply_split cuts a level of >= 1024 patches into two such launches, the full range
is ONE launch of the workgroup-per-patch kernels (tests/test_gpu_sigma_ahead.py has the argument).  Which of the two
workgroup-per-patch forms a level takes is the rule of cond_layout.h, restated here on the host plan; the rule itself is
checked by tests/test_cond_ahead_rule.py.

Shapes: the N = 8 level of ldc3d [P2+FB]^3 (729 patches: 3 / 9 / 21 / 33 dofs without a group, 57-dof stars with two groups of
15, 153-dof stars with six) listed twice and four times; synthetic levels of >= 1025 disjoint "arrowhead" patches with
caller-supplied groups (group sizes 14 / 16 / 18 with blocks of 2, 15 / 18 with blocks of 3, a group of one node, a patch without
a group, 14 / 16 / 18 and 15 / 18 / 27 coupled skeleton entries -- row pairs of B that fill one wave, two, or part of one --,
a patch of exactly 512 row pairs and one of 513); 2-D Scott-Vogelius macro stars with the generator's groups."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_sigma_ahead import applies, repeated

AHEAD_M = 16          # csrc/cond_layout.h: COND_AHEAD_M, the columns of a row pair a lane requests at once


def takes_ahead(plan):
    """cond_ahead (csrc/cond_layout.h) on a host plan"""
    mp = int(plan["max_pairs"])
    waves = 1 if mp <= 64 else 2 if mp <= 128 else 4 if mp <= 256 else 8
    return int(plan["max_m"]) <= AHEAD_M and mp <= 64 * waves


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


def test_vertex_stars_take_the_early_load_form_and_keep_the_bits(cctx, star_level):
    from alfi_amd import _hostlib
    L = star_level
    sizes = set(np.diff(L.patch_ptr).tolist())
    assert len(L.patch_ptr) - 1 == 729 and {3, 9, 21, 33, 57, 153} <= sizes
    g = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)
    pp, pd, gg = repeated(L, 2, g)                                              # 1458 patches
    plan = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, pp, pd, gg)
    print("vertex stars: max_m %d, max_pairs %d" % (plan["max_m"], plan["max_pairs"]))
    assert plan["max_m"] == 15 and plan["max_pairs"] == 84 and takes_ahead(plan)
    full, (halves, uneven) = applies(cctx, L, pp, pd, None, (729, 500), 0)      # (applies asserts condensed() == 2)
    assert np.array_equal(halves, full)                                         # 729 | 729: both in the chunked form
    assert np.array_equal(uneven, full)                                         # 500 | 958
    pp, pd, _ = repeated(L, 4)
    full, (split,) = applies(cctx, L, pp, pd, None, (1459,), 1)                 # two per-patch launches in natural order
    assert np.array_equal(split, full)


# ---- synthetic levels: disjoint patches, caller-supplied groups ----------------------------------------------------------------
# a patch shape: (nodes per group, skeleton nodes each group couples to, skeleton nodes); the skeleton is dense
def _shape(groups, coupled, ns):
    assert len(groups) == len(coupled) and all(c <= ns for c in coupled)
    return tuple(groups), tuple(coupled), ns


def arrowhead_level(bs, shapes, npatch, seed):
    """(BSR, patch_ptr, patch_dofs, groups): patch p has the shape shapes[p % len(shapes)] on nodes of its own; group g couples
    to itself and to ``coupled[g]`` skeleton nodes (a window that moves with g), symmetric sparsity, diagonally dominant"""
    from alfi_amd.problem import BSR
    rng = np.random.default_rng(seed)
    rowptr, colidx, pdofs, glab, pp = [0], [], [], [], [0]
    node0 = 0
    for p in range(npatch):
        groups, coupled, ns = shapes[p % len(shapes)]
        nI = sum(groups)
        nn = nI + ns
        mask = np.zeros((nn, nn), dtype=bool)
        lab = np.full(nn, -1, dtype=np.int32)
        a = 0
        for gi, (k, c) in enumerate(zip(groups, coupled)):
            mask[a:a + k, a:a + k] = True
            cols = nI + (np.arange(c) + 3 * gi) % ns
            mask[np.ix_(np.arange(a, a + k), cols)] = True
            mask[np.ix_(cols, np.arange(a, a + k))] = True
            lab[a:a + k] = 7 + 2 * gi                  # (any distinct non-negative labels)
            a += k
        mask[nI:, nI:] = True
        perm = rng.permutation(nn)                     # groups and skeleton interleaved in the patch's (ascending) node list
        local = np.zeros_like(mask)
        local[np.ix_(perm, perm)] = mask
        for i in range(nn):
            cols = np.flatnonzero(local[i])
            colidx.append(node0 + cols)
            rowptr.append(rowptr[-1] + len(cols))
        llab = np.empty_like(lab)
        llab[perm] = lab
        nodes = node0 + np.arange(nn)
        pdofs.append((nodes[:, None] * bs + np.arange(bs)[None, :]).ravel())
        glab.append(np.repeat(llab, bs))
        pp.append(pp[-1] + nn * bs)
        node0 += nn
    colidx = np.concatenate(colidx).astype(np.int32)
    rowptr = np.asarray(rowptr, dtype=np.int32)
    vals = 0.3 * rng.standard_normal((len(colidx), bs, bs))
    rows = np.repeat(np.arange(node0), np.diff(rowptr))
    width = np.diff(rowptr)[rows[rows == colidx]]      # entries of the block row
    vals[rows == colidx] += (2.0 + 0.5 * width * bs)[:, None, None] * np.eye(bs)[None]
    A = BSR(node0, node0, bs, rowptr, colidx, vals)
    return A, np.asarray(pp, dtype=np.int64), np.concatenate(pdofs).astype(np.int32), np.concatenate(glab).astype(np.int32)


# name -> (bs, shapes, early-load form expected, max_m, max_pairs or None)
LEVELS = {
    # groups of 14 and 16 entries and of one node (2), coupled to 14 / 16 / 18 / 2 skeleton entries; a patch without a group
    "bs2-m14-16": (2, [_shape([7, 8, 1], [7, 8, 9], 9), _shape([], [], 4), _shape([8, 8, 7, 1], [9, 1, 8, 7], 10),
                       _shape([1], [1], 1)], True, 16, None),
    # one group of 18 entries in the level: the loop form
    "bs2-m18": (2, [_shape([7, 8, 1], [7, 8, 9], 9), _shape([9, 8], [8, 9], 9), _shape([], [], 3)], False, 18, None),
    # odd groups (15, 3: the pad row), coupled to 15 / 18 / 27 / 3 skeleton entries
    "bs3-m15": (3, [_shape([5, 5, 1], [5, 6, 9], 9), _shape([], [], 2), _shape([5, 1, 5, 5], [9, 1, 6, 5], 9)], True, 15, None),
    "bs3-m18": (3, [_shape([5, 6], [5, 6], 7), _shape([5, 1], [9, 1], 9), _shape([], [], 1)], False, 18, None),
    # 64 groups of 16 entries = 512 row pairs of X: exactly 64 x 8 waves (the front workgroup: 8 waves of X pairs, 2 of B pairs)
    "pairs-512": (2, [_shape([8] * 64, [2] * 64, 6)] + [_shape([8, 7], [8, 9], 9)] * 40, True, 16, 512),
    # ... and one pair more: two passes, the loop form
    "pairs-513": (2, [_shape([8] * 64 + [1], [2] * 64 + [1], 6)] + [_shape([8, 7], [8, 9], 9)] * 40, False, 16, 513),
}


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_caller_supplied_groups_at_the_dispatch_bounds(cctx, name):
    from alfi_amd import _hostlib, hip
    bs, shapes, ahead, max_m, max_pairs = LEVELS[name]
    npatch = 1025
    A, pp, pd, groups = arrowhead_level(bs, shapes, npatch, sorted(LEVELS).index(name))
    plan = _hostlib.plan_condensed(bs, A.rowptr, A.colidx, pp, pd, groups)
    print("%s: %d dofs, max_m %d, max_pairs %d, max_s %d" % (name, A.nbrows * bs, plan["max_m"], plan["max_pairs"], plan["max_s"]))
    assert plan["max_m"] == max_m and takes_ahead(plan) == ahead
    if max_pairs is not None:
        assert plan["max_pairs"] == max_pairs
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
    assert err < 1e-9                                  # (tests/test_gpu_condensed.py: 1e-9 against numpy, 1e-8 against dense)


@pytest.mark.parametrize("k", [2, 3])
def test_macro_stars_of_the_generator(cctx, k):
    from alfi_amd import _hostlib
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem
    from alfi_amd.sv import build_sv_hierarchy
    lv, _ = build_sv_hierarchy(TwoDimLidDrivenCavityProblem(2), 1, k, Re=10.0)
    L = lv[-1]
    times = -(-1025 // (len(L.patch_ptr) - 1))
    pp, pd, groups = repeated(L, times, L.patch_groups)
    pl = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, pp, pd, groups)
    print("[P%d]^2 macro stars: %d patches, max_m %d, max_pairs %d, early-load form: %s"
          % (k, len(pp) - 1, pl["max_m"], pl["max_pairs"], takes_ahead(pl)))
    npatch = len(pp) - 1
    assert npatch >= 1025
    full, (split,) = applies(cctx, L, pp, pd, groups, (npatch // 2,), 2)
    assert np.array_equal(split, full)
