"""The group finder (csrc/find_groups.h) on the rank-local levels of a partitioned hierarchy: what lets a partitioned level condense
its vertex-star factors by itself (alfi_patches_factor looks for groups in the rank's own sparsity and patch lists, no
collective).  No GPU: libalfi_host.so exports the finder and the planner the device library runs.

Shapes: ldc3d [P2+FB]^3, N = 2, nref 2, Re 1000 (tests/test_star_groups.py): levels 1 and 2 with 125 / 729 patches, split over 2
and 3 ranks with every level partitioned (min_dofs = 1).  A ghost patch holds dofs of nodes another rank owns: they are numbered
behind the owned nodes, so the finder may seed its groups elsewhere than on the global level -- the number of groups per patch
is the same, which dofs a group takes need not be."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def hier():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)


@pytest.fixture(scope="module")
def global_counts(hier):
    """level -> groups per patch of the global level"""
    from alfi_amd import _hostlib
    out = {}
    for L in hier[0][1:]:
        g = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)
        out[L.level] = _groups_per_patch(L.patch_ptr, g)
    return out


def _groups_per_patch(ptr, g):
    return np.array([len(np.unique(lab[lab >= 0])) for lab in np.split(g, ptr[1:-1])], dtype=np.int64)


@pytest.mark.parametrize("world", [2, 3])
def test_rank_local_levels_find_the_groups_of_the_global_level(hier, global_counts, world):
    from alfi_amd import _hostlib
    from alfi_amd.dist import build_parts, choose_splits, localize_level
    lv, tr = hier
    splits = choose_splits(lv, world, 1)
    seen = {L.level: np.zeros(len(L.patch_ptr) - 1, dtype=np.int64) for L in lv[1:]}
    ghost_patches = {L.level: [0, 0] for L in lv[1:]}                            # [ghost patches, grouped among them]
    for rank in range(world):
        parts = build_parts(lv, tr, splits, rank, None)
        for L in lv[1:]:
            part = parts[L.level]
            assert part.distributed and part.nb_own > 0
            LL = localize_level(L, part)
            npatch = len(LL.patch_ptr) - 1
            assert npatch > 0
            g = _hostlib.find_groups(LL.bs, LL.A.rowptr, LL.A.colidx, LL.patch_ptr, LL.patch_dofs)
            assert g.dtype == np.int32 and len(g) == len(LL.patch_dofs)
            # one label per node
            assert np.array_equal(g.reshape(-1, LL.bs), np.repeat(g[::LL.bs, None], LL.bs, axis=1))
            cnt = _groups_per_patch(LL.patch_ptr, g)
            # the same patches are grouped, each into as many groups as on the global level
            assert np.array_equal(cnt, global_counts[L.level][LL.patch_ids]), (world, rank, L.level)
            seen[L.level][LL.patch_ids] += 1
            ghost = np.arange(npatch) >= LL.npatch_int
            ghost_patches[L.level][0] += int(ghost.sum())
            ghost_patches[L.level][1] += int((cnt[ghost] > 0).sum())
            # the planner accepts the rank's level: groups and their skeleton couplings of at most 64 dofs, factors below dense
            plan = _hostlib.plan_condensed(LL.bs, LL.A.rowptr, LL.A.colidx, LL.patch_ptr, LL.patch_dofs, g)
            assert plan["ngroups"] == cnt.sum() and len(plan["g_m"]) == plan["ngroups"]
            assert plan["max_m"] <= 64 and plan["g_sc"].max() <= 64
            n = np.diff(LL.patch_ptr)
            dense = int(((n * ((n + 1) & ~1) + 15) & ~15).sum())                  # inv_doubles of csrc/patch_plan.h
            assert plan["mat_doubles"] + plan["sinv_doubles"] < dense
    for L in lv[1:]:
        assert (seen[L.level] == 1).all()                                         # every patch on exactly one rank
        grouped = int((global_counts[L.level] > 0).sum())
        print("world %d level %d: %d of %d patches grouped, %d of %d ghost patches" %
              (world, L.level, grouped, len(seen[L.level]), ghost_patches[L.level][1], ghost_patches[L.level][0]))
        assert grouped == {1: 81, 2: 637}[L.level]
        assert ghost_patches[L.level][1] > 0                                      # the ghost patches are part of the check
