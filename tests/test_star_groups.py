"""The group finder behind the automatically condensed vertex-star factors (csrc/find_groups.h, alfi_patches_find_groups) on
the host: libalfi_host.so exports the same function (alfi_host_find_groups).  No GPU.

Shapes: ldc3d [P2+FB]^3, N = 4 (125 patches: 27 full stars and every boundary shape of 3 / 9 / 21 / 33 / 57 dofs) and N = 8."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def levels():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    lv, _ = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)
    return lv[1:]


def _labels(L):
    from alfi_amd import _hostlib
    return _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)


def test_star_patches_get_six_groups_of_fifteen(levels):
    seen = set()
    for L in levels:
        g = _labels(L)
        assert g.dtype == np.int32 and len(g) == len(L.patch_dofs)
        assert np.array_equal(g, _labels(L))                                  # deterministic
        for p in range(len(L.patch_ptr) - 1):
            lab = g[L.patch_ptr[p]:L.patch_ptr[p + 1]]
            n = len(lab)
            seen.add(n)
            sizes = sorted(np.bincount(lab[lab >= 0]).tolist()) if (lab >= 0).any() else []
            if n == 153:
                assert sizes == [15] * 6 and (lab < 0).sum() == 63, (p, sizes)
            elif n == 57:
                assert sizes == [15] * 2 and (lab < 0).sum() == 27, (p, sizes)
            else:
                assert n <= 33 and sizes == [], (p, n, sizes)
            assert np.array_equal(lab.reshape(-1, L.bs), np.repeat(lab[::L.bs, None], L.bs, axis=1))    # one label per node
    assert seen == {3, 9, 21, 33, 57, 153}


def test_groups_touch_each_other_only_through_the_skeleton_and_shrink_the_factors(levels):
    L = levels[0]
    g = _labels(L)
    S = L.A.to_scipy().tocsr()
    for p in range(len(L.patch_ptr) - 1):
        sl = slice(L.patch_ptr[p], L.patch_ptr[p + 1])
        dofs, lab = L.patch_dofs[sl], g[sl]
        if not (lab >= 0).any():
            continue
        Ap = S[dofs][:, dofs].toarray()
        n, s = len(dofs), int((lab < 0).sum())
        doubles = s * s
        for a in range(lab.max() + 1):
            ia = np.flatnonzero(lab == a)
            for b in range(a + 1, lab.max() + 1):
                ib = np.flatnonzero(lab == b)
                assert not Ap[np.ix_(ia, ib)].any() and not Ap[np.ix_(ib, ia)].any()
            sk = np.flatnonzero(lab < 0)
            sc = int((np.abs(Ap[np.ix_(ia, sk)]).sum(axis=0) + np.abs(Ap[np.ix_(sk, ia)]).sum(axis=1) > 0).sum())
            assert len(ia) <= 64 and sc <= 64
            doubles += len(ia) ** 2 + 2 * len(ia) * sc
        assert doubles <= 0.75 * n * n
        if n == 153:
            assert doubles == 10179                                           # 6 (15^2 + 2 15 27) + 63^2 of 153^2 = 23 409


def test_patches_that_are_not_whole_nodes_stay_dense(levels):
    from alfi_amd import _hostlib
    L = levels[0]
    p = int(np.flatnonzero(np.diff(L.patch_ptr) == 153)[0])
    dofs = L.patch_dofs[L.patch_ptr[p]:L.patch_ptr[p + 1]]
    g = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, np.array([0, 152, 305]), np.concatenate([dofs[1:], dofs]))
    assert (g[:152] == -1).all() and sorted(np.bincount(g[152:][g[152:] >= 0]).tolist()) == [15] * 6
