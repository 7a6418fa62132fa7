"""``composed_injection`` (alfi_amd.dist_nssolver): the rows of I_level ... I_nlev-2 that ``StateExchange`` turns into a level's
gather from the finest velocity, against the level-by-level injection of ``HipNavierStokesSolver._winds``.  CPU only.

Tolerance 1e-13 max|u|: both sides are sums of at most 81 products (<= 9 entries per injection row, two injections composed)
with |w| <= 1 in different orders, so they differ by a few hundred eps at the very most; measured 2.3e-16."""
import numpy as np
import pytest

from alfi_amd.dist_nssolver import composed_injection
from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem, build_hierarchy
from alfi_amd.sv import build_sv_hierarchy


_made = {}


def _sv(name):
    """(levels, transfers, the field on every level) of a Scott-Vogelius hierarchy, built once per module."""
    if name not in _made:
        _made[name] = _build(name)
    return _made[name]


@pytest.fixture(params=["2d-k2", "3d-k3"])
def sv_case(request):
    return _sv(request.param)


def _build(name):
    prob, nref, k = ((TwoDimLidDrivenCavityProblem(4), 2, 2) if name == "2d-k2" else (ThreeDimLidDrivenCavityProblem(1), 2, 3))
    levels, transfers = build_sv_hierarchy(prob, nref, k, Re=0.0, patches=False)
    rng = np.random.default_rng(12)
    u = rng.uniform(-1.0, 1.0, (levels[-1].A.nbrows, prob.dim))
    winds = [None] * len(levels)           # the level-by-level injection (nssolver._winds), once
    winds[-1] = u
    for l in range(len(levels) - 1, 0, -1):
        winds[l - 1] = transfers[l - 1].inject_matrix @ winds[l]
    return levels, transfers, winds


def _row_sets(n, seed):
    return [np.arange(n), np.sort(np.random.default_rng(seed).choice(n, n // 3, replace=False))]


def test_composed_rows_equal_the_level_by_level_injection(sv_case):
    levels, transfers, winds = sv_case
    nlev, u = len(levels), winds[-1]
    assert nlev == 3
    for l in range(nlev - 1):
        for rows in _row_sets(levels[l].A.nbrows, 100 + l):
            C = composed_injection(transfers, nlev, l, rows)
            assert C.shape == (rows.size, u.shape[0]) and C.has_sorted_indices
            err = np.abs(C @ u - winds[l][rows]).max()
            print("level %d, %d rows: max nnz per row %d, error %.2e" % (l, rows.size, np.diff(C.indptr).max(), err))
            assert err <= 1e-13 * np.abs(u).max()
            assert np.abs(np.asarray(C.sum(axis=1)).ravel() - 1.0).max() <= 1e-13


def test_true_interpolation_rows_are_present_in_3d():
    """[P3]^3: not every coarse node is a fine node -- the case an index gather cannot serve."""
    levels, transfers, _ = _sv("3d-k3")
    C = composed_injection(transfers, 3, 0, np.arange(levels[0].A.nbrows))
    assert np.diff(C.indptr).max() > 1 and C.data.min() < 0.0


def test_finest_level_gives_identity_rows(sv_case):
    levels, transfers, _ = sv_case
    rows = np.array([5, 0, 17])
    C = composed_injection(transfers, 3, 2, rows)
    assert C.shape == (3, levels[-1].A.nbrows)
    assert np.array_equal(C.indices, rows) and np.array_equal(C.indptr, [0, 1, 2, 3]) and (C.data == 1.0).all()


def test_nested_hierarchy_gives_the_composed_inject_map():
    levels, transfers = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=0.0)
    nlev = len(levels)
    to_fine = np.arange(levels[-1].A.nbrows)
    for l in range(nlev - 2, -1, -1):
        to_fine = to_fine[np.asarray(transfers[l].inject_map, dtype=np.int64)]
        for rows in _row_sets(levels[l].A.nbrows, 200 + l):
            C = composed_injection(transfers, nlev, l, rows)
            assert C.shape == (rows.size, levels[-1].A.nbrows)
            assert np.array_equal(C.indptr, np.arange(rows.size + 1))
            assert (C.data == 1.0).all()
            assert np.array_equal(C.indices, to_fine[rows])
