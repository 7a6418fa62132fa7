"""The synthetic levels of tests/invert_cases.py stay inside the conditions tests/test_gpu_invert_sizes.py relies on -- checked
on the host, no GPU code: the patch matrices are well conditioned, an UNPIVOTED float64 elimination of every one of them meets
the run-time tolerance (so a correct kernel can), the extended-precision reference is converged, and the small-patch levels
have the awkward patch counts they are there for."""
import numpy as np
import pytest

from tests import invert_cases as ic


def gauss_jordan(A):
    """In-place Gauss-Jordan inversion without pivoting, in the elimination order of invert_small_kernel /
    patch_invert_big_kernel (kernels_patch.hip): pivot k scales row k, eliminates column k from every other row, and the
    column is replaced by that of the inverse."""
    a = np.array(A, dtype=np.float64)
    n = a.shape[0]
    for k in range(n):
        ip = 1.0 / a[k, k]
        row = a[k, :].copy()
        m = a[:, k] * ip
        m[k] = 0.0
        a -= np.outer(m, row)
        a[:, k] = -m
        a[k, :] = row * ip
        a[k, k] = ip
    return a


@pytest.fixture(scope="module", params=[3, 2], ids=["bs3", "bs2"])
def bs(request):
    return request.param


def test_operator_is_a_dense_level_operator(bs):
    A = ic.operator(bs)
    assert A.bs == bs and A.nbrows == A.nbcols == ic.NDOF // bs and A.nnzb == A.nbrows ** 2
    D = ic.dense(bs)
    assert np.array_equal(A.to_scipy().toarray(), D)
    assert np.abs(D - D.T).max() > 1.0                                   # non-symmetric
    assert np.linalg.eigvalsh(0.5 * (D + D.T)).min() > 0.99              # positive definite symmetric part
    for n in ic.sizes_in_use():
        d = ic.dofs(n)
        assert d.shape == (n,) and np.all(np.diff(d) > 0) and 0 <= d[0] and d[-1] < ic.NDOF


def test_patch_matrices_are_well_conditioned(bs):
    worst = max(np.linalg.cond(ic.submatrix(bs, n)) for n in ic.sizes_in_use())
    print("bs %d: worst cond(A[D_n, D_n]) %.3e" % (bs, worst))
    assert worst <= 1e3


def test_reference_is_converged(bs):
    worst = 0.0
    for n in ic.sizes_in_use():
        X = ic.reference(bs, n)
        assert X.dtype == np.longdouble
        R = ic.submatrix(bs, n).astype(np.longdouble) @ X - np.eye(n, dtype=np.longdouble)
        worst = max(worst, float(np.abs(R).max()))
    print("bs %d: worst max |A X_ref - I| %.3e" % (bs, worst))
    assert worst <= 1e-17


def test_unpivoted_elimination_meets_the_tolerance(bs):
    tol = ic.tolerance()
    worst, worst_lapack = 0.0, 0.0
    for n in ic.sizes_in_use():
        X = ic.reference(bs, n)
        err = float(np.abs(gauss_jordan(ic.submatrix(bs, n)) - X).max() / np.abs(X).max())
        assert err <= tol, "bs %d, n %d: unpivoted Gauss-Jordan off by %.3e (tolerance %.3e)" % (bs, n, err, tol)
        worst, worst_lapack = max(worst, err), max(worst_lapack, ic.lapack_error(bs, n))
    print("bs %d: unpivoted Gauss-Jordan %.3e, LAPACK %.3e, tolerance %.3e" % (bs, worst, worst_lapack, tol))
    assert tol == 32.0 * max(ic.lapack_error(b, n) for b in (3, 2) for n in ic.sizes_in_use())
    assert tol < 1e-12                     # (seven orders below the residual probe's 1e-6, with room)


def test_levels_cover_every_cap_and_the_small_counts_are_awkward():
    lv = ic.levels()
    assert list(lv) == [8, 14, 16, 24, 32, 33, 64, 65, 96, 97, 112, 113, 128, 129, 160, 257]
    for cap, sizes in lv.items():
        assert max(sizes) == cap
        if cap <= 160:
            assert set(sizes) == set(range(1, cap + 1))                  # every size the instantiation serves
    assert lv[257] == (1, 2, 63, 64, 65, 127, 128, 129, 160, 161, 162, 191, 192, 193, 255, 256, 257)
    assert lv[8] == tuple(range(1, 9)) * 9                               # 72 patches
    assert sorted({ic.il_lanes(c) for c in ic.SMALL_COUNTS}) == [4, 7, 8, 12, 16]
    assert sorted({ic.small_width(c) for c in ic.SMALL_COUNTS}) == [8, 16, 32]
    for cap in ic.SMALL_COUNTS:
        count, per_wave, per_wg = len(lv[cap]), 64 // ic.il_lanes(cap), 256 // ic.small_width(cap)
        assert count % per_wave != 0 and count % per_wg != 0, (cap, count)
        assert count > 4 * per_wave and count > per_wg, (cap, count)    # more than one workgroup of the apply / the inversion
    ptr, pd = ic.patch_arrays(lv[14])
    assert ptr[-1] == len(pd) == sum(lv[14]) and np.array_equal(pd[ptr[13]:ptr[14]], ic.dofs(14))
