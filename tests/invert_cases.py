"""Synthetic levels that send every dense patch-inversion kernel through every size it serves, with the pivoted repair of
kernels_check.hip out of the picture.  Host only (numpy + alfi_amd.problem); shared by tests/test_invert_cases.py (CPU) and
tests/test_gpu_invert_sizes.py with its worker.

alfi_patches_factor picks the inversion kernel from the LEVEL's largest patch (launch_patch_invert_arrays,
launch_patch_invert_mfma, launch_big_factor) and every instantiation serves all sizes from 1 up to its cap, so a level whose
patches have 1, 2, ..., M dofs exercises one instantiation at every size.  hip.Level.set_patches takes any strictly ascending
dof subset of any operator: no mesh is needed.

operator(bs)    one dense 288 x 288 operator per block size (3: 96 nodes, 2: 144 nodes; its own seed each),
                    A = Q diag(logspace(0, 3, 288)) Q^T + (G - G^T) 30 / sqrt(288),
                non-symmetric with the positive definite symmetric part Q diag Q^T: every principal submatrix (and every
                Schur complement inside it) keeps a positive definite symmetric part, so the unpivoted scalar, 4 x 4-block and
                64 x 64-block eliminations all exist.  cond(A[D, D]) <= 1e3 (tests/test_invert_cases.py); measured: at most
                1.3e2 for either operator over the subsets in use.  Nothing like the real patch operators (cond ~ 1e7), on
                purpose: the error floor is ~1e-15, anything a kernel gets wrong stands out by orders of magnitude.
dofs(n)         the fixed subset D_n = sort(default_rng(1000 + n).choice(288, n, replace=False)), the same on every level.
levels()        {max_np: patch sizes}; the patch of size n is always D_n.
reference(bs, n)  inv(A[D_n, D_n]) in extended precision: LAPACK's inverse + two Newton-Schulz steps X <- X + X (I - A X) in
                np.longdouble.  Measured: max |A X - I| <= 2.6e-18 after the two steps (x86 80-bit long double); all sizes of
                both operators take ~15 s on the host, so they are cached.
tolerance()     32 x the worst, over both operators and all sizes in use, of max |inv_LAPACK - X_ref| / max |X_ref|: the error of
                the float64 PIVOTED inverse against the extended one, computed when the test runs.  Measured: LAPACK 1.6e-15
                (bs 3) and 1.7e-15 (bs 2), so the bound is 5.4e-14; a plain float64 unpivoted Gauss-Jordan in the kernels'
                elimination order: 3.2e-15 (bs 3) and 3.0e-15 (bs 2), 2 x LAPACK.  The factor 32 covers another summation order
                (rank-4 MFMA updates, 64-wide blocked steps), the <= 1 ulp reciprocal of the MFMA kernel and the polish of the
                blocked path -- and stays seven orders below the residual probe's 1e-6: an inversion that is wrong but quietly
                repaired, or wrong below the probe's threshold, cannot pass.

A NEW inversion or apply kernel, or a new dispatch threshold, gets its case HERE: a cap at the threshold and one above it in
MID_CAPS / SMALL_COUNTS / BLOCKED_SIZES."""
import functools

import numpy as np

NDOF = 288

# max_np <= 32: invert_small_kernel<8 | 16 | 32, true> (N lanes per patch, 256 / N patches per workgroup) and the interleaved
# copy of the apply (build_patch_il: G = 4, 7, 8, 12, 16 lanes per patch for these five caps, 64 / G patches per wave, four
# waves per workgroup).  cap -> number of patches: the sizes 1 .. cap over and over, cut at a count that is a multiple neither of
# 64 / G nor of 256 / N (partial last wave / workgroup) and spans several workgroups of both kernels.  (Whole repeats cannot do
# that for the caps 16 and 32 -- 16 r is a multiple of 8 -- so the last pass stops after three patches.)
SMALL_COUNTS = {8: 72, 14: 42, 16: 35, 24: 51, 32: 67}
# every cap and cap + 1 of patch_invert_big_kernel<7 | 10> (<= 112, <= 160) and patch_invert_mfma_kernel<4 | 6 | 8 | 10>
# (<= 64, <= 96, <= 128, <= 160); 33 is the first size above the small kernels
MID_CAPS = (33, 64, 65, 96, 97, 112, 113, 128, 129, 160)
# launch_big_factor (max_np > 160): 64-wide pivot blocks + Newton-Schulz polish
BLOCKED_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 160, 161, 162, 191, 192, 193, 255, 256, 257)


def il_lanes(max_np):
    """G of build_patch_il (kernels_patch.hip)."""
    need = (max_np + 1) // 2
    return 4 if need <= 4 else 7 if need <= 7 else 8 if need <= 8 else 12 if need <= 12 else 16


def small_width(max_np):
    """N of launch_invert_small_any (kernels_patch.hip)."""
    return 8 if max_np <= 8 else 16 if max_np <= 16 else 32


@functools.lru_cache(maxsize=None)
def dense(bs):
    """The dense 288 x 288 operator of block size bs (read-only)."""
    assert bs in (2, 3)
    rng = np.random.default_rng(20 + bs)
    Q, _ = np.linalg.qr(rng.standard_normal((NDOF, NDOF)))
    G = rng.standard_normal((NDOF, NDOF))
    A = (Q * np.logspace(0.0, 3.0, NDOF)) @ Q.T + (G - G.T) * (30.0 / np.sqrt(NDOF))
    A.setflags(write=False)
    return A


def operator(bs):
    from alfi_amd.problem import BSR
    return BSR.from_scipy(dense(bs), bs)


@functools.lru_cache(maxsize=None)
def dofs(n):
    d = np.sort(np.random.default_rng(1000 + n).choice(NDOF, n, replace=False)).astype(np.int32)
    d.setflags(write=False)
    return d


def levels():
    """{max_np: tuple of patch sizes}, in the order the worker runs them."""
    out = {}
    for cap, count in SMALL_COUNTS.items():
        out[cap] = tuple(1 + i % cap for i in range(count))
    for cap in MID_CAPS:
        out[cap] = tuple(range(1, cap + 1))
    out[max(BLOCKED_SIZES)] = BLOCKED_SIZES
    return out


def sizes_in_use():
    return sorted({n for sizes in levels().values() for n in sizes})


def patch_arrays(sizes):
    """(patch_ptr int64, patch_dofs int32) of the level whose patches are D_n for n in sizes."""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return ptr, np.concatenate([dofs(n) for n in sizes]).astype(np.int32)


def submatrix(bs, n):
    d = dofs(n)
    return dense(bs)[np.ix_(d, d)]


@functools.lru_cache(maxsize=None)
def _reference(bs, n):
    A = submatrix(bs, n)
    X64 = np.linalg.inv(A)
    Al, X, I = A.astype(np.longdouble), X64.astype(np.longdouble), np.eye(n, dtype=np.longdouble)
    for _ in range(2):
        X = X + X @ (I - Al @ X)
    lapack_err = float(np.abs(X64 - X).max() / np.abs(X).max())
    X.setflags(write=False)
    return X, lapack_err


def reference(bs, n):
    """inv(A[D_n, D_n]) as np.longdouble (read-only, cached)."""
    return _reference(bs, n)[0]


def lapack_error(bs, n):
    """max |inv_LAPACK - X_ref| / max |X_ref| of that patch."""
    return _reference(bs, n)[1]


@functools.lru_cache(maxsize=None)
def tolerance():
    return 32.0 * max(lapack_error(bs, n) for bs in (3, 2) for n in sizes_in_use())


def apply_input():
    """The seeded level vector the worker applies the patch solves to."""
    return np.random.default_rng(4242).standard_normal(NDOF)
