"""The scratch offsets of the large-patch inversion are made on the device (``big_offsets_kernel``: a one-wave scan over the
patch sizes, 64 patches per step with a carry).  A wrong offset puts a patch's matrix on top of another's, so every inverse of
a batch of MORE than 64 large patches of mixed sizes is compared with NumPy (-m gpu): 150 patches of 162 .. 398 dofs, i.e.
padded sizes 192, 256, 320, 384 and 448 in no particular order, three scan steps, the last one partial.

Tolerance: that of tests/test_gpu_parity.py's large-patch test, which inverts the same kind of operator (random, diagonally
dominant, condition number of a patch below 10) with the same kernels: 1e-10 max|A_p^-1|."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_every_inverse_of_150_large_patches_of_mixed_sizes():
    import scipy.sparse as sp
    from alfi_amd import hip
    from alfi_amd.problem import BSR
    bs, nb, npatch = 2, 400, 150
    rng = np.random.default_rng(3)
    M = sp.random(nb * bs, nb * bs, density=0.02, random_state=5, format="csr")
    M = M + M.T + sp.identity(nb * bs) * 30.0
    A = BSR.from_scipy(sp.csr_matrix(M), bs)
    S = A.to_scipy().tocsr()
    sizes = rng.integers(81, 200, npatch)                 # nodes per patch: 162 .. 398 dofs, all beyond the small-patch path
    sizes[[0, 63, 64, 127, 128, 149]] = [199, 81, 199, 81, 130, 199]       # both extremes at the edges of the scan steps
    ptr, dofs = [0], []
    for sz in sizes:
        nodes = np.sort(rng.choice(nb, sz, replace=False))
        d = (nodes[:, None] * bs + np.arange(bs)).ravel()
        dofs.append(d)
        ptr.append(ptr[-1] + len(d))
    ptr, dofs = np.array(ptr, dtype=np.int64), np.concatenate(dofs).astype(np.int32)
    ctx = hip.Context(0)
    try:
        lvl = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
        lvl.set_patches(ptr, dofs)
        lvl.factor()
        worst = 0.0
        for p in range(npatch):
            d = dofs[ptr[p]:ptr[p + 1]]
            Ainv = np.linalg.inv(S[d][:, d].toarray())
            err = np.abs(lvl.patch_inverse(p, len(d)) - Ainv).max() / np.abs(Ainv).max()
            worst = max(worst, err)
            assert err < 1e-10, (p, len(d), err)
        print("150 large patches, worst relative error of an inverse %.2e" % worst)
        lvl.close()
    finally:
        ctx.close()
