"""Helpers of the Krylov tests (tests/test_gpu_krylov.py, tests/test_gpu_parity.py): synthetic block operators with patch
smoothers that NumPy can invert and apply vectorised, the branch predicates of the FGMRES smoother (csrc/api_smoother.hip,
csrc/kernels_vec.hip) mirrored in Python, and the oracle multigrid fed with the device's own inverses."""
import math

import numpy as np

# csrc/common.h and csrc/api_smoother.hip
RED_BLOCKS = 1024
RED_MAXV = 32
SMALL_N = 50000


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- branch predicates of alfi_smooth_fgmres (unpartitioned, additive levels) ---------------------------------------------
def red_blocks_for(n):
    """Partials per vector of the two-stage reductions (kernels_vec.hip: red_blocks_for)."""
    return min(max(math.ceil(n / 4096), 1), RED_BLOCKS)


def spmv_dot_lpr(bs, avg):
    """Lanes per block row of the fused product (kernels_vec.hip: launch_bsr_spmv_dot)."""
    if bs == 2:
        return 4 if avg <= 12 else (8 if avg <= 40 else 32)
    return 8 if avg <= 24 else (16 if avg <= 48 else 32)


def smoother_path(n, max_row_blocks, k):
    """'fused' (four launches per iteration), 'general-consumer' (the dot partials summed inside the consumer kernel) or
    'general-separate' (one-block reduction launches)."""
    short_rows = max_row_blocks <= 32 or n <= SMALL_N
    if k + 1 <= 16 and short_rows:
        return "fused"
    return "general-consumer" if red_blocks_for(n) <= 256 and k + 1 <= 16 else "general-separate"


def smoother_launch_counts(path, k, nonzero_guess):
    """(MATMULT, BLAS1) profiler regions of one alfi_smooth_fgmres call on the level (csrc/api_smoother.hip)."""
    z = 0 if nonzero_guess else 1
    if path == "fused":
        return (1 - z) + k, z + 1 + k + 1
    return (1 - z) + k, z + 2 + 3 * k + 1


# ---- synthetic levels ----------------------------------------------------------------------------------------------------
class SyntheticLevel(object):
    """A random block operator on ``nb`` nodes (``bs`` x ``bs`` blocks) with the given block-row lengths, strongly diagonally
    dominant -- the diagonal blocks are I + 0.1 noise, the off-diagonal part of every row has Frobenius norm ``rho`` -- so
    that LAPACK's and the device's patch inverses agree to ~1e-15 and block-Jacobi preconditioned FGMRES contracts by about
    ``rho`` per iteration (every iteration still matters after 31 of them).  Patches: ``m`` consecutive nodes, starting at
    every ``step``-th node (step < m: overlapping patches)."""

    def __init__(self, nb, bs, row_len, m=1, step=1, nbc=3, seed=0, rho=0.9):
        rng = np.random.default_rng(seed)
        self.nb, self.bs, self.n = nb, bs, nb * bs
        row_len = np.minimum(np.asarray(row_len, dtype=np.int64), nb)
        maxlen = int(row_len.max())
        # distinct column offsets: 0 first (the diagonal), then random ones; row i takes the first row_len[i] of them
        offs = np.concatenate([[0], rng.choice(np.arange(1, nb), maxlen - 1, replace=False)]).astype(np.int64)
        rowptr = np.concatenate([[0], np.cumsum(row_len)])
        nnzb = int(rowptr[-1])
        rows = np.repeat(np.arange(nb), row_len)
        pos = np.arange(nnzb) - rowptr[rows]
        cols = (rows + offs[pos]) % nb
        order = np.lexsort((cols, rows))
        rows, cols, pos = rows[order], cols[order], pos[order]
        vals = rng.standard_normal((nnzb, bs, bs))
        offd = np.maximum(row_len - 1, 1) * bs * bs
        vals *= (rho / np.sqrt(offd))[rows][:, None, None]
        diag = pos == 0
        vals[diag] = np.eye(bs) + 0.1 * rng.standard_normal((int(diag.sum()), bs, bs)) / bs
        from alfi_amd.problem import BSR
        import scipy.sparse as sp
        self.A = BSR(nb, nb, bs, rowptr, cols, vals)
        self.S = sp.bsr_matrix((self.A.vals, self.A.colidx, self.A.rowptr), shape=(self.n, self.n))
        self.avg = nnzb / nb
        self.max_row = maxlen
        self.keys = rows.astype(np.int64) * nb + cols          # sorted: lexsort by (row, col)
        # patches of m consecutive nodes
        starts = np.arange(0, nb - m + 1, step)
        self.pnodes = starts[:, None] + np.arange(m)[None, :]
        self.pdofs = (self.pnodes[:, :, None] * bs + np.arange(bs)).reshape(len(starts), m * bs)
        self.patch_ptr = np.arange(len(starts) + 1, dtype=np.int64) * (m * bs)
        self.patch_dofs = self.pdofs.ravel().astype(np.int32)
        self.bc = np.sort(rng.choice(self.n, nbc, replace=False)).astype(np.int32) if nbc else np.zeros(0, np.int32)
        self.count = np.bincount(self.patch_dofs, minlength=self.n)
        # patch matrices A[p][p] from the block list, inverted all at once
        npatch = len(starts)
        Ap = np.zeros((npatch, m, bs, m, bs))
        for a in range(m):
            for b in range(m):
                key = self.pnodes[:, a] * nb + self.pnodes[:, b]
                at = np.minimum(np.searchsorted(self.keys, key), nnzb - 1)
                hit = self.keys[at] == key
                Ap[hit, a, :, b, :] = vals[at[hit]]
        self.inv = np.linalg.inv(Ap.reshape(npatch, m * bs, m * bs))

    def matvec(self, x):
        return self.S @ x

    def smoother(self, pou=False):
        """The additive patch smoother (oracle.alfi_oracle.PatchSmoother.apply_additive), vectorised."""
        def apply(x):
            Y = np.einsum("pij,pj->pi", self.inv, x[self.pdofs])
            y = np.bincount(self.patch_dofs, weights=Y.ravel(), minlength=self.n)
            if pou:
                y /= np.maximum(self.count, 1)
            y[self.bc] = x[self.bc]
            return y
        return apply

    def device_level(self, ctx, pou=False):
        from alfi_amd import hip
        dl = hip.Level(ctx, self.A, self.bc)
        dl.set_patches(self.patch_ptr, self.patch_dofs)
        if pou:
            dl.set_partition_of_unity(True)
        dl.factor()
        return dl


# ---- the oracle multigrid with the device's inverses ----------------------------------------------------------------------
def oracle_mg_with_device_inverses(lv, tr, k, dmg, coarse_inv, schoeberl_restriction=True):
    """Oracle multigrid (oracle.alfi_oracle.build_oracle_mg) that applies the DEVICE's patch inverses
    (alfi_patch_get_inverse), interior-block inverses of the transfers (alfi_transfer_get_block_inverse) and the explicit
    coarse inverse ``coarse_inv`` in place of its LAPACK / sparse LU ones: what is left to differ from ``dmg`` is the order
    of floating-point sums."""
    from oracle import alfi_oracle as O
    omg = O.build_oracle_mg(lv, tr, k, schoeberl_restriction=schoeberl_restriction)
    for L, dl, ol in list(zip(lv, dmg.levels, omg.levels))[1:]:
        n = np.diff(L.patch_ptr)
        ol["smoother"].inv = [dl.patch_inverse(p, int(n[p])) for p in range(len(n))]
    for dt, ot in zip(dmg.transfers, omg.transfers):
        m = ot.st.blk_dofs.shape[1]
        binv = [dt.block_inverse(b, m) for b in range(ot.st.blk_dofs.shape[0])]
        # the oracle solves with LU factors; feed it exact "LU factors" of the device inverse's action instead
        ot.st.lu = None
        ot.st._binv = binv

        def patch_apply(x, st=ot.st):
            y = np.zeros_like(x)
            for d, X in zip(st.blk_dofs, st._binv):
                y[d] = X @ x[d]
            y[st.skel] = x[st.skel]
            return y
        ot.st._patch_apply = patch_apply

    class _Coarse(object):
        @staticmethod
        def solve(v):
            return coarse_inv @ v
    omg.coarse_lu = _Coarse()
    return omg
