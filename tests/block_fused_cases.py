"""What tests/test_block_rhs_fused.py (CPU) and tests/test_gpu_block_rhs_fused.py (GPU) share: the dispatch rule of the block
smoother restated in Python (csrc/block_cols.h: block_smooth_mode, block_partial_per_slot, block_dot_vectors), the rule of the
single smoother it rests on (csrc/api_smoother.hip: smoother_takes_fused_iteration) and the banded levels of the GPU tests."""
import numpy as np

LOOP, LOCKSTEP, FUSED = 0, 1, 2
BLOCK_NV = 4
RED_BLOCKS, RED_MAXV = 1024, 32            # csrc/common.h
SMALL_N, SHORT_ROW = 50000, 32             # smoother_takes_fused_iteration


def block_smooth_mode(block_kernels, block_fused, partitioned, fused_iteration, applies_il, apply_waves, piece_width):
    if not block_kernels or partitioned:
        return LOOP
    if not fused_iteration:
        return LOCKSTEP
    if not block_fused:
        return LOOP
    return FUSED if applies_il or apply_waves != 0 or piece_width >= 2 else LOOP


def block_partial_per_slot(red_blocks=RED_BLOCKS, red_maxv=RED_MAXV):
    return 2 * red_blocks * red_maxv


def block_dot_vectors(nvec):
    if nvec < 1 or nvec > 16:
        return 0
    return 4 if nvec <= 4 else 8 if nvec <= 8 else 16


def takes_fused_iteration(n, max_row_blocks, k):
    """a serial additive level with a flat operator"""
    return k + 1 <= 16 and (max_row_blocks <= SHORT_ROW or n <= SMALL_N)


def spmv_dot_lanes(bs, nnzb, nbrows):
    """LPR of launch_bsr_spmv_dot (kernels_vec.hip)"""
    avg = nnzb / nbrows
    if bs == 2:
        return 4 if avg <= 12 else 8 if avg <= 40 else 32
    return 8 if avg <= 24 else 16 if avg <= 48 else 32


def red_blocks_for(n):
    return min(max((n + 4095) // 4096, 1), RED_BLOCKS)


def banded_operator(nb, half, bs, seed):
    """nb block rows of block size bs, block columns i - half .. i + half, diagonally dominant"""
    from alfi_amd.problem import BSR
    rng = np.random.default_rng(seed)
    cols = np.arange(nb)[:, None] + np.arange(-half, half + 1)[None, :]
    ok = (cols >= 0) & (cols < nb)
    rowptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int32)
    colidx = cols[ok].astype(np.int32)
    vals = (0.5 / (2 * half + 1)) * rng.standard_normal((len(colidx), bs, bs))
    diag = colidx == np.repeat(np.arange(nb), ok.sum(axis=1))
    vals[diag] += 4.0 * np.eye(bs)
    return BSR(nb, nb, bs, rowptr, colidx, vals)


def window_patches(nb, bs, nodes, count, seed):
    """count windows of `nodes` consecutive nodes (nodes x bs dofs each), sorted starts, every node from 5 on may be covered"""
    rng = np.random.default_rng(seed)
    starts = np.sort(rng.integers(5, nb - nodes, count))
    m = nodes * bs
    ptr = (m * np.arange(count + 1)).astype(np.int64)
    dofs = (bs * starts[:, None] + np.arange(m)[None, :]).ravel().astype(np.int32)
    return ptr, dofs


# (bs, half-bandwidth) -> lanes per row of the product with dots, on NB block rows (a multiple of no 256 / LPR; bs 3: n odd)
NB = 1003
BANDS = {(2, 2): 4, (2, 10): 8, (2, 25): 32, (3, 5): 8, (3, 20): 16, (3, 30): 32}
# the grid-stride level: more block rows than RED_BLOCKS workgroups of 256 / 4 rows take in one pass
NB_STRIDE = 70001
