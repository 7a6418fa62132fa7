"""Operators whose level product de-duplicates its x gathers (bsr_spmv_dedup_kernel) for the block right-hand sides of
bsr_spmv_dedup_block_kernel, and the width rule of csrc/block_cols.h restated in Python.  Host only (numpy + alfi_amd.problem);
shared by tests/test_block_rhs_dedup.py and tests/test_gpu_block_rhs_dedup.py.

Every operator is a square BSR with random values and sorted columns that de-duplicates without any environment switch: at least
1024 blocks (a group of SPMV_WG blocks) and a block row longer than the 256 blocks of a chunk, so that the product takes equal
chunks, the fix-up launch and the staged gathers.

long(nb)       row 0 holds all nb columns (it lies in group 0 and crosses one or more chunks), rows 1 .. nb - 1 three random
               columns each.  nb = 400: 1597 blocks = 1024 + 573, 7 chunks, ONE wave of the last workgroup idle, 400 distinct
               columns at most; nb = 800: 3197 = 3 * 1024 + 125, 13 chunks, THREE waves idle, 800 distinct columns (default
               width 3 at bs 3).
pattern(tail)  rows of 320, 64, 128, 256, 255, 1, 1100, 63 blocks, then rows of ONE block in column 0: row starts at lane 0 of a
               later wave iteration (block 320), exactly on chunk and group boundaries (512, 768, 1024), at lane 63 (block 1023); a
               row that crosses a group boundary and five chunks (the carry runs in the fix-up); a group of 1024 distinct
               columns (default width 2 at bs 3) and one of a single column; a last chunk closed by the end of the operator,
               ragged (nb = 1200: 3379 blocks = 3 * 1024 + 307) or exact (nb = 1917: 4096 blocks).
"""
import functools

import numpy as np

SPMV_CHUNK = 256                     # csrc/common.h: blocks per wave
SPMV_WG = 1024                       # blocks per workgroup (a group)
DEFAULT_LDS_BUDGET = 64 * 1024       # Context.set_block_lds_bytes
PATTERN_ROWS = (320, 64, 128, 256, 255, 1, 1100, 63)
CASES = (("long", 400), ("long", 800), ("pattern", "ragged"), ("pattern", "exact"))


def block_dedup_lds(max_uniq, bs, nv):
    """csrc/block_cols.h: bytes of LDS of a workgroup of the block product for nv columns"""
    return nv * 8 * bs * max_uniq


def block_dedup_width(max_uniq, bs, budget=DEFAULT_LDS_BUDGET):
    for nv in (4, 3, 2):
        if max_uniq > 0 and budget > 0 and block_dedup_lds(max_uniq, bs, nv) <= budget:
            return nv
    return 0


@functools.lru_cache(maxsize=None)
def structure(kind, arg):
    """(nb, rowptr int32, colidx int32) of long(arg) / pattern(arg); seed 0"""
    rng = np.random.default_rng(0)
    if kind == "long":
        nb = int(arg)
        rows = [np.arange(nb)] + [np.sort(rng.choice(nb, 3, replace=False)) for _ in range(nb - 1)]
    else:
        nb = {"ragged": 1200, "exact": 1917}[arg]
        rows = [np.sort(rng.choice(nb, m, replace=False)) for m in PATTERN_ROWS]
        rows += [np.zeros(1, dtype=np.int64) for _ in range(nb - len(PATTERN_ROWS))]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colidx = np.concatenate(rows).astype(np.int32)
    rowptr.setflags(write=False)
    colidx.setflags(write=False)
    return nb, rowptr, colidx


def operator(kind, arg, bs):
    from alfi_amd.problem import BSR
    nb, rowptr, colidx = structure(kind, arg)
    vals = np.random.default_rng(100 + bs).standard_normal((len(colidx), bs, bs))
    return BSR(nb, nb, bs, rowptr, colidx, vals)


def group_distinct(colidx):
    """distinct columns of every group of SPMV_WG consecutive blocks"""
    return [len(np.unique(colidx[k:k + SPMV_WG])) for k in range(0, len(colidx), SPMV_WG)]


def dedups(rowptr):
    """does the product of an operator with these block rows de-duplicate (csrc/api_ctx.hip, kernels_vec.hip)?"""
    nnzb, longest = int(rowptr[-1]), int(np.diff(rowptr).max())
    return np.diff(rowptr).min() > 0 and nnzb >= SPMV_WG and (longest > SPMV_CHUNK or nnzb > 1 << 21)


def expected_width(kind, arg, bs, budget=DEFAULT_LDS_BUDGET):
    _, rowptr, colidx = structure(kind, arg)
    assert dedups(rowptr)
    return block_dedup_width(max(group_distinct(colidx)), bs, budget)
