"""Synthetic levels of dense MACRO-STAR inverses (patches above 160 dofs) for the block right-hand sides of
kernels_block_big.hip.  Host only (numpy + alfi_amd.problem); shared by tests/test_gpu_block_rhs_macro.py.

operator()   tests/invert_cases.dense at 2736 dofs (bs 3: 912 nodes): A = Q diag(logspace(0, 3, 2736)) Q^T + (G - G^T) 30 / sqrt(2736),
             non-symmetric with a positive definite symmetric part, so every principal submatrix has an unpivoted blocked
             elimination and cond <= ~1e3.
dofs(n)      the fixed subset sort(default_rng(5000 + n).choice(2736, n, replace=False)), the same on every level.
LEVELS       name -> patch sizes.  Every level has 8 .. 16 patches; the large sizes of a level are few (one 2731-dof inverse is 60 MB),
             the rest are small stars that ride along (the macro stars' kernel serves every size from 1 up).  The sizes are the
             smallest at which the block kernel can go wrong: piece boundaries (128-row pieces and the binary digits of the
             remainder), n mod 4 = 0 .. 3 for the guarded FP32 store, odd n for the pad row of the FP64 pair store, and one level
             per value of big_split (workgroups per patch, patch_plan.h) and per width class of the default 64 KiB budget.
"""
import functools

import numpy as np

NDOF = 2736
BS = 3
DEFAULT_LDS_BUDGET = 64 * 1024

LEVELS = {
    "D": (161, 162, 163, 191, 192, 193, 255, 256, 257, 512, 40, 100),
    "E": (513, 640, 641, 161, 300, 77, 258, 400),
    "F": (1153, 1154, 1155, 200, 333, 130, 514, 259),
    "A": (2047, 2048, 170, 385, 97, 260, 131, 642),
    "B": (2049, 170, 385, 97, 260, 131, 642, 1025),
    "C": (2731, 170, 385, 97, 260, 131, 642, 1025),
}
# name -> (big_split of the level, width at the default budget): the table of the width rule (csrc/block_cols.h) and of the
# single launcher's work split
EXPECTED = {"D": (1, 4), "E": (2, 4), "F": (3, 4), "A": (4, 4), "B": (5, 3), "C": (6, 2)}
# every patch <= 64 dofs and one above 32: one wave per patch through patch_apply_kernel (kernels_block.hip batches it)
SMALL_STARS = (33, 47, 64, 40, 50, 60, 35, 45)


def block_big_lds(max_np, nv):
    """csrc/block_cols.h: bytes of LDS of a workgroup of the block kernel for nv columns"""
    return nv * 8 * ((max_np + 1) & ~1)


def block_big_width(max_np, budget=DEFAULT_LDS_BUDGET):
    for nv in (4, 3, 2):
        if budget > 0 and block_big_lds(max_np, nv) <= budget:
            return nv
    return 0


def big_split(npatch, max_np):
    """csrc/patch_plan.h"""
    want = (2048 + npatch - 1) // npatch
    cap = ((max_np + 127) // 128 + 3) // 4
    return max(1, min(want, cap))


@functools.lru_cache(maxsize=None)
def dense():
    rng = np.random.default_rng(23)
    Q, _ = np.linalg.qr(rng.standard_normal((NDOF, NDOF)))
    G = rng.standard_normal((NDOF, NDOF))
    A = (Q * np.logspace(0.0, 3.0, NDOF)) @ Q.T + (G - G.T) * (30.0 / np.sqrt(NDOF))
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def operator():
    """the dense operator as one BSR with every block stored (built directly: 912 x 912 blocks of 3 x 3)"""
    from alfi_amd.problem import BSR
    nb = NDOF // BS
    vals = np.ascontiguousarray(dense().reshape(nb, BS, nb, BS).transpose(0, 2, 1, 3).reshape(nb * nb, BS, BS))
    rowptr = (nb * np.arange(nb + 1)).astype(np.int32)
    colidx = np.tile(np.arange(nb, dtype=np.int32), nb)
    return BSR(nb, nb, BS, rowptr, colidx, vals)


@functools.lru_cache(maxsize=None)
def dofs(n):
    d = np.sort(np.random.default_rng(5000 + n).choice(NDOF, n, replace=False)).astype(np.int32)
    d.setflags(write=False)
    return d


def patch_arrays(sizes):
    """(patch_ptr int64, patch_dofs int32) of the level whose patches are dofs(n) for n in sizes"""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return ptr, np.concatenate([dofs(n) for n in sizes]).astype(np.int32)
