"""What tests/test_block_rhs_condensed.py (CPU) and tests/test_gpu_block_rhs_condensed.py share: the width rule of the condensed
block apply restated on a host plan (alfi_amd._hostlib.plan_condensed), the waves per patch of the workgroup-per-patch apply,
and the repetition of a patch set -- with its group labels -- up to a wanted number of patches."""
import numpy as np

DEFAULT_LDS_BUDGET = 64 * 1024        # Context.set_block_lds_bytes
PER_PATCH_MIN = 1024                  # csrc/cond_layout.h: COND_PER_PATCH_MIN


def lds_per_column(plan):
    """LDS of the one-vector front / back launches of the level (bytes): what one more column costs a workgroup"""
    return int(max(plan["lds_front"], plan["lds_back"]))


def expected_width(plan, budget=DEFAULT_LDS_BUDGET, npatch=None):
    """The widest NV of 4, 3, 2 with NV x max(lds_front, lds_back) <= budget, else 0; 0 below PER_PATCH_MIN patches."""
    if npatch is not None and npatch < PER_PATCH_MIN:
        return 0
    for nv in (4, 3, 2):
        if nv * lds_per_column(plan) <= budget:
            return nv
    return 0


def waves_per_patch(plan):
    """waves per patch of cond_front / cond_back: by the most row pairs of X / W or of B in one patch"""
    mp = int(plan["max_pairs"])
    return 1 if mp <= 64 else 2 if mp <= 128 else 4 if mp <= 256 else 8


def repeat_patches(patch_ptr, patch_dofs, groups, npatch):
    """The patch list repeated cyclically to ``npatch`` patches: (patch_ptr int64, patch_dofs int32, groups int32 or None)"""
    patch_ptr = np.asarray(patch_ptr, dtype=np.int64)
    base = len(patch_ptr) - 1
    reps, rest = divmod(int(npatch), base)
    cut = int(patch_ptr[rest])
    sizes = np.concatenate([np.tile(np.diff(patch_ptr), reps), np.diff(patch_ptr)[:rest]])
    pp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tile = lambda a: np.concatenate([np.tile(np.asarray(a), reps), np.asarray(a)[:cut]]).astype(np.int32)
    return pp, tile(patch_dofs), None if groups is None else tile(groups)
