"""Worker of tests/test_gpu_dist_patch_storage.py: one rank of a partitioned hierarchy whose ranks ask their local levels for
single-precision patch storage (DistMultigrid(patch_factor_dtype="f32")), ranks sharing the box's single GPU.

    dist_gpu_patch_storage_worker.py OUT OVERLAP      the levels' applies, two V-cycles and a full cycle

Writes <OUT>/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out, overlap = sys.argv[1], int(sys.argv[2])
    import torch
    import torch.distributed as dist
    from alfi_amd.dist import DistMultigrid
    from tests.dist_gpu_star_condense_worker import K, hierarchy, level_input
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    lv, tr = hierarchy()
    dmg = DistMultigrid(lv, tr, K, robust_restriction=False, min_dofs=1, overlap=bool(overlap), overlap_min_dofs=0,
                        patch_factor_dtype="f32")
    if os.environ.get("ALFI_TEST_EXPECT_TRANSPORT"):
        assert dmg.transport == os.environ["ALFI_TEST_EXPECT_TRANSPORT"], dmg.transport
    smoothed = [(dl, LL) for dl, LL in zip(dmg.levels, dmg.local_levels) if LL.level > 0]
    res = {"levels": np.array([LL.level for _, LL in smoothed]),
           "dtypes": np.array([d or "" for d, LL in zip(dmg.patch_storage_dtypes(), dmg.local_levels) if LL.level > 0]),
           "noted": np.array([getattr(LL, "patch_factor_dtype", "") for _, LL in smoothed]),
           "modes": np.array([st[0] for st in dmg.patch_storage() if st is not None]),
           "bytes": np.array([st[1] for st in dmg.patch_storage() if st is not None]),
           "probes": np.array([dl.patch_check() for dl, _ in smoothed]),
           "overlap_levels": np.array(dmg.overlap_levels, dtype=np.int64)}
    for dl, LL in smoothed:
        x = level_input(lv[LL.level])
        loc = np.zeros(LL.n)
        own = LL.part.own_dofs()
        loc[:LL.n_own] = x[own]
        dx, dy = dmg.ctx.vec(loc), dmg.ctx.vec(LL.n)
        with torch.cuda.stream(dmg.stream):
            dl.patch_apply(dx, dy)
            y = dy.get()[:LL.n_own]
            dl.patch_apply(dx, dy)
            again = dy.get()[:LL.n_own]
        res["apply%d" % LL.level], res["dofs%d" % LL.level] = y, own
        res["repeat%d" % LL.level] = np.array(int(np.array_equal(y, again)))
    b = np.random.default_rng(0).standard_normal(lv[-1].n)
    b[lv[-1].bc_dofs] = 0.0
    db, dx = dmg.local_vec(b), dmg.local_vec()
    dmg.vcycle(db, dx)
    dmg.vcycle(db, dx)
    res["xv"] = dmg.owned(dx)
    dmg.fcycle(db, dx)
    res["xf"] = dmg.owned(dx)
    np.savez(os.path.join(out, "rank%d.npz" % rank), **res)
    dmg.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
