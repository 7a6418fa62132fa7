"""Worker of tests/test_gpu_one_driver.py: one rank of a partitioned hierarchy (ranks share the box's GPU, native transport over
tests/mock_rccl).  One smoother call on the finest level (zero initial guess) and one V-cycle; writes the rank's exchange and
all-reduce counts of each (alfi_ctx_comm_stats) to <out>/rank<r>.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    case, out = sys.argv[1], sys.argv[2]
    import torch
    import torch.distributed as dist
    from tests.test_dist_cpu import _hier
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from alfi_amd.dist import DistMultigrid
    lv, tr, k, min_dofs = _hier(case)
    dmg = DistMultigrid(lv, tr, k, robust_restriction=False, min_dofs=min_dofs)
    assert dmg.transport == "rccl", dmg.transport
    b = np.random.default_rng(0).standard_normal(lv[-1].n)
    b[lv[-1].bc_dofs] = 0.0
    db, dx = dmg.local_vec(b), dmg.local_vec()
    ctx = dmg.ctx
    ctx.comm_stats(reset=True)
    with torch.cuda.stream(dmg.stream):
        dmg._in_cycle = True
        dmg.levels[-1].smooth(k, db, dx, nonzero_guess=False)
        dmg._in_cycle = False
    ctx.sync()
    smooth = ctx.comm_stats(reset=True)
    dmg.vcycle(db, dx)
    ctx.sync()
    vcycle = ctx.comm_stats(reset=True)
    res = {"k": k, "levels": len(dmg.levels), "overlap_levels": list(dmg.overlap_levels), "smooth": list(smooth[:2]),
           "vcycle": list(vcycle[:2]), "finite": bool(np.isfinite(dmg.owned(dx)).all())}
    with open(os.path.join(out, "rank%d.json" % rank), "w") as f:
        json.dump(res, f)
    dmg.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
