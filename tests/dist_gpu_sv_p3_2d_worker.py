"""Worker of tests/test_gpu_sv_p3_2d.py::test_partitioned_newton_on_two_ranks: one rank of the Burman-stabilised [P3]^2-P2dg
Newton / Reynolds-continuation loop on partitioned levels (alfi_amd.dist.DistNavierStokesSolver, state distributed on the
devices), ranks sharing the box's single GPU.

    dist_gpu_sv_p3_2d_worker.py OUT WEIGHT"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (10, 100)


def main():
    out, weight = sys.argv[1], float(sys.argv[2])
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from alfi_amd import _hostlib
    from alfi_amd.dist import DistNavierStokesSolver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem
    s = DistNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 3, min_dofs=1, discretisation="sv",
                               stabilisation_type="burman", stabilisation_weight=weight)
    # every host assembly during the Newton loops is counted: the device path must need none
    calls = []
    real, real_burman = _hostlib.assemble_bsr, _hostlib.burman
    _hostlib.assemble_bsr = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    _hostlib.burman = lambda *a, **kw: (calls.append(1), real_burman(*a, **kw))[1]
    # what crosses PCIe per Newton step of the SECOND solve (alfi_transfer_stats: every copy the library makes)
    res = {RES[0]: s.solve(RES[0])[1]}
    s.ctx.transfer_stats(reset=True)
    res[RES[1]] = s.solve(RES[1])[1]
    h2d, d2h = s.ctx.transfer_stats()
    per_step = max(h2d, d2h) / max(res[RES[1]]["nonlinear_iter"], 1)
    _hostlib.assemble_bsr, _hostlib.burman = real, real_burman
    resident = bool(s._device_state_resident())
    partitioned = s.dmg.local_levels[-1].part.nb_own > 0 and s.dmg.local_levels[-1].part.nb_own < s.levels[-1].V.num_nodes
    u_all, p_all = s.u.copy(), s.p.copy()            # COLLECTIVE: every rank contributes its owned entries
    gathered = [None] * world
    dist.all_gather_object(gathered, (len(calls), bool(s.device_assembly), per_step, resident, bool(partitioned)))
    if rank == 0:
        np.savez(os.path.join(out, "sv_p3_2d.npz"), u=u_all, p=p_all, its=[res[r]["linear_iter"] for r in RES],
                 newton=[res[r]["nonlinear_iter"] for r in RES], conv=[res[r]["converged"] for r in RES],
                 host_assemblies=[g[0] for g in gathered], device_assembly=[g[1] for g in gathered],
                 bytes_per_step=[g[2] for g in gathered], resident=[g[3] for g in gathered],
                 partitioned=[g[4] for g in gathered])
    s.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
