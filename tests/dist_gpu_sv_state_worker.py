"""Worker of tests/test_gpu_dist_sv_state.py: one rank of the Scott-Vogelius Newton / Reynolds-continuation loop on partitioned
levels (alfi_amd.dist.DistNavierStokesSolver) with the Newton state distributed on the devices, ranks sharing the box's single
GPU.

    dist_gpu_sv_state_worker.py OUT CASE MIN_DOFS BURMAN DEVICE_STATE      (CASE: 2d | 3d; BURMAN: weight or 0)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = (10, 100)


def main():
    out, case, min_dofs, burman, device_state = sys.argv[1], sys.argv[2], int(sys.argv[3]), float(sys.argv[4]), sys.argv[5] == "1"
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from alfi_amd import _hostlib
    from alfi_amd.dist import DistNavierStokesSolver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    prob, nref, k = ((TwoDimLidDrivenCavityProblem(4), 2, 2) if case == "2d" else (ThreeDimLidDrivenCavityProblem(1), 1, 3))
    kw = dict(stabilisation_type="burman", stabilisation_weight=burman) if burman else {}
    s = DistNavierStokesSolver(prob, nref, k, min_dofs=min_dofs, discretisation="sv", device_state=device_state, **kw)
    # every host assembly during the Newton loops is counted (the cells' rows and the Burman host pass): the device path
    # must need none
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
    u_all, p_all = s.u.copy(), s.p.copy()            # COLLECTIVE: every rank contributes its owned entries
    # the level states the loop left on the device (the last residual evaluation filled them from the final velocity) against
    # the level-by-level injection of the gathered velocity on the host
    state_err, levels_checked = -1.0, 0
    if resident:
        state_err = 0.0
        for asm, w in zip(s._asm, s._winds(u_all)[s.dmg.lmin:]):
            if asm is None:
                continue
            with s._on_stream():
                got = asm[1].get()
            state_err = max(state_err, float(np.abs(got.reshape(-1, prob.dim) - w[asm[0]]).max()))
            levels_checked += 1
    gathered = [None] * world
    dist.all_gather_object(gathered, (len(calls), state_err, bool(s.device_assembly), per_step, resident, levels_checked))
    if rank == 0:
        np.savez(os.path.join(out, "sv_state.npz"), u=u_all, p=p_all, its=[res[r]["linear_iter"] for r in RES],
                 newton=[res[r]["nonlinear_iter"] for r in RES], conv=[res[r]["converged"] for r in RES],
                 host_assemblies=[g[0] for g in gathered], state_err=[g[1] for g in gathered],
                 device_assembly=[g[2] for g in gathered], bytes_per_step=[g[3] for g in gathered],
                 resident=[g[4] for g in gathered], levels_checked=[g[5] for g in gathered])
    s.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
