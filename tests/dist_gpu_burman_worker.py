"""Worker of tests/test_gpu_dist_burman.py: one rank of the Burman-stabilised Scott-Vogelius Newton / Reynolds-continuation
loop on partitioned levels (alfi_amd.dist.DistNavierStokesSolver), ranks sharing the box's single GPU.

    dist_gpu_burman_worker.py OUT CASE MIN_DOFS      (CASE: 2d | 3d)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT = 5e-3
RES = (10, 100)


def main():
    out, case, min_dofs = sys.argv[1], sys.argv[2], int(sys.argv[3])
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from alfi_amd import _hostlib
    from alfi_amd.dist import DistNavierStokesSolver, local_host_operator
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    prob, nref, k = ((TwoDimLidDrivenCavityProblem(4), 2, 2) if case == "2d" else (ThreeDimLidDrivenCavityProblem(1), 1, 3))
    s = DistNavierStokesSolver(prob, nref, k, min_dofs=min_dofs, discretisation="sv", stabilisation_type="burman",
                               stabilisation_weight=WEIGHT)
    # every host assembly during the Newton loops is counted (the cells' rows and the Burman host pass): the device path
    # must need none
    calls = []
    real, real_burman = _hostlib.assemble_bsr, _hostlib.burman
    _hostlib.assemble_bsr = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    _hostlib.burman = lambda *a, **kw: (calls.append(1), real_burman(*a, **kw))[1]
    res = {re: s.solve(re)[1] for re in RES}
    _hostlib.assemble_bsr, _hostlib.burman = real, real_burman
    u_all, p_all = s.u.copy(), s.p.copy()
    asm_err, inverses = -1.0, []
    if s.device_assembly:
        # the Burman refresh about the final state against the rank-local host assembly of the same rows; then the patch
        # inverses of a few owned patches (the parent compares them with the single-GPU solver's)
        asm_err = 0.0
        winds = s._winds(u_all)
        s._upload_states(u_all)
        for asm, dl, LL in zip(s._asm, s.dmg.levels, s.dmg.local_levels):
            if asm is None:
                continue
            L = s.levels[LL.level]
            with s._on_stream():
                dl.assemble_burman(s.nu, s.gamma, 1.0, asm[1], s.burman_weight, True)
                dev = dl.get_values()
            ref, _ = local_host_operator(L, LL.part, s._facet_parts[LL.level], s.nu, s.gamma, 1.0, winds[LL.level],
                                         s.burman_weight)
            asm_err = max(asm_err, float(np.abs(dev - ref.vals).max() / np.abs(ref.vals).max()))
            if LL.level == 0:
                continue
            with s._on_stream():
                dl.factor()
            npatch = len(LL.patch_ptr) - 1
            for p in sorted(set([0, npatch // 2, npatch - 1])):
                ld = LL.patch_dofs[LL.patch_ptr[p]:LL.patch_ptr[p + 1]].astype(np.int64)
                gd = LL.part.nodes[ld // L.bs] * L.bs + ld % L.bs
                with s._on_stream():
                    X = dl.patch_inverse(p, ld.size)
                inverses.append((LL.level, gd, X))
    gathered = [None] * world
    dist.all_gather_object(gathered, (len(calls), asm_err, bool(s.device_assembly), inverses))
    if rank == 0:
        inv = [x for g in gathered for x in g[3]]
        np.savez(os.path.join(out, "burman.npz"), u=u_all, p=p_all, its=[res[r]["linear_iter"] for r in RES],
                 newton=[res[r]["nonlinear_iter"] for r in RES], conv=[res[r]["converged"] for r in RES],
                 host_assemblies=[g[0] for g in gathered], asm_err=[g[1] for g in gathered],
                 device_assembly=[g[2] for g in gathered], inv_level=np.array([x[0] for x in inv], dtype=np.int64),
                 inv_ptr=np.cumsum([0] + [x[1].size for x in inv]), inv_vptr=np.cumsum([0] + [x[2].size for x in inv]),
                 inv_dofs=np.concatenate([x[1] for x in inv] + [[]]),
                 inv_vals=np.concatenate([x[2].ravel() for x in inv] + [[]]))
    s.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
