"""Worker of tests/test_gpu_dist_star_condense.py: one rank of a partitioned hierarchy whose levels condense their vertex-star
factors themselves (DistMultigrid / DistNavierStokesSolver with condense_min_bytes), ranks sharing the box's single GPU.

    dist_gpu_star_condense_worker.py OUT cycles CMB OVERLAP     two V-cycles, a full cycle (both restrictions), the levels' applies
    dist_gpu_star_condense_worker.py OUT mult                   set_multiplicative on levels that condensed themselves
    dist_gpu_star_condense_worker.py OUT newton                 Newton + continuation, [P2+FB]^3-P0, operators formed on the device
    dist_gpu_star_condense_worker.py OUT burman                 Burman-stabilised Scott-Vogelius pair

CMB: the keyword's value, "none" = left out.  Every mode writes <OUT>/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 4
RES = (10, 100)


def hierarchy():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)


def level_input(L):
    """the vector the patch apply of global level L is tested on (Dirichlet entries non-zero on purpose)"""
    return np.random.default_rng(10 + L.level).standard_normal(L.n)


def dense_bytes(patch_ptr):
    n = np.diff(np.asarray(patch_ptr, dtype=np.int64))
    # alfi_patches_factor_bytes of a dense level: even leading dimensions, every inverse padded to 16 doubles (patch_plan.h)
    return int(8 * ((n * ((n + 1) & ~1) + 15) & ~15).sum())


def storage_report(dmg):
    """Per smoothed local level: level, mode, factor bytes, dense bytes, whether the rank owns a patch the finder groups, what the
    device level recorded on the local level (hip.note_patch_level) and what hip.condense_patches says."""
    import torch
    from alfi_amd import hip
    rows = []
    with torch.cuda.stream(dmg.stream):
        for st, dl, LL in zip(dmg.patch_storage(), dmg.levels, dmg.local_levels):
            if st is None:
                continue
            grouped = bool((dl.find_patch_groups() >= 0).any())
            rows.append((LL.level, st[0], st[1], dense_bytes(LL.patch_ptr), int(grouped), int(getattr(LL, "patch_storage", -1)),
                         int(getattr(LL, "patch_factor_bytes", -1)), int(hip.condense_patches(LL))))
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def probes(dmg):
    """(worst residual, flagged, repaired, worst afterwards) of the last factorisation of every smoothed local level"""
    return np.array([dl.patch_check() for dl, LL in zip(dmg.levels, dmg.local_levels) if LL.level > 0 and len(LL.patch_ptr) > 1])


def run_cycles(out, rank, cmb, overlap):
    import torch
    from alfi_amd.dist import DistMultigrid
    lv, tr = hierarchy()
    kw = {} if cmb == "none" else {"condense_min_bytes": int(cmb)}
    dmg = DistMultigrid(lv, tr, K, robust_restriction=False, min_dofs=1, overlap=bool(int(overlap)), overlap_min_dofs=0, **kw)
    if os.environ.get("ALFI_TEST_EXPECT_TRANSPORT"):
        assert dmg.transport == os.environ["ALFI_TEST_EXPECT_TRANSPORT"], dmg.transport
    res = {"storage": storage_report(dmg), "probes": probes(dmg), "overlap_levels": np.array(dmg.overlap_levels, dtype=np.int64),
           "distributed": np.array([int(p.distributed) for p in dmg.parts])}
    # the patch apply of every smoothed level (collective: forward halo, the rank's patches, reverse add)
    for dl, LL in zip(dmg.levels, dmg.local_levels):
        if LL.level == 0:
            continue
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
    db = dmg.local_vec(b)
    base = dmg.mg
    for robust in (0, 1):
        # (the other restriction: a second cycle handle over the same device levels and transfers)
        dmg.mg = base if robust == 0 else base.variant(True)
        dx = dmg.local_vec()
        dmg.vcycle(db, dx)
        dmg.vcycle(db, dx)
        res["xv%d" % robust] = dmg.owned(dx)
        dmg.fcycle(db, dx)
        res["xf%d" % robust] = dmg.owned(dx)
        if robust:
            dmg.sync()
            dmg.mg.close_handle()
    dmg.mg = base
    res["storage_after"] = storage_report(dmg)
    np.savez(os.path.join(out, "rank%d.npz" % rank), **res)
    dmg.close()


def run_mult(out, rank):
    """tests/dist_gpu_mult_worker.py on levels that condensed themselves first: the case and the comparison of
    test_partitioned_multiplicative (3d-P2FB = levels 0 and 1 of the hierarchy above; the SPMD oracle on the same rank-local data)"""
    import torch
    from alfi_amd.dist import DistMultigrid
    from oracle.dist_oracle import DistOracle
    from tests.test_dist_cpu import _hier
    lv, tr, k, min_dofs = _hier("3d-P2FB")
    dmg = DistMultigrid(lv, tr, k, robust_restriction=False, min_dofs=min_dofs, condense_min_bytes=0)
    before = storage_report(dmg)
    orders = []
    for LL, dl in zip(dmg.local_levels, dmg.levels):
        npatch = len(LL.patch_ptr) - 1
        if LL.level > 0 and npatch > 0:
            order = np.arange(npatch)[::-1].copy()
            with torch.cuda.stream(dmg.stream):
                assert dl.set_multiplicative(order, True) >= 1
            orders.append(order)
        else:
            orders.append(None if LL.level == 0 or npatch == 0 else np.zeros(0, dtype=np.int64))
    after = storage_report(dmg)
    omg = DistOracle(dmg.local_levels, dmg.local_transfers, dmg.lmin, k, dmg.comm, robust=False, mult_orders=orders, symmetrise=True)
    b = np.random.default_rng(0).standard_normal(lv[-1].n)
    b[lv[-1].bc_dofs] = 0.0
    F = dmg.fine
    bl = np.zeros(F.n)
    bl[:F.n_own] = b[F.part.own_dofs()]
    top = len(dmg.local_levels) - 1
    db, dx = dmg.local_vec(b), dmg.local_vec()
    with torch.cuda.stream(dmg.stream):
        dmg.levels[-1].patch_apply(db, dx)
    ref = omg.patch_apply(top, bl.copy())
    e1 = np.abs(dmg.owned(dx) - ref[:F.n_own]).max() / np.abs(ref[:F.n_own]).max()
    dx = dmg.local_vec()
    dmg.vcycle(db, dx)
    refv = omg.vcycle(top, bl.copy(), np.zeros(F.n))
    e2 = np.abs(dmg.owned(dx) - refv[:F.n_own]).max() / np.abs(refv[:F.n_own]).max()
    with torch.cuda.stream(dmg.stream):
        dmg.levels[-1].factor()                              # stays dense at the next factorisation
    np.savez(os.path.join(out, "rank%d.npz" % rank), before=before, after=after, refactored=storage_report(dmg), e1=e1, e2=e2)
    dmg.close()


def run_newton(out, rank, world):
    """The pkp0-3d run of tests/dist_gpu_newton_worker.py with the threshold at 0: the operators are formed on the device, so the
    levels decide at the solver's first refresh; the storage and the probe are read after every refresh."""
    import torch.distributed as dist
    from alfi_amd.dist import DistNavierStokesSolver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem
    s = DistNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 2, min_dofs=1, condense_min_bytes=0)
    seen = []
    refactor = s.dmg.refactor

    def noted(*a, **kw):
        refactor(*a, **kw)
        seen.append((storage_report(s.dmg), probes(s.dmg)))
    s.dmg.refactor = noted
    res = {re: s.solve(re)[1] for re in RES}
    s.dmg.refactor = refactor
    u_all, p_all = s.u, s.p                                  # COLLECTIVE
    gathered = [None] * world
    dist.all_gather_object(gathered, (bool(s.device_assembly), seen))
    if rank == 0:
        np.savez(os.path.join(out, "rank0.npz"), u=u_all, p=p_all, its=[res[r]["linear_iter"] for r in RES],
                 newton=[res[r]["nonlinear_iter"] for r in RES], conv=[res[r]["converged"] for r in RES],
                 device_assembly=[g[0] for g in gathered], refreshes=[len(g[1]) for g in gathered],
                 storage=np.concatenate([st for g in gathered for st, _ in g[1]]),
                 probes=np.concatenate([pr for g in gathered for _, pr in g[1]]))
    s.close()


def run_burman(out, rank):
    from alfi_amd.dist import DistNavierStokesSolver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem
    s = DistNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 2, 2, min_dofs=1, discretisation="sv", stabilisation_type="burman",
                               stabilisation_weight=5e-3, condense_min_bytes=0)
    before = storage_report(s.dmg)
    info = s.solve(10)[1]
    np.savez(os.path.join(out, "rank%d.npz" % rank), before=before, after=storage_report(s.dmg), conv=info["converged"])
    s.close()


def main():
    out, mode = sys.argv[1], sys.argv[2]
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    if mode == "cycles":
        run_cycles(out, rank, sys.argv[3], sys.argv[4])
    elif mode == "mult":
        run_mult(out, rank)
    elif mode == "newton":
        run_newton(out, rank, world)
    elif mode == "burman":
        run_burman(out, rank)
    else:
        raise ValueError(mode)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
