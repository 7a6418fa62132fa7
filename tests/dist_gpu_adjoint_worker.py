"""Worker of tests/test_gpu_dist_adjoint.py: one rank of an adjoint solve on partitioned levels
(alfi_amd.dist.DistNavierStokesSolver.solve_adjoint: the transposed operator refresh, alfi_level_set_assembly_transposed),
ranks sharing the box's single GPU.

    dist_gpu_adjoint_worker.py OUT MODE CASE MIN_DOFS DEVICE_STATE
        MODE: solve | list | trace | plain | refuse      CASE: pkp0 | supg | sv-burman | 3d-k1

Rank 0 writes OUT/MODE.pkl."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _force(x):
    d = x.shape[1]
    f = np.zeros_like(x)
    for i in range(d):
        f[:, i] = np.sin(np.pi * x[:, (i + 1) % d]) + 0.5 * x[:, i] * x[:, (i + 2) % d]
    return f


def _weight(x):
    w = np.zeros_like(x)
    w[:, 0] = np.cos(0.5 * np.pi * x[:, 1])
    w[:, 1] = 1.0 + x[:, 0] * x[:, 1]
    return w


def make_solver(cls, case, **kw):
    """The solver of a case, single-GPU (the parent's reference) or partitioned, from the same arguments."""
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    if case == "pkp0":
        return cls(TwoDimLidDrivenCavityProblem(4), 2, 2, **kw)
    if case == "supg":
        return cls(TwoDimLidDrivenCavityProblem(4), 1, 2, stabilisation_type="supg", **kw)
    if case == "sv-burman":
        return cls(TwoDimLidDrivenCavityProblem(4), 2, 2, discretisation="sv", stabilisation_type="burman",
                   stabilisation_weight=5e-3, **kw)
    assert case == "3d-k1"
    return cls(ThreeDimLidDrivenCavityProblem(2), 1, 1, **kw)


def functional(s, seed=3):
    """A load part and a random pressure part, as tests/test_gpu_adjoint.py::test_adjoint_residual takes."""
    from alfi_amd.adjoint import LinearFunctional, LoadFunctional
    g_u = LoadFunctional(_weight if s.problem.dim == 2 else _force).gradient(s, None, None)[0]
    return LinearFunctional(g_u, np.random.default_rng(seed).standard_normal(s.n_p) + 0.2)


def functionals(s):
    from alfi_amd.adjoint import LinearFunctional, LoadFunctional
    g_p = np.random.default_rng(5).standard_normal(s.n_p) + 0.2
    return [LoadFunctional(_weight), LinearFunctional(LoadFunctional(_force).gradient(s, None, None)[0], g_p), LoadFunctional(_force)]


def _mirror(rowptr, colidx):
    """Index of block (j, i) for every block (i, j) of the rank's local sparsity, whose columns are not sorted."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key, mkey = rows * n + colidx, np.asarray(colidx, dtype=np.int64) * n + rows
    order = np.argsort(key)
    pos = np.searchsorted(key[order], mkey)
    assert np.array_equal(key[order][pos], mkey)
    return order[pos]


def _operator_and_patch_checks(s, u_all, with_patches):
    """Per level with owned rows: forward refresh about the final state -> vf, the switch on -> vt, vt == transpose(vf[mirror])
    bitwise; a few owned patches' inverses under the transposed refresh against the transposes of the forward ones."""
    levels, patches = [], []
    s._upload_states(u_all)
    for asm, dl, LL in zip(s._asm, s.dmg.levels, s.dmg.local_levels):
        if asm is None:
            continue
        with s._on_stream():
            s._assemble_level(dl, asm[1], None, 1.0)
            vf = dl.get_values()
            inv = []
            npatch = len(LL.patch_ptr) - 1
            ps = sorted(set([0, npatch // 3, npatch // 2, npatch - 1])) if with_patches and LL.level > 0 and npatch > 0 else []
            if ps and dl.condensed() == 0:
                dl.factor()
                inv = [dl.patch_inverse(p, int(LL.patch_ptr[p + 1] - LL.patch_ptr[p])) for p in ps]
            dl.set_assembly_transposed(True)
            try:
                s._assemble_level(dl, asm[1], None, 1.0)
            finally:
                dl.set_assembly_transposed(False)
            vt = dl.get_values()
            mirror = _mirror(np.asarray(LL.A.rowptr, dtype=np.int64), np.asarray(LL.A.colidx, dtype=np.int64))
            want = np.transpose(vf[mirror], (0, 2, 1))
            levels.append((LL.level, bool(np.array_equal(vt, want)), bool(np.array_equal(vt, vf)), int(dl.nnzb),
                           int(LL.part.nb_loc - LL.part.nb_own)))
            if inv:
                dl.factor()
                for p, X in zip(ps, inv):
                    Y = dl.patch_inverse(p, X.shape[0])
                    patches.append((LL.level, int(p), float(np.abs(Y - X.T).max() / np.abs(X).max())))
    return levels, patches


def _counted(s):
    """Calls of the refresh and of the factorisation, counted."""
    n = {"refresh": 0, "factor": 0}
    refresh, factor = s._refresh_device, s._factor_levels

    def r(*a, **k):
        n["refresh"] += 1
        return refresh(*a, **k)

    def f(*a, **k):
        n["factor"] += 1
        return factor(*a, **k)
    s._refresh_device, s._factor_levels = r, f
    return n


def main():
    out, mode, case, min_dofs, device_state = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5] == "1"
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from alfi_amd.dist import DistNavierStokesSolver
    s = make_solver(DistNavierStokesSolver, case, min_dofs=min_dofs, device_state=device_state)
    res = {"device_assembly": bool(s.device_assembly), "resident": bool(s._device_state_resident())}
    if mode == "refuse":
        try:
            s.setup_adjoint(functional(s))
            res["refused"] = "no"
        except NotImplementedError as e:
            res["refused"] = str(e)
    elif mode == "solve":
        res["forward"] = [s.solve(re)[1] for re in (10.0, 50.0)]
        J = functional(s)
        z, info = s.solve_adjoint(J, rtol=1e-10, atol=0.0)
        u_all, p_all = s.u.copy(), s.p.copy()
        res.update(u=u_all, p=p_all, lam_u=z[0], lam_p=z[1], info=info, same_object=z is s.z_adj)
        res["levels"], res["patches"] = _operator_and_patch_checks(s, u_all, case in ("pkp0", "sv-burman"))
    elif mode == "list":
        for re in (10.0, 50.0):
            s.solve(re)
        Js = functionals(s)
        single = []
        for J in Js:
            z, info = s.solve_adjoint(J, rtol=1e-10, atol=0.0)
            single.append((z[0].copy(), z[1].copy(), info))
        n = _counted(s)
        z, info = s.solve_adjoint(Js, rtol=1e-10, atol=0.0)
        res.update(single=single, block=[(a.copy(), b.copy()) for a, b in z], info=info, counts=n, is_list=isinstance(z, list))
    else:                                   # trace / plain: the continuation with / without an adjoint solve after every step
        from alfi_amd.adjoint import LoadFunctional
        steps = []
        for re in (10.0, 100.0):
            _, info = s.solve(re)
            steps.append((s.u.copy(), s.p.copy(), info["linear_iter"], info["nonlinear_iter"], bool(info["converged"])))
            if mode == "trace":
                _, ainfo = s.solve_adjoint(LoadFunctional(_weight))
                res.setdefault("adjoint_converged", []).append(bool(ainfo["converged"]))
        res["steps"] = steps
    gathered = [None] * world
    dist.all_gather_object(gathered, {k: res[k] for k in ("device_assembly", "resident", "refused", "levels", "patches") if k in res})
    if rank == 0:
        res["ranks"] = gathered
        with open(os.path.join(out, mode + ".pkl"), "wb") as f:
            pickle.dump(res, f)
    s.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
