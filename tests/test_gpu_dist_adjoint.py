"""Adjoint solves on partitioned levels (-m gpu): DistNavierStokesSolver.solve_adjoint -- every rank refreshes its own rows of
the transposed operators on the device (alfi_level_set_assembly_transposed), no exchange beyond the forward refresh's --
against the single-GPU HipNavierStokesSolver with the same arguments at the ranks' state.  Ranks share the box's one GPU
(worker: tests/dist_gpu_adjoint_worker.py; gloo callback transport or tests/mock_rccl)."""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dist_gpu_adjoint_worker as W      # (the cases' solvers and functionals, shared with the ranks)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _start_ranks(out, mode, case, world, transport="callback", min_dofs=1, device_state=True, env_extra=None):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="4")
        if transport == "rccl":
            from tests.mock_rccl.build import build
            env.update(ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=build())
        env.update(env_extra or {})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_adjoint_worker.py"), str(out), mode,
                                       case, str(min_dofs), "1" if device_state else "0"], env=env, cwd=ROOT))
    return procs


def _finish_ranks(procs, out, mode):
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    with open(os.path.join(str(out), mode + ".pkl"), "rb") as f:
        return pickle.load(f)


def _run_ranks(out, mode, case, world, **kw):
    return _finish_ranks(_start_ranks(out, mode, case, world, **kw), out, mode)


@pytest.fixture(scope="module")
def reference():
    """The single-GPU solver of a case after the continuation Re 10 -> 50, made once."""
    from alfi_amd.nssolver import HipNavierStokesSolver
    made = {}

    def get(case):
        if case not in made:
            s = W.make_solver(HipNavierStokesSolver, case)
            for re in (10.0, 50.0):
                assert s.solve(re)[1]["converged"]
            made[case] = s
        return made[case]
    yield get
    for s in made.values():
        s.close()


def _check_solve(z, s, case, world):
    import scipy.sparse as sp
    from alfi_amd.adjoint import adjoint_rhs
    from alfi_amd.problem import BSR
    assert all(g["device_assembly"] for g in z["ranks"]) and len(z["ranks"]) == world
    assert all(i["converged"] for i in z["forward"])
    # the transposed refresh of every rank's levels: bitwise the transposes of the mirror blocks, on ghost rows too
    levels = [x for g in z["ranks"] for x in g["levels"]]
    assert len(levels) >= world and all(ok for _, ok, _, _, _ in levels), levels
    assert not any(same for _, _, same, _, _ in levels)
    assert any(nghost > 0 for _, _, _, _, nghost in levels)
    patches = [x for g in z["ranks"] for x in g["patches"]]
    if case in ("pkp0", "sv-burman"):
        assert len(patches) >= 3
    assert all(err <= 1e-10 for _, _, err in patches), patches
    # the adjoint: the single-GPU solver moved to the ranks' gathered state; its own adjoint solve there, then its forward
    # Jacobian K
    info = z["info"]
    assert info["converged"] and info["linear_iter"] > 0 and z["same_object"]
    s.u, s.p = z["u"].copy(), z["p"].copy()
    J = W.functional(s)
    _, ref = s.solve_adjoint(J, rtol=1e-10, atol=0.0)
    assert set(info) == set(ref) and info["transpose_s"] == 0.0
    assert isinstance(info["linear_iter"], int) and isinstance(info["converged"], bool)
    assert abs(info["linear_iter"] - ref["linear_iter"]) <= 2, (info["linear_iter"], ref["linear_iter"])
    L = s.levels[-1]
    s._refresh_device(None, 1.0)
    A = BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx, s.hmg.mg.levels[-1].get_values()).to_scipy()
    K = sp.bmat([[A, s.B.T], [s.B, None]]).tocsr()
    lam = np.concatenate([z["lam_u"], z["lam_p"]])
    g = adjoint_rhs(*J.gradient(s, s.u, s.p), L.bc_dofs, s.n_p, s.vol if s.nullspace else None)
    r = K.T @ lam - g
    rr, gn = np.linalg.norm(r), np.linalg.norm(g)
    print("[dist adjoint] %s on %d ranks: |K^T lam - g| / |g| = %.3e, reported %.3e, Krylov %d (single GPU %d)"
          % (case, world, rr / gn, info["residual_norm"] / gn, info["linear_iter"], ref["linear_iter"]))
    assert rr <= 1e-5 * gn, (case, rr / gn)
    assert abs(rr - info["residual_norm"]) <= 1e-2 * rr + 1e-14 * gn, (case, rr, info["residual_norm"])
    assert abs(info["rhs_norm"] - gn) <= 1e-12 * gn
    assert np.all(z["lam_u"][L.bc_dofs] == 0.0)
    assert abs(s.vol @ z["lam_p"]) <= 1e-12 * np.abs(z["lam_p"]).max() * s.area


@pytest.mark.parametrize("case,world,transport", [("pkp0", 2, "callback"), ("supg", 3, "rccl"), ("sv-burman", 2, "callback"),
                                                  ("3d-k1", 2, "callback")])
def test_partitioned_adjoint(tmp_path, reference, case, world, transport):
    """[P2]^2-P0 and the Burman-stabilised Scott-Vogelius pair on 2 ranks, SUPG on 3 over tests/mock_rccl, 3-D k = 1 on 2;
    every level partitioned, the state distributed on the devices."""
    z = _run_ranks(tmp_path, "solve", case, world, transport=transport)
    assert all(g["resident"] for g in z["ranks"])
    _check_solve(z, reference(case), case, world)


def test_partitioned_adjoint_single_owner_coarse_levels(tmp_path, reference):
    """min_dofs = the finest level's size: the coarse levels live on one rank alone, the finest is partitioned."""
    s = reference("pkp0")
    _check_solve(_run_ranks(tmp_path, "solve", "pkp0", 2, min_dofs=s.levels[-1].n), s, "pkp0", 2)


def test_partitioned_adjoint_replicated_host_state(tmp_path, reference):
    """device_state=False: the states of the transposed refresh are uploaded from the replicated host state."""
    z = _run_ranks(tmp_path, "solve", "pkp0", 2, device_state=False)
    assert not any(g["resident"] for g in z["ranks"])
    _check_solve(z, reference("pkp0"), "pkp0", 2)


def test_partitioned_adjoint_of_a_list(tmp_path):
    """solve_adjoint([J1, J2, J3]) on 2 ranks: every z_adj[i] bitwise that of solve_adjoint(Ji) on the same ranks, after ONE
    refresh and ONE factorisation."""
    z = _run_ranks(tmp_path, "list", "pkp0", 2)
    assert z["is_list"] and len(z["block"]) == 3 and z["counts"] == {"refresh": 1, "factor": 1}, z["counts"]
    info = z["info"]
    for i, ((lu, lp, inf), (bu, bp)) in enumerate(zip(z["single"], z["block"])):
        assert inf["converged"] and inf["linear_iter"] > 0 and np.abs(lu).max() > 0.0
        assert np.array_equal(lu, bu) and np.array_equal(lp, bp), i
        assert info["linear_iter"][i] == inf["linear_iter"] and info["residual_norm"][i] == inf["residual_norm"]
        assert info["rhs_norm"][i] == inf["rhs_norm"] and info["converged"][i] is True
    assert isinstance(info["refresh_s"], float) and isinstance(info["factor_s"], float)


def test_partitioned_adjoint_leaves_no_trace(tmp_path):
    """Continuation 10 -> 100 with an adjoint solve after every step: the states bit for bit and the Newton / Krylov counts of
    the same ranks without the adjoint solves (the two runs side by side on the GPU)."""
    outs = {m: tmp_path / m for m in ("plain", "trace")}
    for d in outs.values():
        d.mkdir()
    procs = {m: _start_ranks(outs[m], m, "pkp0", 2) for m in outs}
    try:
        runs = {m: _finish_ranks(procs[m], outs[m], m) for m in outs}
    finally:
        for ps in procs.values():
            for p in ps:
                if p.poll() is None:
                    p.kill()
                    p.wait(timeout=30)
    assert runs["trace"]["adjoint_converged"] == [True, True]
    for a, b in zip(runs["plain"]["steps"], runs["trace"]["steps"]):
        assert a[4] and b[4]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2:] == b[2:]


def test_partitioned_adjoint_refused_on_host_assembly(tmp_path):
    """ALFI_DEVICE_ASSEMBLY=0: setup_adjoint raises NotImplementedError ("partitioned") on every rank, before any
    collective; the workers exit cleanly."""
    z = _run_ranks(tmp_path, "refuse", "pkp0", 2, env_extra={"ALFI_DEVICE_ASSEMBLY": "0"})
    assert len(z["ranks"]) == 2
    for g in z["ranks"]:
        assert not g["device_assembly"] and "partitioned" in g["refused"], g
