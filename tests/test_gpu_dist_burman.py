"""Burman-stabilised Scott-Vogelius Newton on partitioned levels (-m gpu): DistNavierStokesSolver(discretisation="sv",
stabilisation_type="burman") against the single-GPU HipNavierStokesSolver with the same arguments, ranks sharing the box's one
GPU (worker: tests/dist_gpu_burman_worker.py).  Same Newton counts, Krylov counts within 2, the same solution; on the device
path no host assembly during the Newton loops, the rank's refreshed rows equal to its host assembly (Burman term included) and
its owned patches' inverses equal to the single-GPU ones."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT = 5e-3
RES = (10, 100)


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


@pytest.fixture(scope="module")
def reference():
    """The single-GPU solvers, one per problem, run once (Re 10 -> 100) and kept for the patch-inverse comparisons."""
    from alfi_amd.nssolver import HipNavierStokesSolver, run_solver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    made = {}

    def get(case):
        if case not in made:
            prob, nref, k = ((TwoDimLidDrivenCavityProblem(4), 2, 2) if case == "2d" else (ThreeDimLidDrivenCavityProblem(1), 1, 3))
            s = HipNavierStokesSolver(prob, nref, k, discretisation="sv", stabilisation_type="burman", stabilisation_weight=WEIGHT)
            made[case] = (s, run_solver(s, list(RES)))
        return made[case]
    yield get
    for s, _ in made.values():
        s.close()


def _run_ranks(tmp_path, case, world, transport="callback", min_dofs=1, env_extra=None):
    port = _free_port()
    procs = []
    try:
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="4")
            if transport == "rccl":
                from tests.mock_rccl.build import build
                env.update(ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=build())
            env.update(env_extra or {})
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_burman_worker.py"),
                                           str(tmp_path), case, str(min_dofs)], env=env, cwd=ROOT))
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return np.load(os.path.join(str(tmp_path), "burman.npz"))


def _compare_counts_and_state(z, s, res):
    assert all(z["conv"]) and all(res[r]["converged"] for r in RES)
    assert list(z["newton"]) == [res[r]["nonlinear_iter"] for r in RES], (list(z["newton"]), res)
    assert all(abs(int(a) - res[r]["linear_iter"]) <= 2 for a, r in zip(z["its"], RES)), (list(z["its"]), res)
    assert np.abs(z["u"] - s.u).max() < 1e-7 * np.abs(s.u).max()
    assert np.abs(z["p"] - s.p).max() < 1e-6 * np.abs(s.p).max()


def _compare_patch_inverses(z, s):
    """The ranks' inverses of their owned patches (refresh about their final state, adv = 1) against the single-GPU solver's
    inverses of the same patches about the same state."""
    assert len(z["inv_level"]) > 0
    s._device_states(np.asarray(z["u"]))
    mgl = s.hmg.mg.levels
    index = {}
    for lev in sorted(set(int(x) for x in z["inv_level"])):
        dl, st, obj = mgl[lev], s._dstate[lev], s.hmg.pc_objs[lev]
        dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
        dl.factor()
        ptr = obj.patch_ptr
        index[lev] = {tuple(np.sort(obj.patch_dofs[ptr[p]:ptr[p + 1]])): p for p in range(len(ptr) - 1)}
    worst = 0.0
    for i, lev in enumerate(z["inv_level"]):
        lev = int(lev)
        gd = z["inv_dofs"][z["inv_ptr"][i]:z["inv_ptr"][i + 1]].astype(np.int64)
        n = gd.size
        X = z["inv_vals"][z["inv_vptr"][i]:z["inv_vptr"][i + 1]].reshape(n, n)
        obj = s.hmg.pc_objs[lev]
        p = index[lev][tuple(np.sort(gd))]
        od = obj.patch_dofs[obj.patch_ptr[p]:obj.patch_ptr[p + 1]].astype(np.int64)
        perm = np.argsort(gd)[np.searchsorted(np.sort(gd), od)]          # gd[perm] == od
        assert np.array_equal(gd[perm], od)
        ref = s.hmg.mg.levels[lev].patch_inverse(p, n)
        worst = max(worst, float(np.abs(X[perm][:, perm] - ref).max() / np.abs(ref).max()))
    assert worst <= 1e-10, worst


@pytest.mark.parametrize("case,world,transport", [("2d", 2, "callback"), ("2d", 3, "rccl"), ("3d", 2, "callback")])
def test_partitioned_burman_newton(tmp_path, reference, case, world, transport):
    """[P2]^2 on 2 ranks (gloo callback) and on 3 over tests/mock_rccl, [P3]^3 on 2 ranks; every level partitioned."""
    s, res = reference(case)
    z = _run_ranks(tmp_path, case, world, transport)
    assert all(z["device_assembly"]) and list(z["host_assemblies"]) == [0] * world, (z["device_assembly"], z["host_assemblies"])
    assert max(z["asm_err"]) < 1e-12, z["asm_err"]
    _compare_counts_and_state(z, s, res)
    _compare_patch_inverses(z, s)


def test_partitioned_burman_newton_single_owner_coarse_levels(tmp_path, reference):
    """min_dofs = the finest level's size: the coarse levels live on rank 0 alone (their facets, patches and the facet rule
    those of the single-GPU path), the finest is partitioned."""
    s, res = reference("2d")
    z = _run_ranks(tmp_path, "2d", 2, min_dofs=s.levels[-1].n)
    assert all(z["device_assembly"]) and list(z["host_assemblies"]) == [0, 0]
    assert max(z["asm_err"]) < 1e-12, z["asm_err"]
    _compare_counts_and_state(z, s, res)
    _compare_patch_inverses(z, s)


def test_partitioned_burman_newton_host_assembly(tmp_path, reference):
    """ALFI_DEVICE_ASSEMBLY=0: every rank assembles its rows and its facets' Burman terms on the host; same counts."""
    s, res = reference("2d")
    z = _run_ranks(tmp_path, "2d", 2, env_extra={"ALFI_DEVICE_ASSEMBLY": "0"})
    assert not any(z["device_assembly"])
    _compare_counts_and_state(z, s, res)
