"""The Scott-Vogelius Newton state distributed on the devices (-m gpu): DistNavierStokesSolver(discretisation="sv"), with and
without Burman terms, against the single-GPU HipNavierStokesSolver with the same arguments, ranks sharing the box's one GPU
(worker: tests/dist_gpu_sv_state_worker.py).  On the barycentric hierarchy a level's refresh state is a weighted gather of the
exchanged finest velocity (StateExchange + alfi_vec_gather_csr): the loop must be the resident one, move less than 1 KB per
Newton step and rank across PCIe (the bound and the measurement tests/test_gpu_dist.py::test_partitioned_newton applies to the
P0-pressure pairs), assemble nothing on the host, leave on every level the state the level-by-level injection gives, and
reproduce the single-GPU solver's counts and solution to test_partitioned_newton's tolerances.  ``device_state=False`` keeps
the replicated loop."""
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
    """The single-GPU solvers, one per (problem, Burman weight), run once (Re 10 -> 100)."""
    from alfi_amd.nssolver import HipNavierStokesSolver, run_solver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    made = {}

    def get(case, burman=0.0):
        if (case, burman) not in made:
            prob, nref, k = ((TwoDimLidDrivenCavityProblem(4), 2, 2) if case == "2d" else (ThreeDimLidDrivenCavityProblem(1), 1, 3))
            kw = dict(stabilisation_type="burman", stabilisation_weight=burman) if burman else {}
            s = HipNavierStokesSolver(prob, nref, k, discretisation="sv", **kw)
            made[case, burman] = (s, run_solver(s, list(RES)))
        return made[case, burman]
    yield get
    for s, _ in made.values():
        s.close()


def _run_ranks(tmp_path, case, world, transport="callback", min_dofs=1, burman=0.0, device_state=True):
    port = _free_port()
    procs = []
    try:
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="4")
            if transport == "rccl":
                from tests.mock_rccl.build import build
                env.update(ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=build())
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_sv_state_worker.py"),
                                           str(tmp_path), case, str(min_dofs), repr(burman), "1" if device_state else "0"],
                                          env=env, cwd=ROOT))
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return np.load(os.path.join(str(tmp_path), "sv_state.npz"))


def _compare_counts_and_state(z, s, res):
    """The tolerances of test_partitioned_newton."""
    assert all(z["conv"]) and all(res[r]["converged"] for r in RES)
    assert list(z["newton"]) == [res[r]["nonlinear_iter"] for r in RES], (list(z["newton"]), res)
    assert all(abs(int(a) - res[r]["linear_iter"]) <= 2 for a, r in zip(z["its"], RES)), (list(z["its"]), res)
    assert np.abs(z["u"] - s.u).max() < 1e-7 * np.abs(s.u).max()
    assert np.abs(z["p"] - s.p).max() < 1e-6 * np.abs(s.p).max()


def _check_resident(z, world):
    print("resident %s, bytes across PCIe per Newton step and rank %s, host assemblies %s, level-state error %s (max|u| %.3g)"
          % (list(z["resident"]), list(z["bytes_per_step"]), list(z["host_assemblies"]), list(z["state_err"]),
             np.abs(z["u"]).max()))
    assert all(z["device_assembly"]) and all(z["resident"]), (z["device_assembly"], z["resident"])
    assert max(z["bytes_per_step"]) <= 1024, z["bytes_per_step"]
    assert list(z["host_assemblies"]) == [0] * world, z["host_assemblies"]
    assert min(z["levels_checked"]) >= 1
    assert 0.0 <= max(z["state_err"]) <= 1e-13 * np.abs(z["u"]).max(), z["state_err"]


@pytest.mark.parametrize("case,world,transport,burman", [("2d", 2, "callback", 0.0), ("2d", 3, "rccl", 0.0),
                                                         ("3d", 2, "callback", 0.0), ("2d", 2, "callback", WEIGHT)])
def test_partitioned_sv_newton_state_on_the_devices(tmp_path, reference, case, world, transport, burman):
    """[P2]^2 on 2 ranks (gloo callback) and on 3 over tests/mock_rccl, [P3]^3 on 2 ranks (true interpolation weights on the
    coarse level), [P2]^2 with Burman terms (the state grows by the nodes of the facets' off-rank cells); every level
    partitioned."""
    s, res = reference(case, burman)
    z = _run_ranks(tmp_path, case, world, transport, burman=burman)
    _check_resident(z, world)
    _compare_counts_and_state(z, s, res)


def test_partitioned_sv_newton_state_single_owner_coarse_levels(tmp_path, reference):
    """min_dofs = the finest level's size: the coarse levels live on rank 0 alone and pull their columns of the composed
    injection through the same exchange; the finest is partitioned."""
    s, res = reference("2d")
    z = _run_ranks(tmp_path, "2d", 2, min_dofs=s.levels[-1].n)
    _check_resident(z, 2)
    _compare_counts_and_state(z, s, res)


def test_partitioned_sv_newton_replicated_state_kept(tmp_path, reference):
    """device_state=False: the replicated host loop, the same counts and solution."""
    s, res = reference("2d")
    z = _run_ranks(tmp_path, "2d", 2, device_state=False)
    assert not any(z["resident"])
    _compare_counts_and_state(z, s, res)
