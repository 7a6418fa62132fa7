"""Vertex-star patch factors condensed by the library itself on PARTITIONED levels (the automatic policy of alfi_patches_factor,
rank-local: every rank looks for groups in its own sparsity and patch lists; forced at these sizes with the keyword
condense_min_bytes=0 of DistMultigrid / DistNavierStokesSolver) against the single-GPU path with dense inverses.  -m gpu; the
ranks (at most 3) share the box's one GPU, worker: tests/dist_gpu_star_condense_worker.py.

Shapes: ldc3d [P2+FB]^3, N = 2, nref 2, Re 1000 (tests/test_gpu_star_condense.py): 125 and 729 patches, full stars of 153 dofs and
every boundary shape (3 / 9 / 21 / 33 / 57 dofs); every range launch of an overlapped exchange stays below 1024 patches and takes
the chunked form of the condensed apply.  The workgroup-per-patch form of a range launch: the N = 8 level with its patch set
listed three times (2187 patches, all interior) as a one-rank forced partition with the overlapped sequence on, whose two
interior ranges hold 1093 and 1094 patches (in-process, well under a second; the alternative, the N = 16 level on 2 ranks, has
4913 patches and 8 times the dofs).
Tolerances: condensed against dense applies 1e-8 of the largest entry (tests/test_gpu_star_condense.py), cycles 1e-5
(CYCLE_TOL, tests/test_gpu_parity.py), multiplicative sweeps and the Newton solution those of tests/test_gpu_dist.py."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dist_gpu_star_condense_worker.py")
APPLY_TOL = 1e-8
CYCLE_TOL = 1e-5
# columns of the worker's storage report
LEVEL, MODE, BYTES, DENSE, GROUPED, NOTED, NOTED_BYTES, CONDENSE_PATCHES = range(8)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _run_ranks(tmp_path, world, args, transport="callback", env_extra=None):
    port = _free_port()
    procs = []
    try:
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="4")
            if transport == "rccl":
                from tests.mock_rccl.build import build
                env.update(ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=build(), ALFI_TEST_EXPECT_TRANSPORT="rccl")
            env.update(env_extra or {})
            procs.append(subprocess.Popen([sys.executable, WORKER, str(tmp_path)] + [str(a) for a in args], env=env, cwd=ROOT))
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world) if
            os.path.exists(os.path.join(str(tmp_path), "rank%d.npz" % r))]


@pytest.fixture(scope="module")
def reference():
    """The single-GPU results with dense inverses (default threshold), computed once: the patch apply of levels 1 and 2, two
    V-cycles and a full cycle with either restriction."""
    from alfi_amd import hip
    from tests.dist_gpu_star_condense_worker import K, hierarchy, level_input
    lv, tr = hierarchy()
    ctx = hip.Context(0)
    ref = {"n": [L.n for L in lv]}
    b = np.random.default_rng(0).standard_normal(lv[-1].n)
    b[lv[-1].bc_dofs] = 0.0
    for robust in (0, 1):
        mg = hip.Multigrid(ctx, lv, tr, K, robust_restriction=bool(robust))
        assert [d.condensed() for d in mg.levels[1:]] == [0, 0]
        if robust == 0:
            for L, dl in zip(lv[1:], mg.levels[1:]):
                dx, dy = ctx.vec(level_input(L)), ctx.vec(L.n)
                dl.patch_apply(dx, dy)
                ref["apply%d" % L.level] = dy.get()
        db, dx = ctx.vec(b), ctx.vec(lv[-1].n)
        mg.vcycle(db, dx)
        mg.vcycle(db, dx)
        ref["xv%d" % robust] = dx.get()
        mg.fcycle(db, dx)
        ref["xf%d" % robust] = dx.get()
        mg.close()
    ctx.close()
    return ref


def _assemble(ranks, key, dofs_key, n):
    out = np.full(n, np.nan)
    for z in ranks:
        out[z[dofs_key]] = z[key]
    assert not np.isnan(out).any()
    return out


def _check_cycles_run(ranks, ref, world, overlap, condensed):
    assert len(ranks) == world
    total = {}
    for r, z in enumerate(ranks):
        assert list(z["distributed"][1:]) == [1, 1]
        assert list(z["overlap_levels"]) == ([1, 2] if overlap else [])
        st = z["storage"]
        assert list(st[:, LEVEL]) == [1, 2] and np.array_equal(st, z["storage_after"])
        for row in st:
            want = 2 if condensed and row[GROUPED] else 0
            print("rank %d level %d: mode %d, %d factor bytes (dense %d)" % (r, row[LEVEL], row[MODE], row[BYTES], row[DENSE]))
            assert row[MODE] == want and row[NOTED] == want and row[CONDENSE_PATCHES] == (want == 2)
            assert row[NOTED_BYTES] == row[BYTES]
            assert (row[BYTES] < row[DENSE]) if want == 2 else (row[BYTES] == row[DENSE])
            t = total.setdefault(int(row[LEVEL]), [0, 0])
            t[0] += int(row[BYTES])
            t[1] += int(row[DENSE])
        if condensed:
            assert st[:, GROUPED].all()             # at this shape every rank owns full stars on both levels
        worst, flagged, repaired = z["probes"][:, 0], z["probes"][:, 1], z["probes"][:, 2]
        assert (worst >= 0.0).all() and (worst < 1e-6).all() and np.array_equal(flagged, repaired)
        assert z["repeat1"] == 1 and z["repeat2"] == 1                          # bitwise reproducible
    for lev, (got, dense) in sorted(total.items()):
        print("level %d: factor bytes over the ranks %d, dense %d: ratio %.3f" % (lev, got, dense, got / dense))
        assert (got < dense) if condensed else (got == dense)
    for lev in (1, 2):
        y = _assemble(ranks, "apply%d" % lev, "dofs%d" % lev, ref["n"][lev])
        e = relerr(y, ref["apply%d" % lev])
        print("level %d: patch apply against the single-GPU dense apply %.3e" % (lev, e))
        assert e < APPLY_TOL
    for robust in (0, 1):
        for key in ("xv%d" % robust, "xf%d" % robust):
            x = _assemble(ranks, key, "dofs2", ref["n"][2])
            e = relerr(x, ref[key])
            print("%s against the single-GPU cycles %.3e" % (key, e))
            assert e < CYCLE_TOL


RUNS = [(2, "callback", 0), (2, "callback", 1), (3, "rccl", 0), (3, "rccl", 1)]


@pytest.mark.parametrize("world,transport,overlap", RUNS)
def test_partitioned_levels_condense_themselves(tmp_path, reference, world, transport, overlap):
    """2 ranks over the gloo callback, 3 over tests/mock_rccl; overlap off and forced on; in every run both restrictions.  Every
    rank stores condensed factors on the groups it found itself (mode 2) on both smoothed levels -- dense inverses (0) before
    partitioned levels looked for groups -- and applies and cycles equal the single-GPU ones with dense inverses."""
    ranks = _run_ranks(tmp_path, world, ["cycles", 0, overlap], transport)
    _check_cycles_run(ranks, reference, world, overlap, True)


@pytest.mark.parametrize("world,transport,overlap", RUNS)
def test_partitioned_levels_below_the_default_threshold_stay_dense(tmp_path, reference, world, transport, overlap):
    ranks = _run_ranks(tmp_path, world, ["cycles", "none", overlap], transport)
    _check_cycles_run(ranks, reference, world, overlap, False)


def test_partitioned_levels_stay_dense_without_alfi_condense(tmp_path, reference):
    ranks = _run_ranks(tmp_path, 2, ["cycles", 0, 1], env_extra={"ALFI_CONDENSE": "0"})
    _check_cycles_run(ranks, reference, 2, 1, False)


def test_range_launches_of_a_thousand_patches_and_more():
    """The workgroup-per-patch kernels of the condensed apply in RANGE launches (the overlapped sequence of a partitioned level):
    a one-rank forced partition of the N = 8 level, its 729 patches listed three times -- no ghosts, so the two interior ranges
    are [0, 1093) and [1093, 2187)."""
    from alfi_amd import hip
    from alfi_amd.dist import DistMultigrid
    from tests.dist_gpu_star_condense_worker import K, hierarchy, level_input
    lv, tr = hierarchy()
    lv = list(lv)
    L = lv[2] = copy.copy(lv[2])
    pp = np.asarray(L.patch_ptr, dtype=np.int64)
    L.patch_ptr = np.concatenate([pp, pp[1:] + pp[-1], pp[1:] + 2 * pp[-1]])
    L.patch_dofs = np.tile(L.patch_dofs, 3)
    L.patch_seeds = np.tile(L.patch_seeds, 3)
    npatch = len(L.patch_ptr) - 1
    assert npatch == 2187 and npatch // 2 >= 1024
    b = np.random.default_rng(0).standard_normal(L.n)
    b[L.bc_dofs] = 0.0
    x = level_input(L)
    ctx = hip.Context(0)
    mg = hip.Multigrid(ctx, lv, tr, K)
    assert [d.condensed() for d in mg.levels[1:]] == [0, 0]
    dx, dy, db, du = ctx.vec(x), ctx.vec(L.n), ctx.vec(b), ctx.vec(L.n)
    mg.levels[2].patch_apply(dx, dy)
    ref_y = dy.get()
    mg.vcycle(db, du)
    mg.vcycle(db, du)
    ref_v = du.get()
    mg.fcycle(db, du)
    ref_f = du.get()
    mg.close()
    ctx.close()
    dmg = DistMultigrid(lv, tr, K, solo=(0, 1), min_dofs=1, force_distributed=True, overlap=True, overlap_min_dofs=0,
                        condense_min_bytes=0)
    try:
        assert dmg.overlap_levels == [1, 2] and all(p.distributed for p in dmg.parts[1:])
        fin = dmg.local_levels[2]
        assert fin.npatch_int == npatch and fin.n == fin.n_own == L.n
        assert [s[0] for s in dmg.patch_storage()[1:]] == [2, 2]
        worst, flagged, repaired, _ = dmg.levels[2].patch_check()
        assert 0.0 <= worst < 1e-6 and flagged == repaired
        own = fin.part.own_dofs()
        dx, dy = dmg.local_vec(x), dmg.local_vec()
        dmg.levels[2].patch_apply(dx, dy)
        y = np.empty(L.n)
        y[own] = dmg.owned(dy)
        print("1093 + 1094 patches: apply against dense %.3e, factor bytes %.3f of dense"
              % (relerr(y, ref_y), dmg.levels[2].factor_bytes() / float(_dense_bytes(L.patch_ptr))))
        assert relerr(y, ref_y) < APPLY_TOL
        assert dmg.levels[2].factor_bytes() < _dense_bytes(L.patch_ptr)
        db, du = dmg.local_vec(b), dmg.local_vec()
        v = np.empty(L.n)
        dmg.vcycle(db, du)
        dmg.vcycle(db, du)
        v[own] = dmg.owned(du)
        assert relerr(v, ref_v) < CYCLE_TOL
        dmg.fcycle(db, du)
        v[own] = dmg.owned(du)
        assert relerr(v, ref_f) < CYCLE_TOL
    finally:
        dmg.close()


def _dense_bytes(patch_ptr):
    from tests.dist_gpu_star_condense_worker import dense_bytes
    return dense_bytes(patch_ptr)


def test_multiplicative_sweeps_send_a_partitioned_level_back_to_dense(tmp_path):
    """set_multiplicative on partitioned levels that condensed themselves (3 ranks, the case of test_partitioned_multiplicative):
    back to dense inverses for good, and the sweep and the V-cycle equal the SPMD oracle's on the same rank-local data."""
    ranks = _run_ranks(tmp_path, 3, ["mult"])
    assert len(ranks) == 3
    for z in ranks:
        before, after, again = z["before"], z["after"], z["refactored"]
        assert len(before) == 1 and before[0, GROUPED] == 1
        assert before[0, MODE] == 2 and before[0, NOTED] == 2 and before[0, BYTES] < before[0, DENSE]
        for st in (after, again):
            assert st[0, MODE] == 0 and st[0, NOTED] == 0 and st[0, BYTES] == st[0, DENSE] and st[0, CONDENSE_PATCHES] == 0
        print("sweep %.3e, V-cycle %.3e against the oracle" % (float(z["e1"]), float(z["e2"])))
        assert float(z["e1"]) < 1e-7 and float(z["e2"]) < 1e-5


def test_partitioned_newton_on_levels_that_condense_themselves(tmp_path):
    """[P2+FB]^3-P0 Newton with Reynolds continuation 10 -> 100 on 2 ranks, operators formed on the device: the levels decide at
    the solver's first refresh (not at construction), hold mode 2 after every refresh with a clean residual probe, and the run
    takes the Newton steps of the single-GPU solver (dense inverses), Krylov counts within 2, the same solution."""
    from alfi_amd.nssolver import HipNavierStokesSolver, run_solver
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem
    from tests.dist_gpu_star_condense_worker import RES
    port = _free_port()
    procs = []
    try:
        for r in range(2):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       OMP_NUM_THREADS="4")
            procs.append(subprocess.Popen([sys.executable, WORKER, str(tmp_path), "newton"], env=env, cwd=ROOT))
        s = HipNavierStokesSolver(ThreeDimLidDrivenCavityProblem(2), 1, 2)      # the reference while the ranks run
        res = run_solver(s, list(RES))
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    try:
        z = np.load(os.path.join(str(tmp_path), "rank0.npz"))
        assert all(z["device_assembly"])
        newton = [res[r]["nonlinear_iter"] for r in RES]
        assert min(z["refreshes"]) >= sum(newton) and len(set(z["refreshes"].tolist())) == 1
        st, pr = z["storage"], z["probes"]
        assert len(st) == 2 * int(z["refreshes"][0]) and len(pr) == len(st)      # one smoothed level, two ranks
        assert (st[:, GROUPED] == 1).all() and (st[:, MODE] == 2).all() and (st[:, NOTED] == 2).all()
        assert (st[:, BYTES] < st[:, DENSE]).all()
        print("probe: worst %.3e, flagged %d, repaired %d" % (pr[:, 0].max(), pr[:, 1].sum(), pr[:, 2].sum()))
        assert (pr[:, 0] >= 0.0).all() and (pr[:, 0] < 1e-6).all() and np.array_equal(pr[:, 1], pr[:, 2])
        assert all(z["conv"]) and all(res[r]["converged"] for r in RES)
        assert list(z["newton"]) == newton
        assert all(abs(int(a) - res[r]["linear_iter"]) <= 2 for a, r in zip(z["its"], RES)), (list(z["its"]), res)
        assert np.abs(z["u"] - s.u).max() < 1e-7 * np.abs(s.u).max()
        assert np.abs(z["p"] - s.p).max() < 1e-6 * np.abs(s.p).max()
    finally:
        s.close()


def test_partitioned_burman_levels_stay_dense(tmp_path):
    """The Burman-stabilised Scott-Vogelius pair on 2 ranks with the threshold at 0: dense inverses on every level, before and
    after a Newton solve (the facet term couples macro interiors; PCPATCH's facet rule changes the patch matrices)."""
    ranks = _run_ranks(tmp_path, 2, ["burman"])
    assert len(ranks) == 2
    for z in ranks:
        assert bool(z["conv"])
        for st in (z["before"], z["after"]):
            assert len(st) == 2
            assert (st[:, MODE] == 0).all() and (st[:, NOTED] == 0).all() and (st[:, CONDENSE_PATCHES] == 0).all()
        assert (z["after"][:, BYTES] == z["after"][:, DENSE]).all()
