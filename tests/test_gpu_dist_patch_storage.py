"""Single-precision patch storage on PARTITIONED levels (DistMultigrid(patch_factor_dtype="f32"): every rank asks its own local
levels, no collective) against the single-GPU path with the same storage.  -m gpu; the ranks (at most 3) share the box's one GPU,
worker: tests/dist_gpu_patch_storage_worker.py.

Shapes: ldc3d [P2+FB]^3, N = 2, nref 2, Re 1000 (tests/test_gpu_dist_star_condense.py): 125 and 729 patches, stars of 153 dofs and
every boundary shape; with the overlap forced on every apply is three range launches of the FP32 kernel.
Tolerances: applies 1e-8 of the largest entry, cycles 1e-5 (tests/test_gpu_dist_star_condense.py) -- against single-GPU results
that store FP32 too.

Every rank eliminates its patches in the order of the unpartitioned patch (dist.localize_level: patch_rank ->
alfi_patches_set_canonical_order), so its float32 values are those of the single-GPU level; without that order the FP64 inverses
differ by round-off (ghost dofs are numbered last), entries cross float32 rounding boundaries, and applies agreed to 0.8-1.4e-8,
two V-cycles to 2.7e-5 only (FP64 storage: 1e-10 and 5e-8)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dist_gpu_patch_storage_worker.py")
APPLY_TOL = 1e-8
CYCLE_TOL = 1e-5


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _run_ranks(tmp_path, world, overlap, transport):
    port = _free_port()
    procs = []
    try:
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="4")
            if transport == "rccl":
                from tests.mock_rccl.build import build
                env.update(ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=build(), ALFI_TEST_EXPECT_TRANSPORT="rccl")
            procs.append(subprocess.Popen([sys.executable, WORKER, str(tmp_path), str(overlap)], env=env, cwd=ROOT))
        for p in procs:                                       # every rank under its own time limit, every exit status checked
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]


@pytest.fixture(scope="module")
def reference():
    """The single-GPU results with FP32 storage, computed once: the patch apply of levels 1 and 2, two V-cycles, a full cycle."""
    from alfi_amd import hip
    from tests.dist_gpu_star_condense_worker import K, hierarchy, level_input
    lv, tr = hierarchy()
    ctx = hip.Context(0)
    ref = {"n": [L.n for L in lv]}
    b = np.random.default_rng(0).standard_normal(lv[-1].n)
    b[lv[-1].bc_dofs] = 0.0
    mg = hip.Multigrid(ctx, lv, tr, K, patch_factor_dtype="f32")
    assert [d.patch_storage_dtype() for d in mg.levels[1:]] == ["f32", "f32"] and [d.condensed() for d in mg.levels[1:]] == [0, 0]
    ref["bytes"] = [d.factor_bytes() for d in mg.levels[1:]]
    for L, dl in zip(lv[1:], mg.levels[1:]):
        dx, dy = ctx.vec(level_input(L)), ctx.vec(L.n)
        dl.patch_apply(dx, dy)
        ref["apply%d" % L.level] = dy.get()
    db, dx = ctx.vec(b), ctx.vec(lv[-1].n)
    mg.vcycle(db, dx)
    mg.vcycle(db, dx)
    ref["xv"] = dx.get()
    mg.fcycle(db, dx)
    ref["xf"] = dx.get()
    mg.close()
    ctx.close()
    return ref


def _assemble(ranks, key, dofs_key, n):
    out = np.full(n, np.nan)
    for z in ranks:
        out[z[dofs_key]] = z[key]
    assert not np.isnan(out).any()
    return out


@pytest.mark.parametrize("world,transport,overlap", [(2, "callback", 0), (2, "callback", 1), (3, "rccl", 0), (3, "rccl", 1)])
def test_partitioned_levels_store_single_precision(tmp_path, reference, world, transport, overlap):
    """2 ranks over the gloo callback, 3 over tests/mock_rccl; overlap off and forced on."""
    ranks = _run_ranks(tmp_path, world, overlap, transport)
    for r, z in enumerate(ranks):
        assert list(z["levels"]) == [1, 2]
        assert list(z["overlap_levels"]) == ([1, 2] if overlap else [])
        assert list(z["dtypes"]) == ["f32", "f32"] and list(z["noted"]) == ["f32", "f32"] and list(z["modes"]) == [0, 0]
        worst, flagged, repaired = z["probes"][:, 0], z["probes"][:, 1], z["probes"][:, 2]
        assert (worst >= 0.0).all() and (worst < 1e-6).all() and np.array_equal(flagged, repaired)
        assert z["repeat1"] == 1 and z["repeat2"] == 1                          # bitwise reproducible
        print("rank %d: factor bytes %s (one GPU: %s)" % (r, list(z["bytes"]), reference["bytes"]))
    for lev in (1, 2):
        e = relerr(_assemble(ranks, "apply%d" % lev, "dofs%d" % lev, reference["n"][lev]), reference["apply%d" % lev])
        print("level %d: patch apply against the single-GPU FP32 apply %.3e" % (lev, e))
        assert e < APPLY_TOL
    for key in ("xv", "xf"):
        e = relerr(_assemble(ranks, key, "dofs2", reference["n"][2]), reference[key])
        print("%s against the single-GPU FP32 cycles %.3e" % (key, e))
        assert e < CYCLE_TOL
