"""The single calls are the one-column case of one driver per algorithm (csrc: smooth_fgmres_general, vcycle / fcycle,
saddle_solve_chunk), on workspaces of one type (csrc/krylov_ws.h).  -m gpu

No tolerance anywhere: every comparison is bit for bit.  Shapes: the banded operators of tests/block_fused_cases.py (NB block
rows, block size 2, and block size 3 for an odd n and a padded ldv), a 2-D hierarchy of three levels (N = 4, two refinements:
levels >= 2 recurse twice in a W-cycle), and the small Stokes problem of tests/test_gpu_block_rhs.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import hip
from tests import block_fused_cases as fc

SENTINEL = -7.25


def _wide(n, extra):
    return ((n + 1) & ~1) + extra


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _banded(ctx, bs, half):
    dl = hip.Level(ctx, fc.banded_operator(fc.NB, half, bs, 5), np.arange(0, 4 * bs, dtype=np.int32))
    dl.set_patches(*fc.window_patches(fc.NB, bs, 7 if bs == 2 else 5, 301, 6))
    dl.set_patch_groups(None)
    dl.factor()
    return dl


@pytest.fixture(scope="module", params=[(2, 2), (3, 5)], ids=["bs2", "bs3"])
def banded(ctx, request):
    dl = _banded(ctx, *request.param)
    yield dl
    dl.close()


def _one_column_calls(n, single, block):
    """single(b, x0) -> x and block(B, X, cols) (in place) agree: ncol = 1, and cols = [2] of a 3-column operand with ldx > n"""
    rng = np.random.default_rng(31)
    B, X0 = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    ref = [single(B[:, c], X0[:, c]) for c in range(3)]
    assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0.0
    return B, X0, ref


def _check_one_column(ctx, n, single, block):
    B, X0, ref = _one_column_calls(n, single, block)
    dB, dX = ctx.mat(B[:, :1]), ctx.mat(X0[:, :1])
    block(dB, dX, None)
    assert np.array_equal(dX.get()[:, 0], ref[0])
    Xs = X0.copy()
    Xs[:, :2] = SENTINEL
    dB, dX = ctx.mat(B, ld=_wide(n, 2)), ctx.mat(Xs, ld=_wide(n, 6))
    block(dB, dX, [2])
    got = dX.get()
    assert np.array_equal(got[:, 2], ref[2]) and np.all(got[:, :2] == SENTINEL)
    assert np.array_equal(dB.get(), B)


# ---- one-column block calls are the single call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("guess", [False, True])
def test_one_column_smoother_on_the_general_path(ctx, banded, guess):
    dl, k = banded, 16                                                # k + 1 <= 16 fails: the general path on any level
    assert dl.smooth_block_mode(k) == fc.LOCKSTEP

    def single(b, x0):
        db, dx = ctx.vec(b), ctx.vec(x0)
        dl.smooth(k, db, dx, nonzero_guess=guess)
        return dx.get()
    _check_one_column(ctx, dl.n, single, lambda dB, dX, cols: dl.smooth_block(k, dB, dX, nonzero_guess=guess, cols=cols))


@pytest.fixture(scope="module")
def hier(ctx):
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, build_hierarchy
    lv, tr = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=100.0)
    assert len(lv) == 3
    mg = hip.Multigrid(ctx, lv, tr, 2)
    yield mg, lv
    mg.close()


@pytest.mark.parametrize("cycle_type", ["v", "w"])
@pytest.mark.parametrize("smoother", ["fgmres", "chebyshev"])
def test_one_column_cycles(ctx, hier, smoother, cycle_type):
    mg, lv = hier
    n = lv[-1].n
    try:
        mg.set_cycle_type(cycle_type)
        if smoother == "chebyshev":
            mg.set_smoother("chebyshev", mg.chebyshev_bounds())
        for one, blk in ((mg.vcycle, mg.vcycle_block), (mg.fcycle, mg.fcycle_block)):
            def single(b, x0):
                db, dx = ctx.vec(b), ctx.vec(x0)
                one(db, dx)
                return dx.get()
            _check_one_column(ctx, n, single, lambda dB, dX, cols: blk(dB, dX, cols=cols))
    finally:
        mg.set_smoother("fgmres")
        mg.set_cycle_type("v")


@pytest.fixture(scope="module")
def ns():
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 1, 2)
    _, info = s.solve(10.0)
    assert info["converged"]
    yield s
    s.ctx.set_graph(False)
    s.close()


def _saddle_rhs(s, ncol, seed=21):
    n, nu = s.n_u + s.n_p, s.n_u
    B = np.random.default_rng(seed).standard_normal((n, ncol))
    B[s.levels[-1].bc_dofs] = 0.0
    B[nu:] -= B[nu:].mean(axis=0)
    return B


def test_one_column_outer_solve_across_restarts(ns):
    s, restart = ns, 3
    sad, ctx, n = s.saddle, s.ctx, s.n_u + s.n_p
    B = _saddle_rhs(s, 3)
    atol = 1e-7 * np.linalg.norm(B[:, 0])
    ref = []
    for c in range(3):
        db, dx = ctx.vec(B[:, c]), ctx.vec(n)
        its, rn = sad.solve(db, dx, 1e-6, atol, 200, restart)
        ref.append((its, rn, dx.get()))
    assert all(restart < r[0] < 200 for r in ref), [r[0] for r in ref]          # every column restarted, and converged
    dX = ctx.mat(np.full((n, 1), SENTINEL))
    its, rn = sad.solve_block(ctx.mat(B[:, :1]), dX, 1e-6, atol, 200, restart)
    assert list(its) == [ref[0][0]] and list(rn) == [ref[0][1]] and np.array_equal(dX.get()[:, 0], ref[0][2])
    dX = ctx.mat(np.full((n, 3), SENTINEL), ld=_wide(n, 4))
    its, rn = sad.solve_block(ctx.mat(B, ld=_wide(n, 2)), dX, 1e-6, atol, 200, restart, cols=[2])
    got = dX.get()
    assert list(its) == [ref[2][0]] and list(rn) == [ref[2][1]]
    assert np.array_equal(got[:, 2], ref[2][2]) and np.all(got[:, :2] == SENTINEL)


# ---- block calls do not disturb a captured single cycle -------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["vcycle", "saddle_solve"])
def test_block_calls_leave_the_single_workspaces_alone(ns, what):
    s = ns
    ctx, mg, sad, F = s.ctx, s.hmg.mg, s.saddle, s.hmg.mg.levels[-1]
    nf, n = F.n, s.n_u + s.n_p
    rng = np.random.default_rng(8)
    b = rng.standard_normal(nf)
    b[s.levels[-1].bc_dofs] = 0.0
    rhs = _saddle_rhs(s, 4, seed=9)
    atol = 1e-7 * np.linalg.norm(rhs[:, 0])
    db, dx = ctx.vec(b), ctx.vec(nf)
    dr, ds = ctx.vec(rhs[:, 0]), ctx.vec(n)

    def single():
        if what == "vcycle":
            dx.zero()
            mg.vcycle(db, dx)
            return dx.get()
        its, rn = sad.solve(dr, ds, 1e-6, atol, 200, 3)
        return np.concatenate([ds.get(), [its, rn]])
    ctx.set_graph(True)
    try:
        first = [single() for _ in range(3)]                            # eager, capture, replay
        assert np.array_equal(first[0], first[1]) and np.array_equal(first[0], first[2])
        Bf = rng.standard_normal((nf, 4))
        Bf[s.levels[-1].bc_dofs] = 0.0
        mg.vcycle_block(ctx.mat(Bf), ctx.mat(nf, 4))
        F.smooth_block(mg.k, ctx.mat(Bf), ctx.mat(nf, 4), nonzero_guess=False)
        its, _ = sad.solve_block(ctx.mat(rhs), ctx.mat(n, 4), 1e-6, atol, 200, 5)
        assert max(its) > 0
        again = single()                                                # the replay of the graph captured before the block calls
        assert np.array_equal(again, first[0])
        assert np.array_equal(single(), first[0])
    finally:
        ctx.set_graph(False)


# ---- growing the block workspace keeps earlier columns' results ------------------------------------------------------------------------
def test_growing_the_block_workspace(ctx):
    dl = _banded(ctx, 3, 5)
    try:
        n = dl.n
        rng = np.random.default_rng(17)
        B, X0 = rng.standard_normal((n, 4)), rng.standard_normal((n, 4))

        def run(k, ncol):
            dX = ctx.mat(X0[:, :ncol])
            dl.smooth_block(k, ctx.mat(B[:, :ncol]), dX, nonzero_guess=True)
            return dX.get()

        def single(k):
            db, dx = ctx.vec(B[:, 0]), ctx.vec(X0[:, 0])
            dl.smooth(k, db, dx, nonzero_guess=True)
            return dx.get()
        k = 16                                                          # the lockstep mode: the block Krylov workspace itself
        two = run(k, 2)
        four = run(k, 4)                                                # the workspace grows from 2 to 4 slots
        assert np.array_equal(run(k, 2), two) and np.array_equal(four[:, :2], two)
        # K of the single workspace only grows: k = 3 computes the same before and after k = 5 (levels of the four-launch iteration
        # and its block form, whose workspaces follow the single one's K)
        dl2 = _banded(ctx, 2, 2)
        try:
            X0b, Bb = X0[:dl2.n], B[:dl2.n]

            def run2(k, ncol):
                dX = ctx.mat(X0b[:, :ncol])
                dl2.smooth_block(k, ctx.mat(Bb[:, :ncol]), dX, nonzero_guess=True)
                return dX.get()

            def single2(k):
                db, dx = ctx.vec(Bb[:, 0]), ctx.vec(X0b[:, 0])
                dl2.smooth(k, db, dx, nonzero_guess=True)
                return dx.get()
            s3, b3 = single2(3), run2(3, 2)
            s5, b5 = single2(5), run2(5, 4)
            assert np.array_equal(single2(3), s3) and np.array_equal(run2(3, 2), b3)
            assert np.array_equal(b3[:, 0], s3) and np.array_equal(b5[:, 0], s5)
        finally:
            dl2.close()
        assert np.array_equal(single(3), run(3, 1)[:, 0])
    finally:
        dl.close()


# ---- partitioned single calls: the exchanges and all-reduces of the launch chain ------------------------------------------------------
@pytest.mark.parametrize("exact", ["1", "0"])
def test_partitioned_single_calls_exchange_what_the_launch_chain_says(tmp_path, exact):
    """Two ranks over the mock transport, three levels all partitioned, FGMRES(3), no overlapped exchanges, plain restriction.
    Counts per rank (alfi_ctx_comm_stats), from the launch chain of smooth_fgmres_general and vcycle:

    smoother, zero guess: per iteration the forward exchange of the patch solves' input and ONE sum exchange of their result --
    the product takes the ghost values from it (ghosts_current) and exchanges nothing: 2 k halo exchanges; all-reduces: |r0|,
    then per iteration the dots and, with the exact norm, |w - V h|: 1 + 2 k (1 + k with the Pythagorean norm).

    V-cycle: level 2 smooths twice with a nonzero guess (one more forward exchange each, for r0 = b - A x), level 1 once with a
    zero and once with a nonzero guess; per level >= 1 the residual (1), the restriction (1 reverse-add on the coarse level) and
    the prolongation (2 forward): (2 + 4 k + 4) + (1 + 4 k + 4) = 8 k + 11 exchanges and 4 smoother calls' all-reduces."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from tests.mock_rccl.build import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world, lib = 2, build()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="4", ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=lib,
                   ALFI_DIST_OVERLAP="0", ALFI_DIST_EXACT_NORM=exact)
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "dist_gpu_one_driver_worker.py"),
                                       "2d-all-distributed", str(tmp_path)], env=env, cwd=root))
    for p in procs:
        assert p.wait(timeout=300) == 0
    k = 3
    per_call = 1 + 2 * k if exact == "1" else 1 + k
    for r in range(world):
        with open(os.path.join(str(tmp_path), "rank%d.json" % r)) as f:
            got = json.load(f)
        print("rank", r, got)
        assert got["k"] == k and got["levels"] == 3 and got["overlap_levels"] == [] and got["finite"]
        assert got["smooth"] == [6, per_call] == [2 * k, per_call]
        assert got["vcycle"] == [35, 4 * per_call] == [8 * k + 11, 4 * per_call]
