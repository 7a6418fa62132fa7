#!/usr/bin/env python3
"""What the host drivers (level smoother, V / full cycle, outer FGMRES) launch and compute, as one JSON document: for a fixed
list of small cases the SHA-256 of every result vector, the profiling-event counts per (level, event kind) and the ctx's
communication counters.  Two trees that print the same document run the same kernels the same number of times on the same
data -- the check of a host-only refactor:

    python scripts/driver_digest.py > new.json          # and the same command in a checkout of the other revision

Uses only the Python layer (alfi_amd/hip.py, dist.py, nssolver.py), so it runs unchanged on older revisions.  Needs a GPU.
Every hierarchy has THREE levels (two refinements), so that a W-cycle recurses twice on level 2 and the full cycle passes
through an intermediate level.  Cases: banded levels of block size 2 and 3 on the smoother's general path (k = 16; zero and
nonzero initial guess; 1 and 4 columns, a column list of a wider operand), additive and with multiplicative sweeps; the 2-D
hierarchy (V, W and full cycles, FGMRES and Chebyshev smoother, block forms, captured replay); a 3-D hierarchy with condensed
patch factors; the saddle solve with restarts, single and block; a one-rank forced partition (the partitioned branches of the
smoother, the cycles and the outer solve); two ranks over the mock transport (tests/mock_rccl), every level partitioned, without
and with overlapped exchanges -- without, the sum exchange after the patch solves hands the ghost values to the product."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alfi_amd import hip                                                                  # noqa: E402
from alfi_amd.problem import (ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem, build_hierarchy,   # noqa: E402
                              build_pressure_coupling)
from tests import block_fused_cases as fc                                                 # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


class Recorder(object):
    def __init__(self, ctx, level_ids):
        self.ctx, self.ids, self.out = ctx, list(level_ids), {}

    def run(self, name, fn):
        """fn() -> arrays; recorded with the events and the communication it caused"""
        ctx = self.ctx
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.comm_stats(reset=True)
        res = fn()
        ctx.sync()
        prof = {"%d/%s" % (i, ev): c for i in self.ids for ev, (_, c) in sorted(ctx.prof_get(i).items()) if c}
        comm = list(ctx.comm_stats(reset=True))
        ctx.prof_enable(False)
        self.out[name] = {"sha256": [sha(r) for r in res], "events": prof, "comm": comm}


def wide(n, extra):
    return ((n + 1) & ~1) + extra


def smoother_cases(rec, ctx, dl, tag, k):
    n = dl.n
    rng = np.random.default_rng(7)
    B, X0 = rng.standard_normal((n, 4)), rng.standard_normal((n, 4))
    for guess in (False, True):
        def single():
            out = []
            for c in range(2):
                db, dx = ctx.vec(B[:, c]), ctx.vec(X0[:, c])
                dl.smooth(k, db, dx, nonzero_guess=guess)
                out.append(dx.get())
            return out

        def block(ncol, cols=None):
            def f():
                dB, dX = ctx.mat(B[:, :max(ncol, 3)], ld=wide(n, 2)), ctx.mat(X0[:, :max(ncol, 3)], ld=wide(n, 4))
                dl.smooth_block(k, dB, dX, nonzero_guess=guess, cols=cols)
                return [dX.get()]
            return f
        rec.run("%s/smooth k=%d guess=%d" % (tag, k, guess), single)
        rec.run("%s/smooth_block 1 col k=%d guess=%d" % (tag, k, guess), block(1))
        rec.run("%s/smooth_block cols=[2] k=%d guess=%d" % (tag, k, guess), block(1, [2]))
        rec.run("%s/smooth_block 4 cols k=%d guess=%d" % (tag, k, guess), block(4))


def banded(out):
    ctx = hip.Context(0)
    for bs, half in ((2, 2), (3, 5)):
        A = fc.banded_operator(fc.NB, half, bs, 5)
        dl = hip.Level(ctx, A, np.arange(0, 4 * bs, dtype=np.int32))
        dl.set_patches(*fc.window_patches(fc.NB, bs, 7 if bs == 2 else 5, 301, 6))
        dl.set_patch_groups(None)
        dl.factor()
        rec = Recorder(ctx, [dl.id])
        smoother_cases(rec, ctx, dl, "banded bs=%d" % bs, 16)
        smoother_cases(rec, ctx, dl, "banded bs=%d" % bs, 3)
        try:
            dl.set_multiplicative(np.arange(301), True)           # multiplicative sweeps, natural order
        except hip.AlfiHipError as e:                             # (a level that refuses them is recorded as such)
            rec.out["banded bs=%d multiplicative" % bs] = {"refused": str(e)}
        else:
            smoother_cases(rec, ctx, dl, "banded bs=%d multiplicative" % bs, 3)
        out.update(rec.out)
        dl.close()
    ctx.close()


def cycles(rec, ctx, mg, lv, tag):
    n = lv[-1].n
    B = np.random.default_rng(12).standard_normal((n, 4))
    B[lv[-1].bc_dofs] = 0.0

    def single(kind):
        def f():
            out = []
            for c in range(2):
                db, dx = ctx.vec(B[:, c]), ctx.vec(n)
                (mg.vcycle if kind == "v" else mg.fcycle)(db, dx)
                out.append(dx.get())
            return out
        return f

    def block(kind, ncol, cols=None):
        def f():
            dB, dX = ctx.mat(B, ld=wide(n, 2)), ctx.mat(np.zeros((n, 4)), ld=wide(n, 2))
            (mg.vcycle_block if kind == "v" else mg.fcycle_block)(dB, dX, cols=cols if cols else list(range(ncol)))
            return [dX.get()]
        return f
    for kind in ("v", "f"):
        rec.run("%s/%scycle" % (tag, kind), single(kind))
        rec.run("%s/%scycle_block 1 col" % (tag, kind), block(kind, 1))
        rec.run("%s/%scycle_block cols=[2]" % (tag, kind), block(kind, 1, [2]))
        rec.run("%s/%scycle_block 4 cols" % (tag, kind), block(kind, 4))


def hierarchy_2d(out):
    ctx = hip.Context(0)
    lv, tr = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=100.0)
    mg = hip.Multigrid(ctx, lv, tr, 2)
    rec = Recorder(ctx, [L.id for L in mg.levels])
    cycles(rec, ctx, mg, lv, "2d fgmres V")
    mg.set_cycle_type("w")
    cycles(rec, ctx, mg, lv, "2d fgmres W")
    mg.set_smoother("chebyshev", mg.chebyshev_bounds())
    cycles(rec, ctx, mg, lv, "2d chebyshev W")
    mg.set_cycle_type("v")
    cycles(rec, ctx, mg, lv, "2d chebyshev V")
    mg.set_smoother("fgmres")
    smoother_cases(rec, ctx, mg.levels[-1], "2d finest", 16)
    # captured replay: eager, capture, replay of the same pair (events cannot be recorded in a graph: results only)
    ctx.set_graph(True)
    n = lv[-1].n
    b = np.random.default_rng(3).standard_normal(n)
    b[lv[-1].bc_dofs] = 0.0
    db, dx = ctx.vec(b), ctx.vec(n)
    res = []
    for _ in range(3):
        dx.zero()
        mg.vcycle(db, dx)
        res.append(sha(dx.get()))
    ctx.set_graph(False)
    rec.out["2d graph/vcycle eager, capture, replay"] = {"sha256": res, "events": {}, "comm": [0, 0, 0]}
    out.update(rec.out)
    mg.close()
    ctx.close()


def hierarchy_3d(out):
    ctx = hip.Context(0)
    ctx.set_condense_min_bytes(0)                                 # every smoothed level condenses its star patches
    lv, tr = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)
    mg = hip.Multigrid(ctx, lv, tr, 3)
    rec = Recorder(ctx, [L.id for L in mg.levels])
    rec.out["3d/condensed levels"] = {"sha256": [], "events": {}, "comm": [0, 0, 0], "condensed": [bool(L.condensed()) for L in mg.levels[1:]]}
    cycles(rec, ctx, mg, lv, "3d")
    F = mg.levels[-1]
    smoother_cases(rec, ctx, F, "3d finest", 16)
    out.update(rec.out)
    mg.close()
    ctx.close()


def saddle(out):
    from alfi_amd.nssolver import HipNavierStokesSolver
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(4), 2, 2)
    _, info = s.solve(10.0)
    assert info["converged"]
    sad, ctx, n, nu = s.saddle, s.ctx, s.n_u + s.n_p, s.n_u
    rec = Recorder(ctx, [L.id for L in s.hmg.mg.levels])
    B = np.random.default_rng(21).standard_normal((n, 4))
    B[s.levels[-1].bc_dofs] = 0.0
    B[nu:] -= B[nu:].mean(axis=0)
    B[:, 1] = 1e-4 * B[:, 0]
    atol = 1e-7 * np.linalg.norm(B[:, 0])
    for restart in (3, 30):
        def single():
            out_ = []
            for c in range(3):
                db, dx = ctx.vec(B[:, c]), ctx.vec(n)
                its, rn = sad.solve(db, dx, 1e-6, atol, 200, restart)
                out_ += [dx.get(), np.array([its, rn], dtype=np.float64)]
            return out_

        def block(cols):
            def f():
                dB, dX = ctx.mat(B, ld=wide(n, 2)), ctx.mat(np.zeros((n, 4)), ld=wide(n, 2))
                its, rn = sad.solve_block(dB, dX, 1e-6, atol, 200, restart, cols=cols)
                return [dX.get(), np.array(list(its) + list(rn), dtype=np.float64)]
            return f
        rec.run("saddle/solve restart=%d" % restart, single)
        rec.run("saddle/solve_block cols=[2] restart=%d" % restart, block([2]))
        rec.run("saddle/solve_block 4 cols restart=%d" % restart, block([0, 1, 2, 3]))
    out.update(rec.out)
    s.close()


def partitioned(out):
    """one rank, forced partition: every partitioned branch runs (reductions through the ctx's buffer, exchange counters)"""
    from alfi_amd.dist import DistMultigrid, DistSaddle
    lv, tr = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=10.0)
    L = lv[-1]
    dmg = DistMultigrid(lv, tr, 2, solo=(0, 1), min_dofs=1, force_distributed=True)
    Bm, vol = build_pressure_coupling(L)
    sad = DistSaddle(dmg, Bm, vol, L.V.cell_nodes, L.nu, L.gamma, remove_constant_nullspace=True)
    ctx = sad.sad.ctx
    rec = Recorder(ctx, [l.id for l in dmg.mg.levels])
    b = np.random.default_rng(5).standard_normal(L.n)
    b[L.bc_dofs] = 0.0

    def cyc(kind):
        def f():
            db, dx = dmg.local_vec(b), dmg.local_vec()
            (dmg.vcycle if kind == "v" else dmg.fcycle)(db, dx)
            return [dx.get()]
        return f

    def smooth(k, guess):
        def f():
            db, dx = dmg.local_vec(b), dmg.local_vec(0.5 * b)
            dmg.mg.levels[-1].smooth(k, db, dx, nonzero_guess=guess)
            return [dx.get()]
        return f
    rec.run("partitioned/vcycle", cyc("v"))
    rec.run("partitioned/fcycle", cyc("f"))
    for k in (2, 16):
        for guess in (False, True):
            rec.run("partitioned/smooth k=%d guess=%d" % (k, guess), smooth(k, guess))

    def solve():
        rhs = np.random.default_rng(9).standard_normal(sad.n)
        x, its, rn = sad.solve(rhs, rtol=1e-6, atol=1e-12, max_it=40, restart=3)
        return [x, np.array([its, rn], dtype=np.float64)]
    rec.run("partitioned/saddle solve restart=3", solve)
    out.update(rec.out)
    sad.close()
    dmg.close()


def two_rank_worker(overlap, outdir):
    """one of two ranks sharing the GPU, native transport over tests/mock_rccl: the three-level 2-D hierarchy, every level
    partitioned; the rank's owned results, events and communication counters of smoother calls and cycles"""
    import torch
    import torch.distributed as dist
    from alfi_amd.dist import DistMultigrid
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    lv, tr = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 2, 2, Re=100.0)
    dmg = DistMultigrid(lv, tr, 3, robust_restriction=False, min_dofs=1)
    assert dmg.transport == "rccl", dmg.transport
    ctx = dmg.ctx
    rec = Recorder(ctx, [l.id for l in dmg.levels])
    b = np.random.default_rng(5).standard_normal(lv[-1].n)
    b[lv[-1].bc_dofs] = 0.0

    def cyc(kind):
        def f():
            db, dx = dmg.local_vec(b), dmg.local_vec()
            (dmg.vcycle if kind == "v" else dmg.fcycle)(db, dx)
            return [dmg.owned(dx)]
        return f

    def smooth(k, guess):
        def f():
            db, dx = dmg.local_vec(b), dmg.local_vec(0.5 * b)
            with torch.cuda.stream(dmg.stream):
                dmg._in_cycle = True
                try:
                    dmg.levels[-1].smooth(k, db, dx, nonzero_guess=guess)
                finally:
                    dmg._in_cycle = False
            return [dmg.owned(dx)]
        return f
    tag = "two ranks overlap=%s rank %d" % (overlap, rank)
    rec.out[tag + "/set-up"] = {"levels": len(dmg.levels), "overlap_levels": [int(l) for l in dmg.overlap_levels]}
    for k in (3, 16):
        for guess in (False, True):
            rec.run("%s/smooth k=%d guess=%d" % (tag, k, guess), smooth(k, guess))
    rec.run(tag + "/vcycle", cyc("v"))
    rec.run(tag + "/fcycle", cyc("f"))
    with open(os.path.join(outdir, "rank%d.json" % rank), "w") as f:
        json.dump(rec.out, f)
    dmg.close()
    dist.barrier()
    dist.destroy_process_group()


def two_ranks(out):
    """the sum exchange after the patch solves hands the ghost values to the product (overlap 0: 2 k exchanges per smoother
    call); with overlap 1 the exchanges hide behind interior work (3 k)"""
    import socket
    import subprocess
    import tempfile
    from tests.mock_rccl.build import build
    lib = build()
    for overlap in ("0", "1"):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        with tempfile.TemporaryDirectory() as tmp:
            procs = []
            for r in range(2):
                env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                           MASTER_PORT=str(port), OMP_NUM_THREADS="4", ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=lib,
                           ALFI_DIST_OVERLAP=overlap, ALFI_DIST_OVERLAP_MIN_DOFS="0")
                procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--two-rank-worker", overlap, tmp],
                                              env=env, cwd=ROOT, stdout=sys.stderr))
            try:
                for p in procs:
                    if p.wait(timeout=200) != 0:
                        raise RuntimeError("a rank of the two-rank case failed")
            finally:                                   # (a rank that failed leaves its peer waiting in a collective)
                for p in procs:
                    if p.poll() is None:
                        p.kill()
            for r in range(2):
                with open(os.path.join(tmp, "rank%d.json" % r)) as f:
                    out.update(json.load(f))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--two-rank-worker":
        return two_rank_worker(sys.argv[2], sys.argv[3])
    out = {}
    for part in (banded, hierarchy_2d, hierarchy_3d, saddle, partitioned, two_ranks):
        part(out)
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
