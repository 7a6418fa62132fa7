"""Symmetrised multiplicative patch sweeps on condensed factors against the sweeps on dense inverses, on the finest level of
bench configurations (default cfg5 and cfg4), in one job:

  dense, persistent     alfi_patches_set_multiplicative, the whole apply as one launch of a resident grid (the default);
  dense, per wavefront  the same level with ALFI_MULT_PERSISTENT=0: one launch per dependency wavefront.  The switch is read once
                        per process, so this leg runs in a child process of this script, after the parent has released its levels;
  condensed             alfi_patches_set_multiplicative_condensed on the level's groups (the hierarchy's macro-cell groups, or
                        the ones the level finds itself): residual / front / sigma / back / update launches per wavefront.

The dense persistent and the condensed sweep are timed alternately, ROUNDS times REPS applies each, in the parent.  Reported: ms
per symmetrised apply (best and median of the rounds), wavefronts, launches per apply, factor bytes, and the relative difference of
the two results.  With --large CFG (default cfg5L) the condensed set-up of that configuration is tried too and its factor bytes
reported.
usage: python scripts/mult_condensed_time.py [cfg ...] [--large cfg5L | --no-large]"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
from alfi_amd import _hostlib, hip
from alfi_amd.relaxation import OrderedRelaxation, Options

ROUNDS, REPS = 3, 3


def finest(cfg):
    lv, _, _ = bench.build_problem(cfg, False)
    L = lv[-1]
    orl = OrderedRelaxation()
    orl.name = "Star"
    orl.opts = Options("", {"pc_patch_construction_Star_sort_order": "0+:1-"})   # the problems' relaxation_direction
    return L, np.asarray(orl.iteration_order(L.V.mesh.coords[L.patch_seeds]), dtype=np.int64)


def level(ctx, L, groups):
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(L.patch_ptr, L.patch_dofs)
    dl.set_patch_groups(groups)
    dl.factor()
    return dl


def timed(ctx, dl, dx, dy, reps):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        dl.patch_apply(dx, dy)
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def rhs(L):
    x = np.random.default_rng(5).standard_normal(L.n)
    x[L.bc_dofs] = 0.0
    return x


def groups_of(L):
    if getattr(L, "patch_groups", None) is not None:
        return np.asarray(L.patch_groups, dtype=np.int32), "macro-cell groups"
    return _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs), "groups found in the sparsity"


def condensed_launches(L, groups, iterset):
    """launches of one symmetrised apply on condensed factors, from the host plans of the same inputs"""
    cond = _hostlib.plan_condensed(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs, groups)
    sweep = _hostlib.plan_sweep(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs, iterset, True)
    sc = _hostlib.plan_sweep_condensed(L.bs, L.patch_ptr, L.patch_dofs, sweep, cond)
    per_wave = 2 + 2 * (np.diff(sc["wk_ptr"]) > 0) + (np.diff(sc["wc_ptr"]) > 0)      # residual, update; front, back; sigma
    return 2 * int(per_wave.sum())


def child(cfg):
    """the dense sweep with one launch per wavefront (ALFI_MULT_PERSISTENT=0 in this process's environment)"""
    assert os.environ.get("ALFI_MULT_PERSISTENT") == "0"
    L, iterset = finest(cfg)
    ctx = hip.Context(0)
    dl = level(ctx, L, None)
    nw = dl.set_multiplicative(iterset, True)
    dx, dy = ctx.vec(rhs(L)), ctx.vec(L.n)
    dl.patch_apply(dx, dy)
    ms = [timed(ctx, dl, dx, dy, REPS) for _ in range(ROUNDS)]
    y = dy.get()
    print("%s dense, per wavefront : %9.2f ms best, %9.2f median; %d launches per apply; checksum %.17g"
          % (cfg, min(ms), float(np.median(ms)), 2 * nw, float(np.abs(y).sum())), flush=True)
    dl.close()
    ctx.close()


def compare(cfg):
    L, iterset = finest(cfg)
    groups, what = groups_of(L)
    ctx = hip.Context(0)
    x = rhs(L)
    dx, dyd, dyc = ctx.vec(x), ctx.vec(L.n), ctx.vec(L.n)
    dl, cl = level(ctx, L, None), level(ctx, L, groups)
    nwd = dl.set_multiplicative(iterset, True)
    nwc = cl.set_multiplicative(iterset, True, condensed=True)
    assert nwd == nwc and cl.condensed() == 1 and dl.condensed() == 0
    sizes = np.diff(L.patch_ptr)
    print("%s finest level: %d dofs, %d patches of up to %d dofs, %s; %d wavefronts per sweep, %d positions"
          % (cfg, L.n, len(sizes), sizes.max(), what, nwc, len(iterset)), flush=True)
    dl.patch_apply(dx, dyd)
    cl.patch_apply(dx, dyc)
    td, tc = [], []
    for _ in range(ROUNDS):
        td.append(timed(ctx, dl, dx, dyd, REPS))
        tc.append(timed(ctx, cl, dx, dyc, REPS))
    yd, yc = dyd.get(), dyc.get()
    print("%s dense, persistent    : %9.2f ms best, %9.2f median; 1 launch per apply; factors %.3f GB; checksum %.17g"
          % (cfg, min(td), float(np.median(td)), dl.factor_bytes() / 1e9, float(np.abs(yd).sum())), flush=True)
    print("%s condensed            : %9.2f ms best, %9.2f median; %d launches per apply; factors %.3f GB"
          % (cfg, min(tc), float(np.median(tc)), condensed_launches(L, groups, iterset), cl.factor_bytes() / 1e9), flush=True)
    print("%s condensed against dense: largest difference %.3e of the largest entry; condensed / dense time %.3f"
          % (cfg, np.abs(yc - yd).max() / np.abs(yd).max(), min(tc) / min(td)), flush=True)
    dl.close()
    cl.close()
    ctx.close()
    env = dict(os.environ, ALFI_MULT_PERSISTENT="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cfg], env=env, check=True)


def large(cfg):
    t0 = time.perf_counter()
    L, iterset = finest(cfg)
    groups, what = groups_of(L)
    t_gen = time.perf_counter() - t0
    ctx = hip.Context(0)
    t0 = time.perf_counter()
    try:
        cl = level(ctx, L, groups)
        nw = cl.set_multiplicative(iterset, True, condensed=True)
        ctx.sync()
    except hip.AlfiHipError as e:
        print("%s: the condensed set-up failed: %s" % (cfg, e), flush=True)
        return
    t_setup = time.perf_counter() - t0
    sizes = np.diff(L.patch_ptr)
    dense = 8 * int(((sizes.astype(np.int64) + 1) // 2 * 2 * sizes).sum())
    print("%s finest level: %d dofs, %d patches of up to %d dofs, %s: condensed sweeps set up in %.1f s (host generation %.1f s); "
          "%d wavefronts per sweep; factors %.3f GB (dense inverses would be %.1f GB)"
          % (cfg, L.n, len(sizes), sizes.max(), what, t_setup, t_gen, nw, cl.factor_bytes() / 1e9, dense / 1e9), flush=True)
    dx, dy = ctx.vec(rhs(L)), ctx.vec(L.n)
    cl.patch_apply(dx, dy)
    ms = [timed(ctx, cl, dx, dy, REPS) for _ in range(ROUNDS)]
    print("%s condensed            : %9.2f ms best, %9.2f median; %d launches per apply"
          % (cfg, min(ms), float(np.median(ms)), condensed_launches(L, groups, iterset)), flush=True)
    cl.close()
    ctx.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        child(args[1])
        sys.exit(0)
    big = "cfg5L"
    if "--no-large" in args:
        args.remove("--no-large")
        big = None
    if "--large" in args:
        i = args.index("--large")
        big = args[i + 1]
        del args[i:i + 2]
    for cfg in args or ["cfg5", "cfg4"]:
        compare(cfg)
    if big:
        large(big)
