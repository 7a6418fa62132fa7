"""Storage of the dense patch inverses, three ways on one bench configuration in ONE process: FP64 with the library's default
policy (levels of 1 GiB and more condense their vertex stars), FP64 dense on every level, and FP32 (patch_factor_dtype="f32").
The hierarchy is generated once, set up once per mode, and the modes are timed alternately, round after round.

usage: python scripts/factor_dtype_time.py cfg4 [--rounds 3] [--cycles 10] [--out FILE]

Per mode: ms per V(k,k) cycle (every round, and the spread over the rounds), device time of the PATCH_APPLY events per level of
one instrumented cycle, factor bytes and storage per level, stored bytes / time of the finest level's apply, wall time of the
finest level's alfi_patches_factor (gather, inversion, probe; FP32: the conversion too), device memory in use after set-up
(FP32: the ctx's FP64 work buffer included, so this is that mode's peak) and the relative residual after the timed cycles."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

MODES = [("f64-default", None, None), ("f64-dense", -1, None), ("f32", None, "f32")]


def used_bytes():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cfg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from alfi_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("factor_dtype_time.py measures on the GPU; none is visible")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    t0 = time.time()
    lv, tr, k = bench.build_problem(args.cfg, False)
    fine = lv[-1]
    say("%s: %s" % (args.cfg, bench.describe(args.cfg)))
    say("hierarchy generated on the host in %.1f s; patches per level %s, largest patch %d dofs"
        % (time.time() - t0, [len(L.patch_ptr) - 1 for L in lv[1:]], int(np.diff(fine.patch_ptr).max())))
    b = np.random.default_rng(0).standard_normal(fine.n)
    b[fine.bc_dofs] = 0.0
    runs = {}
    base = used_bytes()
    for name, threshold, dtype in MODES:
        ctx = hip.Context(0)
        if threshold is not None:
            ctx.set_condense_min_bytes(threshold)
        before = used_bytes()
        t0 = time.time()
        mg = hip.Multigrid(ctx, lv, tr, k, patch_factor_dtype=dtype)
        ctx.sync()
        setup = time.time() - t0
        mem = used_bytes() - before
        top = mg.levels[-1]
        fac = []
        for _ in range(3):
            ctx.sync()
            t0 = time.time()
            top.factor()
            ctx.sync()
            fac.append(1e3 * (time.time() - t0))
        runs[name] = dict(ctx=ctx, mg=mg, db=ctx.vec(b), dx=ctx.vec(fine.n), ms=[], setup=setup, mem=mem, fac=fac,
                          storage=[(d.patch_storage_dtype(), d.condensed(), d.factor_bytes()) for d in mg.levels[1:]],
                          probe=[d.patch_check() for d in mg.levels[1:]])
        say("%-12s set up in %.1f s, device memory +%.2f GB; storage per level %s"
            % (name, setup, mem / 1e9, ["%s/mode %d/%.3f GB" % (a, m, fb / 1e9) for a, m, fb in runs[name]["storage"]]))
    for r in runs.values():                                   # warm-up: every shape the timed window uses
        for _ in range(3):
            r["mg"].vcycle(r["db"], r["dx"])
        r["ctx"].sync()
    for _ in range(args.rounds):
        for name, _, _ in MODES:
            r = runs[name]
            r["ctx"].sync()
            t0 = time.time()
            for _ in range(args.cycles):
                r["mg"].vcycle(r["db"], r["dx"])
            r["ctx"].sync()
            r["ms"].append(1e3 * (time.time() - t0) / args.cycles)
    say()
    say("ms per V(%d,%d) cycle, %d rounds of %d cycles, the modes alternating:" % (k, k, args.rounds, args.cycles))
    for name, _, _ in MODES:
        ms = runs[name]["ms"]
        say("  %-12s %s   best %.3f  spread %.3f" % (name, "  ".join("%8.3f" % m for m in ms), min(ms), max(ms) - min(ms)))
    say()
    say("one instrumented cycle: PATCH_APPLY device time per level (ms, launches), factor bytes, stored bytes / apply time:")
    for name, _, _ in MODES:
        r = runs[name]
        ctx, mg = r["ctx"], r["mg"]
        ctx.prof_enable(2)
        ctx.prof_reset()
        mg.vcycle(r["db"], r["dx"])
        ctx.sync()
        for dl, (dt, mode, fb) in zip(mg.levels[1:], r["storage"]):
            ms, cnt = ctx.prof_get(dl.id)["PATCH_APPLY"]
            per = ms / max(cnt, 1)
            say("  %-12s level %d  %s mode %d  %8.3f GB  PATCH_APPLY %9.3f ms in %3d launches = %8.4f ms each  %6.3f TB/s"
                % (name, dl.id, dt, mode, fb / 1e9, ms, cnt, per, fb / (per * 1e-3) / 1e12 if per > 0 else 0.0))
        ctx.prof_enable(False)
        rr = ctx.vec(fine.n)
        mg.levels[-1].residual(r["db"], r["dx"], rr)
        res = np.linalg.norm(rr.get()) / np.linalg.norm(b)
        worst = max(p[0] for p in r["probe"])
        say("  %-12s finest level alfi_patches_factor %s ms; probe worst %.1e, flagged %d; relative residual after the cycles %.4e"
            % (name, " ".join("%.2f" % f for f in r["fac"]), worst, sum(p[1] for p in r["probe"]), res))
    say()
    say("device memory in use before any mode: %.2f GB" % (base / 1e9))
    for r in runs.values():
        r["mg"].close()
        r["ctx"].close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
