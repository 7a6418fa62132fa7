"""Storage of dense macro-star inverses on Burman levels, FP64 against FP32 (macro_factor_dtype="f32"), on one
Burman-stabilised Scott-Vogelius configuration in ONE process.  Each mode sets up its own solver (the hierarchy is generated
per solver: the generation is not what is measured), refreshes its operators at the same state, and the modes are then timed
ALTERNATELY, round after round.

usage: python scripts/macro_f32_time.py CASE [--rounds 3] [--cycles 10] [--out FILE]
  CASE  bfs3d     the config-5-like channel of scripts/burman_time.py --bfs3d --nref 1 ([P3]^3 macro stars: big_apply kernels;
                  --nref 2: config 5's own two smoothed levels)
        cubic2d   the 2-D cubic pair [P3]^2-P2dg, baseN 10, nref 4 (macro stars of <= 146 dofs: the vertex-star kernels)
        ldc3d     3-D [P3]^3 lid-driven cavity, --baseN, nref 1 (macro stars of <= 1599 dofs, a small stand-in for bfs3d)

Per mode: ms per V-cycle (every round and the spread over the rounds), device time of the PATCH_APPLY events per level of one
instrumented cycle and stored bytes / time, wall time of the finest level's alfi_patches_factor (FP32: the ranges, probes and the
conversion included), device memory the mode added, the residual probe's figures and the relative residual after the timed
cycles.  The yardstick of the FP32 apply is the FP64 apply of the same level in the same job."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

MODES = [("f64-dense", None), ("f32", "f32")]


def used_bytes():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def make_solver(args, dtype):
    from alfi_amd import problem as P
    from alfi_amd.nssolver import HipNavierStokesSolver
    if args.case == "bfs3d":
        prob, nref, k = P.ThreeDimBackwardsFacingStepProblem(1, msh=args.mesh), args.nref, 3
    elif args.case == "cubic2d":
        prob, nref, k = P.TwoDimLidDrivenCavityProblem(10), 4, 3
    else:
        prob, nref, k = P.ThreeDimLidDrivenCavityProblem(args.baseN), 1, 3
    return HipNavierStokesSolver(prob, nref, k, discretisation="sv", stabilisation_type="burman",
                                 stabilisation_weight=args.weight, macro_factor_dtype=dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["bfs3d", "cubic2d", "ldc3d"])
    ap.add_argument("--mesh", default=None)
    ap.add_argument("--nref", type=int, default=1, help="bfs3d: refinements (2: the 1765 + 303 macro stars of config 5)")
    ap.add_argument("--baseN", type=int, default=2)
    ap.add_argument("--re", type=float, default=100.0)
    ap.add_argument("--weight", type=float, default=5e-3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("macro_f32_time.py measures on the GPU; none is visible")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    runs = {}
    base = used_bytes()
    for name, dtype in MODES:
        before = used_bytes()
        t0 = time.time()
        s = make_solver(args, dtype)
        setup = time.time() - t0
        ctx, mgl = s.ctx, s.hmg.mg.levels
        s.nu = s.char_L * s.char_U / args.re
        u = np.zeros(s.n_u)
        x = s.levels[-1].V.node_coords
        u.reshape(-1, s.problem.dim)[:, 0] = np.sin(np.pi * x[:, 0]) * np.sin(np.pi * x[:, 1])
        u[s.levels[-1].bc_dofs] = 0.0
        s._device_states(u)
        for dl, st in zip(mgl, s._dstate):                      # the Burman refresh of a Newton step, at the same state
            dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True)
        s._factor_levels()
        ctx.sync()
        mem = used_bytes() - before
        top, fac = mgl[-1], []
        for _ in range(3):
            ctx.sync()
            t0 = time.time()
            top.factor()
            ctx.sync()
            fac.append(1e3 * (time.time() - t0))
        if not runs:
            fine = s.levels[-1]
            sizes = [np.diff(L.patch_ptr) for L in s.levels[1:]]
            say("%s: Burman-stabilised [P3]^%d Scott-Vogelius, weight %g, Re %g; dofs per level %s, patches %s, largest patch %s dofs"
                % (args.case, s.problem.dim, args.weight, args.re, [L.n for L in s.levels], [len(z) for z in sizes],
                   [int(z.max()) for z in sizes]))
            b = np.random.default_rng(0).standard_normal(fine.n)
            b[fine.bc_dofs] = 0.0
        runs[name] = dict(s=s, ctx=ctx, mg=s.hmg.mg, db=ctx.vec(b), dx=ctx.vec(len(b)), ms=[], mem=mem, fac=fac,
                          work=ctx.f32_work_bytes(),
                          storage=[(d.patch_storage_dtype(), d.condensed(), d.factor_bytes()) for d in mgl[1:]],
                          probe=[d.patch_check() for d in mgl[1:]])
        say("%-10s set up in %.1f s (host generation included), device memory +%.2f GB (of it the ctx's FP64 work buffer %.3f GB); "
            "storage per level %s" % (name, setup, mem / 1e9, runs[name]["work"] / 1e9,
                                      ["%s/mode %d/%.3f GB" % (a, m, fb / 1e9) for a, m, fb in runs[name]["storage"]]))
    for r in runs.values():                                   # warm-up: every shape the timed window uses
        for _ in range(3):
            r["mg"].vcycle(r["db"], r["dx"])
        r["ctx"].sync()
    for _ in range(args.rounds):
        for name, _ in MODES:
            r = runs[name]
            r["ctx"].sync()
            t0 = time.time()
            for _ in range(args.cycles):
                r["mg"].vcycle(r["db"], r["dx"])
            r["ctx"].sync()
            r["ms"].append(1e3 * (time.time() - t0) / args.cycles)
    say()
    say("ms per V-cycle, %d rounds of %d cycles, the modes alternating:" % (args.rounds, args.cycles))
    for name, _ in MODES:
        ms = runs[name]["ms"]
        say("  %-10s %s   best %.3f  spread %.3f" % (name, "  ".join("%8.3f" % m for m in ms), min(ms), max(ms) - min(ms)))
    say()
    say("instrumented cycles (%d, the modes alternating): PATCH_APPLY device time per level and launch, factor bytes, stored bytes / "
        "apply time:" % args.rounds)
    per_launch = {name: {} for name, _ in MODES}
    for _ in range(args.rounds):
        for name, _ in MODES:
            r = runs[name]
            ctx, mg = r["ctx"], r["mg"]
            ctx.prof_enable(2)
            ctx.prof_reset()
            mg.vcycle(r["db"], r["dx"])
            ctx.sync()
            for dl in mg.levels[1:]:
                ms, cnt = ctx.prof_get(dl.id)["PATCH_APPLY"]
                per_launch[name].setdefault(dl.id, []).append((ms / max(cnt, 1), cnt))
            ctx.prof_enable(False)
    for name, _ in MODES:
        r = runs[name]
        for dl, (dt, mode, fb) in zip(r["mg"].levels[1:], r["storage"]):
            per = [p for p, _ in per_launch[name][dl.id]]
            best = min(per)
            say("  %-10s level %d  %s mode %d  %8.3f GB  PATCH_APPLY %s ms per launch (%d launches a cycle)  best %8.4f  spread %.4f  "
                "%6.3f TB/s" % (name, dl.id, dt, mode, fb / 1e9, " ".join("%8.4f" % p for p in per), per_launch[name][dl.id][0][1],
                                best, max(per) - min(per), fb / (best * 1e-3) / 1e12 if best > 0 else 0.0))
    say()
    for name, _ in MODES:
        r = runs[name]
        rr = r["ctx"].vec(len(b))
        r["mg"].levels[-1].residual(r["db"], r["dx"], rr)
        res = np.linalg.norm(rr.get()) / np.linalg.norm(b)
        say("  %-10s finest level alfi_patches_factor %s ms; probe (worst, flagged, repaired, worst after) per level %s; relative "
            "residual after the cycles %.4e" % (name, " ".join("%.2f" % f for f in r["fac"]),
                                                ["%.1e/%d/%d/%.1e" % p for p in r["probe"]], res))
    say()
    say("device memory in use before any mode: %.2f GB" % (base / 1e9))
    for r in runs.values():
        r["s"].close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
