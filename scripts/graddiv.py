"""The reference's grad-div experiment (examples/graddiv/graddiv.py) on the GPU: 2 sym grad u : grad v + gamma div u div v =
(1, v) with homogeneous Dirichlet conditions, solved by CG (rtol 1e-8, at most 200 iterations) preconditioned by one W-cycle
with a Chebyshev(2) level smoother around patch solves or point Jacobi, with or without the Schoeberl transfer, for
gamma in {0, 1, 10, 1e2, 1e3, 1e4, 1e6, 1e8}.  Prints the reference's two table lines (">200": not converged) and the seconds
per CG iteration.

    python scripts/graddiv.py --dim 2 --baseN 4 --nref 2 --k 2 --discretisation pkp0 --smoother patch --transfer
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMMAS = [0, 1, 1e1, 1e2, 1e3, 1e4, 1e6, 1e8]


def hierarchy(args, gamma):
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem, build_hierarchy
    prob = TwoDimLidDrivenCavityProblem(args.baseN) if args.dim == 2 else ThreeDimLidDrivenCavityProblem(args.baseN)
    if args.discretisation == "sv":
        from alfi_amd.sv import build_sv_hierarchy
        return build_sv_hierarchy(prob, args.nref, args.k, Re=0, gamma=float(gamma), advect=False)
    return build_hierarchy(prob, args.nref, args.k, Re=0, gamma=float(gamma), advect=False)


def cycle_profile(ctx, cg, b):
    """Event table of ONE preconditioner application (a W-cycle) per level: launches and device milliseconds by class."""
    db, dx = ctx.vec(b), ctx.vec(b.shape[0])
    cg.mg.vcycle(db, dx)                    # warm
    ctx.sync()
    ctx.prof_enable(True)
    ctx.prof_reset()
    dx.zero()
    cg.mg.vcycle(db, dx)
    ctx.sync()
    lines = ["level  dofs  " + "  ".join("%14s" % e for e in ("PATCH_APPLY", "PATCH_SCATTER", "MATMULT", "BLAS1", "PROLONG",
                                                                 "RESTRICT", "COARSE"))]
    for l, L in enumerate(cg.mg.levels):
        ev = ctx.prof_get(L.id)
        lines.append("%5d %5d  " % (l, L.n) + "  ".join("%4d x %6.3f ms" % (ev[e][1], ev[e][0]) for e in
                                                       ("PATCH_APPLY", "PATCH_SCATTER", "MATMULT", "BLAS1", "PROLONG",
                                                        "RESTRICT", "COARSE")))
    ctx.prof_enable(False)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, required=True, choices=[2, 3])
    ap.add_argument("--baseN", type=int, default=4)
    ap.add_argument("--nref", type=int, default=1)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--discretisation", choices=["pkp0", "sv"], default="pkp0")
    ap.add_argument("--smoother", choices=["patch", "jacobi"], required=True)
    ap.add_argument("--patch", choices=["star", "macro"], default="star")
    ap.add_argument("--transfer", action="store_true", help="the Schoeberl transfer (otherwise the plain one)")
    ap.add_argument("--gammas", type=float, nargs="*", default=GAMMAS)
    ap.add_argument("--profile", action="store_true", help="also print the event table of one W-cycle at the last gamma")
    args = ap.parse_args()
    if args.discretisation == "sv" and args.smoother == "patch" and args.patch != "macro":
        print("note: the reference runs Scott-Vogelius with --patch macro", file=sys.stderr)

    from alfi_amd import hip
    from alfi_amd.solver import HipCG, graddiv_solver
    ctx = hip.Context(0)
    params = graddiv_solver(args.smoother, patch=args.patch)
    iters, secs, ndofs, prof = [">%d" % params["ksp_max_it"]] * len(args.gammas), [], 0, None
    for i, gamma in enumerate(args.gammas):
        lv, tr = hierarchy(args, gamma)
        L = lv[-1]
        ndofs = L.n
        b = np.ones(L.n)
        b[L.bc_dofs] = 0.0
        try:
            cg = HipCG(ctx, lv, tr, params, transfer=args.transfer)
        except hip.AlfiHipError as e:      # the reference's `except: break`: a set-up that fails ends the sweep
            print("gamma = %g: %s" % (gamma, e), file=sys.stderr)
            break
        cg.solve(b)                         # warm-up (workspace allocations, first launches)
        ctx.sync()
        t0 = time.perf_counter()
        _, its, rn = cg.solve(b)
        dt = time.perf_counter() - t0
        secs.append(dt / max(its, 1))
        if rn <= cg.rtol * np.linalg.norm(b):
            iters[i] = its
        if args.profile and i == len(args.gammas) - 1:
            prof = cycle_profile(ctx, cg, b)
        cg.close()

    def row(cells):      # the reference's LaTeX table row
        print("&" + "\t&\t".join(str(c) for c in cells) + "\\\\")
    row(["Ref", "dofs"] + ["%.0e" % g for g in args.gammas])
    row([args.nref, ndofs] + iters)
    print("seconds per CG iteration: " + "  ".join("%.2e" % s for s in secs))
    if prof:
        print("\n".join(prof))
    ctx.close()


if __name__ == "__main__":
    main()
