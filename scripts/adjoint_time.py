#!/usr/bin/env python3
"""Cost of an adjoint solve (alfi_amd.adjoint, alfi_level_transpose) at a bench configuration's size, against the forward
Newton step:  python scripts/adjoint_time.py cfg4 [--re 10 100 1000] [--stabilisation-type supg|gls] [--sv] [--host]

After every forward ``solve(re)`` one adjoint solve with J = int w . u (LoadFunctional, w = e_x) about the converged state.
Prints the refresh, transpose, factor and solve seconds of the adjoint, its Krylov iterations and those of the last Newton
step of the forward solve (same operator state, same tolerances).
--functionals K (default 1): K functionals J_i = int e_(i mod dim) (1 + i) . u as ONE list: one refresh, transpose and
factorisation and one block solve for the K adjoints; the iterations and residual norms are printed per functional.
--compare-block-kernels: that block solve twice more each with the batched kernels off and on (Context.set_block_kernels).
--compare-block-fused: that block solve three times each with the block form of the four-launch smoother iteration off and on
(Context.set_block_fused), alternating; a 2-D config (cfg1, cfg2) is where every level takes that form."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _ex(x):
    w = np.zeros_like(x)
    w[:, 0] = 1.0
    return w


def _axis(i):
    def w(x):
        out = np.zeros_like(x)
        out[:, i % x.shape[1]] = 1.0 + i
        return out
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--re", type=float, nargs="+", default=[10.0, 100.0, 1000.0])
    ap.add_argument("--stabilisation-type", choices=["none", "supg", "gls"], default="none")
    ap.add_argument("--stabilisation-weight", type=float, default=0.05)
    ap.add_argument("--sv", action="store_true", help="cfg5s (Scott-Vogelius) with Burman stabilisation instead of CONFIG")
    ap.add_argument("--burman-weight", type=float, default=5e-3)
    ap.add_argument("--functionals", type=int, default=1, help="K functionals given as one list (K = 1: the single path)")
    ap.add_argument("--compare-block-kernels", action="store_true",
                    help="with --functionals K > 1: the block solve again with the batched kernels off and on (same bits), solve seconds")
    ap.add_argument("--compare-block-fused", action="store_true",
                    help="with --functionals K > 1: the block solve again, three rounds, with the block fused smoother iteration off "
                         "and on (Context.set_block_fused; same bits), solve seconds")
    ap.add_argument("--host", action="store_true", help="host assembly (the transpose still runs on the device values)")
    args = ap.parse_args()
    from alfi_amd.adjoint import LoadFunctional
    from alfi_amd.nssolver import HipNavierStokesSolver
    from dist_newton_time import problem_and_options
    args.supg = args.stabilisation_weight if args.stabilisation_type == "supg" else None
    args.burman = None
    if args.sv:
        args.config, args.supg, args.burman = "cfg5s", None, args.burman_weight
    prob, nref, ke, kw = problem_and_options(args)
    if args.stabilisation_type == "gls" and not args.sv:
        kw.update(stabilisation_type="gls", stabilisation_weight=args.stabilisation_weight)
    t0 = time.time()
    s = HipNavierStokesSolver(prob, nref, ke, device_assembly=not args.host, **kw)
    label = "%s%s" % (args.config, "" if args.sv or args.stabilisation_type == "none" else " " + args.stabilisation_type)
    print("%s: %d velocity + %d pressure dofs, setup %.1f s, device assembly %s, levels nnzb %s"
          % (label, s.n_u, s.n_p, time.time() - t0, s.device_assembly, [dl.nnzb for dl in s.hmg.mg.levels]), flush=True)
    steps = []                                      # Krylov iterations of every forward Newton step
    solve_name = "_zsolve" if s.device_assembly else "_linear_solve"
    inner = getattr(s, solve_name)

    def recording(*a):
        r = inner(*a)
        steps.append(r[-2])
        return r
    setattr(s, solve_name, recording)
    if args.functionals < 1:
        raise SystemExit("--functionals must be >= 1")
    many = args.functionals > 1
    s.setup_adjoint([LoadFunctional(_axis(i)) for i in range(args.functionals)] if many else LoadFunctional(_ex))
    for re in args.re:
        del steps[:]
        t0 = time.time()
        _, info = s.solve(re)
        wall = time.time() - t0
        n = max(info["nonlinear_iter"], 1)
        a = s.solver_adjoint.solve()
        if many:
            print("Re %g: forward %d Newton steps, %d Krylov its (last step %s), converged %s, %.2f s per Newton step | "
                  "%d adjoints in one block solve: Krylov its %s, converged %s, |r| %s of |b| %s; refresh %.3f s, transpose %.4f s, "
                  "factor %.3f s (each once), solve %.3f s, total %.3f s"
                  % (re, info["nonlinear_iter"], info["linear_iter"], steps[-1] if steps else "-", info["converged"], wall / n,
                     args.functionals, a["linear_iter"], a["converged"], ["%.2e" % r for r in a["residual_norm"]],
                     ["%.2e" % b for b in a["rhs_norm"]], a["refresh_s"], a["transpose_s"], a["factor_s"], a["solve_s"],
                     60.0 * a["time"]), flush=True)
            if args.compare_block_kernels:          # off = every block call loops the single-vector call: what a list cost before
                for on in (False, True, False, True):
                    s.ctx.set_block_kernels(on)
                    r = s.solver_adjoint.solve()
                    print("    batched kernels %-3s: solve %.3f s, Krylov its %s" % ("on" if on else "off", r["solve_s"], r["linear_iter"]),
                          flush=True)
            if args.compare_block_fused:            # off = the levels of the four-launch iteration loop whole smoother calls
                k = s.hmg.mg.k
                print("    smoother modes of the levels (Level.smooth_block_mode(%d)): %s"
                      % (k, [dl.smooth_block_mode(k) for dl in s.hmg.mg.levels[1:]]), flush=True)
                for on in (False, True) * 3:
                    s.ctx.set_block_fused(on)
                    r = s.solver_adjoint.solve()
                    print("    block fused iteration %-3s: solve %.3f s, Krylov its %s" % ("on" if on else "off", r["solve_s"],
                                                                                         r["linear_iter"]), flush=True)
            continue
        print("Re %g: forward %d Newton steps, %d Krylov its (last step %s), converged %s, %.2f s per Newton step | "
              "adjoint %d Krylov its, converged %s, |r| %.2e of |b| %.2e; refresh %.3f s, transpose %.4f s, factor %.3f s, "
              "solve %.3f s, total %.3f s"
              % (re, info["nonlinear_iter"], info["linear_iter"], steps[-1] if steps else "-", info["converged"], wall / n,
                 a["linear_iter"], a["converged"], a["residual_norm"], a["rhs_norm"], a["refresh_s"], a["transpose_s"],
                 a["factor_s"], a["solve_s"], 60.0 * a["time"]), flush=True)
    # the transpose pass alone, every level, repeated (the operator returns to itself after an even number)
    mgl = s.hmg.mg.levels
    for dl in mgl:
        dl.transpose()
    s.ctx.sync()
    reps = 10
    t0 = time.time()
    for _ in range(reps):
        for dl in mgl:
            dl.transpose()
    s.ctx.sync()
    dt = (time.time() - t0) / reps
    bs = mgl[-1].bs
    alg = sum(2 * 8 * bs * bs * dl.nnzb for dl in mgl)
    print("transpose of all levels: %.3f ms, %.1f MB algorithmic (2 x 8 bs^2 nnzb), %.0f GB/s; finest level %d blocks"
          % (1e3 * dt, alg / 1e6, alg / dt / 1e9, mgl[-1].nnzb), flush=True)
    s.close()


if __name__ == "__main__":
    main()
