#!/usr/bin/env python3
"""Wall time of Newton steps with the operators refreshed ON THE DEVICE (alfi_level_assemble) against the host rediscretisation
+ re-upload, at a bench configuration's size:  python scripts/newton_step_time.py cfg4 [--host] [--re 10 100]

Prints per Reynolds number the Newton / Krylov counts and the split of the wall time into assembly, patch + coarse
factorisation, residual evaluation and linear solve (HipNavierStokesSolver.timings)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--host", action="store_true", help="host rediscretisation (the round-2 path)")
    ap.add_argument("--re", type=float, nargs="+", default=[10.0, 100.0])
    ap.add_argument("--supg", type=float, default=None, metavar="WEIGHT",
                    help="SUPG stabilisation with this weight (the reference's production runs: 0.05, generate_submission:18-20)")
    ap.add_argument("--burman", type=float, default=None, metavar="WEIGHT",
                    help="Burman stabilisation of the Scott-Vogelius configs (cfg5s, cfg5) with this weight")
    ap.add_argument("--gls", type=float, default=None, metavar="WEIGHT",
                    help="GLS stabilisation of the P0-pressure configs with this weight")
    ap.add_argument("--adjoint", action="store_true",
                    help="one adjoint solve after every forward solve (refresh / transpose / factor / solve seconds, Krylov "
                         "count), and at the end the all-levels refresh with the transposed switch on next to the forward one")
    args = ap.parse_args()
    from alfi_amd.nssolver import HipNavierStokesSolver
    from dist_newton_time import problem_and_options
    if args.gls is not None and (args.supg is not None or args.burman is not None):
        raise SystemExit("--gls excludes --supg and --burman")
    prob, nref, ke, kw = problem_and_options(args)
    if args.gls is not None:
        kw.update(stabilisation_type="gls", stabilisation_weight=args.gls)
    t0 = time.time()
    s = HipNavierStokesSolver(prob, nref, ke, device_assembly=not args.host, **kw)
    print("%s: %d velocity + %d pressure dofs, setup %.1f s, device assembly %s" % (args.config, s.n_u, s.n_p, time.time() - t0,
                                                                                  s.device_assembly), flush=True)
    for re in args.re:
        for kk in s.timings:
            s.timings[kk] = 0 if kk == "newton_steps" else 0.0
        t0 = time.time()
        _, info = s.solve(re)
        wall = time.time() - t0
        n = max(s.timings["newton_steps"], 1)
        print("Re %g: %d Newton steps, %d Krylov its, converged %s, wall %.2f s = %.2f s per Newton step "
              "(assemble %.3f, factor %.3f, residual %.3f, solve %.3f per step)"
              % (re, info["nonlinear_iter"], info["linear_iter"], info["converged"], wall, wall / n,
                 s.timings["assemble_s"] / n, s.timings["factor_s"] / n, s.timings["residual_s"] / n, s.timings["solve_s"] / n),
              flush=True)
        if args.adjoint:
            print(adjoint_line(re, s.solve_adjoint(adjoint_functional(s))[1]), flush=True)
    if args.adjoint and s.device_assembly:
        t_fwd, t_tr = transposed_refresh_time(s, [dl for dl, _, _ in s._device_levels()])
        print("refresh of all levels about the final state: forward %.3f ms, transposed %.3f ms, ratio %.3f"
              % (1e3 * t_fwd, 1e3 * t_tr, t_tr / t_fwd), flush=True)
    s.close()


def adjoint_functional(s):
    """A fixed linear functional of the velocity (the cost of an adjoint solve does not depend on which)."""
    import numpy as np
    from alfi_amd.adjoint import LinearFunctional
    return LinearFunctional(np.random.default_rng(0).standard_normal(s.n_u))


def adjoint_line(re, info):
    return ("Re %g adjoint: %d Krylov its, converged %s, refresh %.3f s, transpose %.3f s, factor %.3f s, solve %.3f s"
            % (re, info["linear_iter"], info["converged"], info["refresh_s"], info["transpose_s"], info["factor_s"], info["solve_s"]))


def transposed_refresh_time(s, levels, reps=5):
    """Seconds per refresh of all levels about the current state with the transposed switch off and on
    (alfi_level_set_assembly_transposed), alternating, the best of ``reps`` each; the forward operators are left in place."""
    _, adv = s._last_solve
    best = [float("inf"), float("inf")]
    s._refresh_device(None, adv)
    for _ in range(reps):
        for on in (0, 1):
            with s._on_stream():
                for dl in levels:
                    dl.set_assembly_transposed(bool(on))
            s.ctx.sync()
            t0 = time.time()
            s._refresh_device(None, adv)
            best[on] = min(best[on], time.time() - t0)
    with s._on_stream():
        for dl in levels:
            dl.set_assembly_transposed(False)
    s._refresh_device(None, adv)
    return best[0], best[1]


if __name__ == "__main__":
    main()
