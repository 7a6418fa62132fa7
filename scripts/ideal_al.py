#!/usr/bin/env python3
"""The ideal augmented-Lagrangian check of the reference (examples/Makefile ``idealal``: iters.py --solver-type allu): the outer
FGMRES + Schur-full solve with fieldsplit_0 an EXACT solve of the augmented velocity block A + gamma B^T M^-1 B (the library's
multifrontal factors of the finest operator, re-factored every Newton step), so the only approximation left is DGMassInv's
Schur complement -(nu + gamma) M_p^-1.  ldc2d, baseN 16, nref 2, [P2]^2-P0 with SUPG, gamma in {0, 1, 10, 1e2, 1e3, 1e4},
Reynolds continuation of iters.py (1, 10, 100, then 200, 300, ... up to --re-max).

Prints the gamma x Re table of average outer iterations per Newton step at Re 10 / 100 / 1000 / 5000 / 10000 and the factor /
solve seconds.  A gamma whose continuation fails (no convergence, or an error such as a factorisation that fails its residual
probe) is marked from that Reynolds number on and the table goes on -- the reference's lines end in ``|| 1``.

  python scripts/ideal_al.py [--gammas 0,1,10,100,1000,10000] [--re-max 10000] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alfi_amd.problem import TwoDimLidDrivenCavityProblem
from alfi_amd.nssolver import HipNavierStokesSolver

FAILED = "div"


def continuation(re_max):
    """iters.py: [1, 10, 100] + range(200, 10000 + 100, 100), cut at re_max."""
    return [r for r in [1, 10, 100] + list(range(200, 10000 + 100, 100)) if r <= re_max]


def run_gamma(args, gamma, res):
    out = {"gamma": gamma, "its": {}, "newton": {}, "failed_at": None, "error": None}
    t0 = time.time()
    s = HipNavierStokesSolver(TwoDimLidDrivenCavityProblem(args.baseN), args.nref, args.k, gamma=gamma,
                              stabilisation_type=args.stabilisation_type, smoothing=6, restriction=True, solver_type="allu")
    out["setup_s"] = time.time() - t0
    out["dofs"] = s.n_u + s.n_p
    for re in res:
        try:
            _, info = s.solve(float(re))
        except Exception as e:          # noqa: BLE001 -- reported in the table, the other gammas go on
            out["failed_at"], out["error"] = re, "%s: %s" % (type(e).__name__, e)
            break
        out["its"][re] = info["linear_iter"] / max(1, info["nonlinear_iter"])
        out["newton"][re] = info["nonlinear_iter"]
        if not info["converged"]:
            out["failed_at"], out["error"] = re, "Newton did not converge (%d steps)" % info["nonlinear_iter"]
            break
        if re in (10, 100, 1000, 5000, 10000):
            print("  gamma %-6g Re %-6d outer its / Newton step %.2f  (%d Newton steps)"
                  % (gamma, re, out["its"][re], info["nonlinear_iter"]), flush=True)
    t = s.timings
    out.update(factor_s=t["factor_s"], solve_s=t["solve_s"], assemble_s=t["assemble_s"], residual_s=t["residual_s"],
               newton_steps=t["newton_steps"], total_s=time.time() - t0)
    if getattr(s, "direct_residual", None) is not None:
        out["factor_bytes"], out["last_probe"] = s.saddle.velocity_info()
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseN", type=int, default=16)
    ap.add_argument("--nref", type=int, default=2)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--gammas", default="0,1,10,100,1000,10000")
    ap.add_argument("--re-max", type=int, default=10000)
    ap.add_argument("--stabilisation-type", default="supg", choices=["none", "supg"])
    ap.add_argument("--json", default=None, help="write the results here as well")
    args = ap.parse_args()
    gammas = [float(g) for g in args.gammas.split(",")]
    res = continuation(args.re_max)
    tableres = [r for r in (10, 100, 1000, 5000, 10000) if r <= max(res)]
    rows = []
    for g in gammas:
        print("[ideal_al] gamma %g: continuation over %d Reynolds numbers" % (g, len(res)), flush=True)
        r = run_gamma(args, g, res)
        if r["failed_at"] is not None:
            print("[ideal_al] gamma %g stopped at Re %d: %s" % (g, r["failed_at"], r["error"]), flush=True)
        rows.append(r)
    dofs = rows[0]["dofs"] if rows else 0
    print("\nldc2d baseN %d nref %d k %d, %s, solver_type allu, %d dofs" % (args.baseN, args.nref, args.k,
                                                                           args.stabilisation_type, dofs))
    print("gamma\t" + "\t".join("Re=%d" % r for r in tableres) + "\t(average outer iterations per Newton step; %s: the "
          "continuation failed at or before this Re)" % FAILED)
    for r in rows:
        cells = []
        for re in tableres:
            ok = r["failed_at"] is None or re < r["failed_at"]
            cells.append("%.2f" % r["its"][re] if ok and re in r["its"] else FAILED)
        print("%g\t" % r["gamma"] + "\t".join(cells))
    print("gamma\tNewton steps\tfactor s\tsolve s\trefresh s\tresidual s\tfactor s / step\tfactor MB")
    for r in rows:
        n = max(1, r["newton_steps"])
        print("%g\t%d\t\t%.2f\t\t%.2f\t%.2f\t\t%.2f\t\t%.4f\t\t%s" % (
            r["gamma"], r["newton_steps"], r["factor_s"], r["solve_s"], r["assemble_s"], r["residual_s"], r["factor_s"] / n,
            "%.1f" % (r["factor_bytes"] / 1e6) if "factor_bytes" in r else "-"))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"args": vars(args), "rows": rows}, f, indent=1, default=str)


if __name__ == "__main__":
    main()
