#!/usr/bin/env python3
"""The cost of the Burman interior-penalty term (alfi/stabilisation.py:139-162) on a Scott-Vogelius hierarchy, per level:
the operator refresh without and with the facet pass, the facet pass alone (operator and residual), the patch factorisation
with PCPATCH's facet rule, the factor bytes (dense on Burman levels), and the V-cycle of the finest level -- against the same
hierarchy without Burman (condensed factors, cell graph).

  python scripts/burman_time.py [--dim 3] [--baseN 1] [--nref 1] [--k 3] [--weight 5e-3] [--reps 3]
  python scripts/burman_time.py --bfs3d [--mesh data/meshes/bfs3d_coarse60.msh] --nref 1      # config-5-like channel

Wall time around synchronised calls (the facet kernels are three launches per call)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t0 = time.time()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.time() - t0) / reps * 1e3


def run(args, burman):
    from alfi_amd.nssolver import HipNavierStokesSolver
    from alfi_amd import problem as P
    if args.bfs3d:
        prob = P.ThreeDimBackwardsFacingStepProblem(1, msh=args.mesh)
    elif args.dim == 2:
        prob = P.TwoDimLidDrivenCavityProblem(args.baseN)
    else:
        prob = P.ThreeDimLidDrivenCavityProblem(args.baseN)
    t0 = time.time()
    s = HipNavierStokesSolver(prob, args.nref, args.k, discretisation="sv", stabilisation_type="burman" if burman else None,
                              stabilisation_weight=args.weight)
    setup = time.time() - t0
    s.nu = s.char_L * s.char_U / args.re
    ctx = s.ctx
    u = np.zeros(s.n_u)
    x = s.levels[-1].V.node_coords
    u.reshape(-1, prob.dim)[:, 0] = np.sin(np.pi * x[:, 0]) * np.sin(np.pi * x[:, 1])
    u[s.levels[-1].bc_dofs] = 0.0
    s._device_states(u)
    rows = []
    for L, dl, st, obj in zip(s.levels, s.hmg.mg.levels, s._dstate, s.hmg.pc_objs):
        r = {"level": L.level, "dofs": L.n, "nnzb": int(L.A.colidx.shape[0])}
        r["refresh_ms"] = timed(ctx, lambda: dl.assemble(s.nu, s.gamma, 1.0, st, True), args.reps)
        if burman:
            r["refresh_burman_ms"] = timed(ctx, lambda: dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True),
                                           args.reps)
            r["facets"] = int(L.facets.nf)
            if L.level == len(s.levels) - 1:
                F = ctx.vec(L.n)
                r["residual_facet_pass_ms"] = timed(ctx, lambda: dl.burman(s.burman_weight, st, False, F), args.reps)
        if obj is not None:
            r["factor_ms"] = timed(ctx, dl.factor, 1)
            r["factor_GB"] = dl.factor_bytes() / 1e9 if hasattr(dl, "factor_bytes") else None
            r["condensed"] = bool(obj.condensed)
        rows.append(r)
    b, xv = ctx.vec(np.random.default_rng(0).standard_normal(s.n_u)), ctx.vec(s.n_u)
    vc = timed(ctx, lambda: s.hmg.mg.vcycle(b, xv), args.reps)
    s.close()
    return {"burman": burman, "setup_s": setup, "vcycle_ms": vc, "levels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--baseN", type=int, default=1)
    ap.add_argument("--nref", type=int, default=1)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--bfs3d", action="store_true")
    ap.add_argument("--mesh", default=None)
    ap.add_argument("--re", type=float, default=100.0)
    ap.add_argument("--weight", type=float, default=5e-3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import json
    for burman in (False, True):
        print(json.dumps(run(args, burman)), flush=True)


if __name__ == "__main__":
    main()
