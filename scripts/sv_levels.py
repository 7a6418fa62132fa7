#!/usr/bin/env python3
"""Per-level sizes of a Scott-Vogelius hierarchy on the synthetic lid-driven cavity -- dofs, macro-star patches (count, largest,
mean size), transfer block size, bytes of the patch factors (condensed where the level has no facet coupling, dense with
--burman) -- and the time of one V-cycle of hip.Multigrid on the finest level.

  python scripts/sv_levels.py --dim 2 --baseN 10 --k 3 --nref 4 --smoothing 6 --restriction [--burman]

The V-cycle time is a host clock around ``--steps`` cycles that end in a device synchronise, after ``--warmup`` cycles."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alfi_amd import hip
from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem
from alfi_amd.sv import build_sv_hierarchy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--baseN", type=int, default=10)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--nref", type=int, default=3)
    ap.add_argument("--re", type=float, default=100.0)
    ap.add_argument("--gamma", type=float, default=1e4)
    ap.add_argument("--smoothing", type=int, default=6)
    ap.add_argument("--restriction", action="store_true")
    ap.add_argument("--burman", action="store_true", help="facet-coupled level graphs: dense patch factors")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    prob = TwoDimLidDrivenCavityProblem(a.baseN) if a.dim == 2 else ThreeDimLidDrivenCavityProblem(a.baseN)
    t0 = time.time()
    lv, tr = build_sv_hierarchy(prob, a.nref, a.k, Re=a.re, gamma=a.gamma, facet_coupling=a.burman)
    t_gen = time.time() - t0
    ctx = hip.Context(0)
    mg = hip.Multigrid(ctx, lv, tr, a.smoothing, robust_restriction=a.restriction)
    print("[P%d]^%d Scott-Vogelius, baseN %d, nref %d, Re %g, gamma %g, %d smoothing steps%s; host generation %.1f s"
          % (a.k, a.dim, a.baseN, a.nref, a.re, a.gamma, a.smoothing, ", facet-coupled" if a.burman else "", t_gen))
    print("level\tdofs\tpatches\tlargest\tmean\tblock\tfactor bytes\tdense bytes")
    for l, L in enumerate(lv):
        if l == 0:
            print("0\t%d\t-\t-\t-\t-\t(coarse solve)\t-" % L.n)
            continue
        sz = np.diff(L.patch_ptr)
        print("%d\t%d\t%d\t%d\t%.1f\t%d\t%d\t%d" % (l, L.n, sz.size, sz.max(), sz.mean(), tr[l - 1].blk_dofs.shape[1],
                                                  mg.levels[l].factor_bytes(), 8 * int((sz.astype(np.int64) ** 2).sum())))
    L = lv[-1]
    b = np.random.default_rng(0).standard_normal(L.n)
    b[L.bc_dofs] = 0.0
    db, dx = ctx.vec(b), ctx.vec(L.n)
    for _ in range(a.warmup):
        mg.vcycle(db, dx)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        mg.vcycle(db, dx)
    ctx.sync()
    dt = (time.perf_counter() - t0) / a.steps
    print("V-cycle on the finest level: %.3f ms (%d cycles after %d warm-up cycles, one run)" % (dt * 1e3, a.steps, a.warmup))
    mg.close()
    ctx.close()


if __name__ == "__main__":
    main()
