#!/usr/bin/env python3
"""The partition of a bench configuration over N ranks, computed on the HOST (no GPU): what every rank would own, hold as
ghosts, whom it would exchange with and how many bytes per exchange -- the plan `bench.py --gpus N` executes.

    python scripts/partition_report.py cfg4 --world 8 > profiles/r03_partition_plan_cfg4_8ranks.json

Per rank and smoothed level also what the rank would STORE for its patches: every rank decides for itself at its first
factorisation (alfi_patches_factor) -- dense inverses below --condense-min-bytes of rank-local dense bytes (default: the library's
1 GiB, csrc/env.h), else the groups the finder (csrc/find_groups.h) sees in the rank's localised sparsity and the condensed factors
the planner (csrc/patch_plan.h) lays out for them; both run here on the host through libalfi_host.so.  Levels with generator
groups or facet coupling are reported as the device path treats them (mode 1 / dense).

(Eight processes cannot share the one GPU of the build box -- the pool allows six -- so the 8-way split of the full-size
configuration is recorded from the partitioner itself; the 4- and 6-rank runs through tests/mock_rccl execute the same code.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def patch_storage(L, part, min_bytes, dtype=None):
    """(mode, factor bytes, dense bytes, dtype) of the rank ``part`` on level ``L``: the decision of alfi_patches_factor on the
    host.  dtype "f32": the rank asked for single-precision storage (alfi_patches_set_storage); a level that has an FP32 form --
    its largest patch has 33 .. 160 dofs, no generator groups, no facet coupling -- stores floats and does not condense."""
    import copy
    from alfi_amd import _hostlib, dist as D, env
    from alfi_amd.problem import BSR
    Ls = copy.copy(L)
    Ls.A = BSR(L.A.nbrows, L.A.nbcols, L.bs, L.A.rowptr, L.A.colidx, None)           # the sparsity is all this needs
    LL = D.localize_level(Ls, part)
    n = np.diff(LL.patch_ptr)
    dense = int(8 * ((n * ((n + 1) & ~1) + 15) & ~15).sum())
    groups, mode = getattr(LL, "patch_groups", None), 1
    if (dtype == "f32" and len(n) and 32 < n.max() <= 160 and not getattr(L, "facet_coupling", False)
            and (groups is None or not env.condense())):
        return 0, int(4 * _hostlib.plan_f32_layout(LL.patch_ptr)["inv32_floats"]), dense, "f32"
    if not env.condense() or getattr(L, "facet_coupling", False) or len(n) == 0:
        return 0, dense, dense, "f64"
    if groups is None:
        if min_bytes < 0 or dense < min_bytes:
            return 0, dense, dense, "f64"
        groups, mode = _hostlib.find_groups(LL.bs, LL.A.rowptr, LL.A.colidx, LL.patch_ptr, LL.patch_dofs), 2
        if not (groups >= 0).any():
            return 0, dense, dense, "f64"
    plan = _hostlib.plan_condensed(LL.bs, LL.A.rowptr, LL.A.colidx, LL.patch_ptr, LL.patch_dofs, groups)
    return mode, int(8 * (plan["mat_doubles"] + plan["sinv_doubles"])), dense, "f64"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--min-dofs", type=int, default=400000)
    ap.add_argument("--condense-min-bytes", type=int, default=1 << 30, help="rank-local dense bytes from which a level condenses "
                    "its vertex-star factors itself (default: the library's)")
    ap.add_argument("--patch-factor-dtype", choices=["f32"], default=None, help="the ranks ask their levels for single-precision "
                    "storage of the dense patch inverses (patch_factor_dtype of DistMultigrid)")
    args = ap.parse_args()
    import bench
    from alfi_amd import dist as D
    t0 = time.time()
    lv, tr, k = bench.build_problem(args.config, False, lazy=bench.CONFIGS[args.config][0] != "sv")
    t_gen = time.time() - t0
    world = args.world
    splits = D.choose_splits(lv, world, args.min_dofs)
    t0 = time.time()
    ghosts = [[D.compute_ghosts(lv, tr, splits, l, r) for r in range(world)] for l in range(len(lv))]
    t_ghost = time.time() - t0
    levels = []
    for l, L in enumerate(lv):
        s = splits[l]
        distributed = bool(np.count_nonzero(np.diff(s)) > 1)
        row = {"level": l, "dofs": int(L.n), "distributed": distributed}
        if not distributed:
            row["owner"] = 0
            levels.append(row)
            continue
        bs = L.bs
        per = []
        for r in range(world):
            g = ghosts[l][r]
            owner = np.searchsorted(s, g, side="right") - 1
            recv = np.bincount(owner, minlength=world)
            # what r sends to q = q's ghosts owned by r
            send = np.array([np.count_nonzero((ghosts[l][q] >= s[r]) & (ghosts[l][q] < s[r + 1])) if q != r else 0
                             for q in range(world)])
            nbr = np.flatnonzero((recv > 0) | (send > 0))
            lo, hi = int(s[r]), int(s[r + 1])
            npatch = int(len(D.owned_patches(L, lo, hi))) if l > 0 else 0
            store = {}
            if npatch > 0:
                mode, fbytes, dense, dtype = patch_storage(L, D.LevelPart(l, bs, s, r, g), args.condense_min_bytes,
                                                           args.patch_factor_dtype)
                store = {"patch_storage_mode": mode, "patch_factor_dtype": dtype, "patch_factor_GB": round(fbytes / 1e9, 3),
                         "dense_inverse_GB": round(dense / 1e9, 3)}
            per.append({"rank": r, "owned_dofs": int((hi - lo) * bs), "ghost_dofs": int(len(g) * bs), **store,
                        "ghost_fraction": round(len(g) / max(hi - lo, 1), 4), "patches": npatch,
                        "neighbours": [int(q) for q in nbr], "n_neighbours": int(len(nbr)),
                        "forward_halo_KB_sent": round(8e-3 * bs * int(send.sum()), 1),
                        "forward_halo_KB_received": round(8e-3 * bs * int(recv.sum()), 1),
                        "largest_message_KB": round(8e-3 * bs * int(max(send.max(), recv.max())), 1)})
        row["ranks"] = per
        row["neighbours_max"] = max(p["n_neighbours"] for p in per)
        row["owned_dofs_min_max"] = [min(p["owned_dofs"] for p in per), max(p["owned_dofs"] for p in per)]
        row["ghost_fraction_max"] = max(p["ghost_fraction"] for p in per)
        if l > 0:
            row["patch_storage_modes"] = [p.get("patch_storage_mode") for p in per]
            row["patch_factor_dtypes"] = [p.get("patch_factor_dtype") for p in per]
            row["patch_factor_GB_total"] = round(sum(p.get("patch_factor_GB", 0.0) for p in per), 3)
        levels.append(row)
    out = {"config": args.config, "workload": bench.describe(args.config), "world": world, "min_dofs": args.min_dofs,
           "host_generation_s": round(t_gen, 1), "ghost_lists_all_ranks_s": round(t_ghost, 1),
           "neighbours_max": max([lv_["neighbours_max"] for lv_ in levels if lv_["distributed"]] + [0]),
           "single_owner_levels": [lv_["level"] for lv_ in levels if not lv_["distributed"]],
           "single_owner_dofs": int(sum(lv_["dofs"] for lv_ in levels if not lv_["distributed"])),
           "levels": levels,
           "note": "exchange counts per V-cycle do not depend on the number of ranks (two distributed levels at config 4: 91 "
                   "halo exchanges + 44 all-reduces, profiles/r02_bench_dist4_native_transport_mock_sharedgpu_functional.json); "
                   "a forward halo exchange is one grouped ncclSend/ncclRecv with exactly the listed neighbours"}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
