"""A/B of the block form of the four-launch smoother iteration on levels that take a chunk in pieces (dense macro stars, condensed
factors) -- no bench configuration has such a level among those of the four-launch iteration, so the levels are the test
suite's: tests/block_big_cases.py D, A (width 4), B (3), C (2) and the 1458 condensed [P2+FB]^3 stars of
tests/test_gpu_block_rhs_condensed.py.  smooth_block(k) at ncol 1 .. 4, Context.set_block_fused on / off alternating, 3 rounds.  usage: timeout -k 10 300 python scripts/block_fused_pieces_time.py [--out FILE]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from alfi_amd import _hostlib, hip
from tests import block_big_cases as bc
from tests.block_cond_cases import repeat_patches

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def ab(ctx, name, dl, k, reps=20, rounds=3):
    rng = np.random.default_rng(1)
    n = dl.n
    B = {c: ctx.mat(rng.standard_normal((n, c))) for c in (1, 2, 3, 4)}
    X = {c: ctx.mat(n, c) for c in (1, 2, 3, 4)}
    say("%s: %d dofs, condensed %d, apply width %d, mode(%d) on %d" % (name, n, dl.condensed(), dl.patch_apply_block_width(), k,
                                                                       dl.smooth_block_mode(k)))

    def timed(c):
        ctx.sync()
        t0 = time.time()
        for _ in range(reps):
            dl.smooth_block(k, B[c], X[c], nonzero_guess=False)
        ctx.sync()
        return 1e3 * (time.time() - t0) / reps
    for on in (True, False):
        ctx.set_block_fused(on)
        for c in (1, 2, 3, 4):
            timed(c)
    res = {(c, on): [] for c in (1, 2, 3, 4) for on in (True, False)}
    for _ in range(rounds):
        for on in (True, False):
            ctx.set_block_fused(on)
            for c in (1, 2, 3, 4):
                res[(c, on)].append(timed(c))
    ctx.set_block_fused(True)
    for c in (1, 2, 3, 4):
        pairs = list(zip(res[(c, True)], res[(c, False)]))
        say("  ncol %d  on/off ms per call, every round: %s   best ratio %.3f  %s"
            % (c, " ".join("%.4f/%.4f" % p for p in pairs), min(res[(c, True)]) / min(res[(c, False)]),
               "" if c == 1 else "faster in every round" if all(a < b for a, b in pairs) else "NOT faster in every round"))


def main():
    ctx = hip.Context(0)
    for name in ("D", "A", "B", "C"):
        dl = hip.Level(ctx, bc.operator(), np.zeros(0, dtype=np.int32))
        dl.set_patches(*bc.patch_arrays(bc.LEVELS[name]))
        dl.set_patch_groups(None)
        dl.factor()
        ab(ctx, "macro stars %s %s" % (name, bc.LEVELS[name]), dl, 6)
        dl.close()
    ctx.close()
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    lv, tr = build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 2, 2, Re=1000.0)
    L = lv[2]
    g = _hostlib.find_groups(L.bs, L.A.rowptr, L.A.colidx, L.patch_ptr, L.patch_dofs)
    pp, pd, gg = repeat_patches(L.patch_ptr, L.patch_dofs, g, 2 * (len(L.patch_ptr) - 1))
    ctx = hip.Context(0)
    ctx.set_condense_min_bytes(0)
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    dl.set_patches(pp, pd)
    dl.factor()
    ab(ctx, "condensed [P2+FB]^3 stars, %d patches" % (len(pp) - 1), dl, 2)
    ab(ctx, "condensed [P2+FB]^3 stars, %d patches" % (len(pp) - 1), dl, 10)
    dl.close()
    ctx.close()
    if len(sys.argv) == 3 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
