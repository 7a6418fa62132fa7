"""Block right-hand sides against looping: time per block patch apply, per block product and per full cycle at 1, 2 and 4
columns, the batched kernels on and off (Context.set_block_kernels: off = the single-vector call per column, which is what a
caller paid before block calls existed), on one bench configuration with DENSE patch inverses -- or, --condensed, with the
default policy (config 4's two large levels and config 5's macro stars hold condensed factors) --, in ONE process.  The hierarchy
is set up once; the two modes alternate, round after round.

usage: timeout -k 10 900 python scripts/block_rhs_time.py cfg3 [--rounds 3] [--reps 20] [--cycles 3] [--dtype f32] [--out FILE]
       timeout -k 10 900 python scripts/block_rhs_time.py cfg4 --condensed [--lds-bytes N] [--out FILE]
       timeout -k 10 900 python scripts/block_rhs_time.py cfg5 [--macro-dtype f32] [--lds-bytes N] [--ncols 1,2,3,4] [--out FILE]
       timeout -k 10 900 python scripts/block_rhs_time.py cfg2 --fused [--ncols 1,2,3,4] [--out FILE]
(one GPU step = one process: give each its own time limit)
Without --condensed every level holds dense inverses: the library looks for no groups and the generator's group labels (the
Scott-Vogelius macro stars of config 5) are dropped.
--lds-bytes: Context.set_block_lds_bytes, the LDS a workgroup of the condensed or the macro stars' block apply or of the
de-duplicated block product may ask for (default 64 KiB; the width of every level's apply and product is printed, with the
largest number of distinct columns in a group of 1024 blocks, which is what sets the product's).
--macro-dtype f32: every level is asked for the FP32 storage of dense macro-star inverses (Level.set_macro_patch_storage) and
factored again; a level that refuses keeps FP64.

--fused: the A/B of the block form of the four-launch smoother iteration instead (Context.set_block_fused; every other block
kernel stays on in both modes, so "off" is what these levels did before that form existed): per level ``smooth_block(k)`` with a
zero guess, and the full cycle, at every ncol, on and off alternating round after round; per level its mode
(Level.smooth_block_mode) and which stage 1 it has (interleaved copy, dense stars, pieces).

Per level with patches and per ncol: best ms per block apply (both stages) and per block product over the rounds, on / off and
their ratio, and the stored bytes (alfi_patches_factor_bytes; operator values + column indices) per second of the batched call.
ncol = 1 always takes the single-vector path, whatever the switch says.  The bytes argument: a batched apply of 4 columns moves
8 n_p^2 + 4 * 20 n_p bytes per patch where 4 single applies move 4 (8 n_p^2 + 20 n_p): 0.26-0.27 of the time at n_p = 111-153
while it stays bandwidth-bound."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cfg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--dtype", default=None, choices=[None, "f32"])
    ap.add_argument("--condensed", action="store_true", help="the default condensation policy instead of dense inverses")
    ap.add_argument("--lds-bytes", type=int, default=None)
    ap.add_argument("--macro-dtype", default=None, choices=[None, "f32"])
    ap.add_argument("--ncols", default="1,2,4", help="column counts to time; 1 is always among them (the single apply)")
    ap.add_argument("--fused", action="store_true", help="A/B of Context.set_block_fused: smoother per level and full cycle")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    NCOLS = tuple(sorted({1} | {int(c) for c in args.ncols.split(",")}))
    import torch
    import bench
    from alfi_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("block_rhs_time.py measures on the GPU; none is visible")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    t0 = time.time()
    lv, tr, k = bench.build_problem(args.cfg, False)
    say("%s: %s" % (args.cfg, bench.describe(args.cfg)))
    say("hierarchy generated on the host in %.1f s; patches per level %s, largest patch %d dofs"
        % (time.time() - t0, [len(L.patch_ptr) - 1 for L in lv[1:]], int(np.diff(lv[-1].patch_ptr).max())))
    ctx = hip.Context(0)
    if not args.condensed:
        ctx.set_condense_min_bytes(-1)              # dense inverses on every level: the library looks for no groups ...
        for L in lv[1:]:
            L.patch_groups = None                   # ... and the generator's are dropped
    if args.lds_bytes is not None:
        ctx.set_block_lds_bytes(args.lds_bytes)
    mg = hip.Multigrid(ctx, lv, tr, k, patch_factor_dtype=args.dtype)
    if args.macro_dtype is not None:
        for d in mg.levels[1:]:
            hip.ask_macro_patch_storage(d, args.macro_dtype)
            d.factor()
        ctx.sync()
    say("%s; per level (dofs, patches, factor GB, apply batched, product batched): %s"
        % ("the default condensation policy" if args.condensed else "dense %s inverses" % (args.dtype or args.macro_dtype or "f64"),
           ["%d/%d/%.3f/%d/%d" % (d.n, len(L.patch_ptr) - 1, d.factor_bytes() / 1e9, d.patch_apply_block_batched(),
                                  d.spmv_block_batched()) for L, d in zip(lv[1:], mg.levels[1:])]))
    if args.condensed:
        # per level: condensed() (0 dense, 1 the caller's groups, 2 the library's), the width of the block apply, the expectation
        # from bytes at 4 columns -- (factor bytes + 4 vector bytes) / (4 (factor bytes + vector bytes)), vector bytes = 20 per
        # patch entry (index, value, staged result) -- and the per-column scratch of a batched apply (one slot of blk_stage and
        # one of blk_ctmp, 8 bytes per patch entry each)
        for L, d in zip(lv[1:], mg.levels[1:]):
            fb, vb = float(d.factor_bytes()), 20.0 * float(L.patch_ptr[-1])
            say("  level %d: condensed %d, block width %d%s, expected 4-column ratio from bytes %.3f, scratch per column slot: stage "
                "%.3f GB + ctmp %.3f GB" % (d.id, d.condensed(), d.patch_apply_block_width(),
                                            "" if args.lds_bytes is None else " (LDS budget %d)" % args.lds_bytes,
                                            (fb + 4 * vb) / (4 * (fb + vb)),
                                            8e-9 * float(((np.diff(L.patch_ptr) + 1) & ~1).sum()), 8e-9 * float(L.patch_ptr[-1])))
    else:
        # dense levels: what each one holds, the width of its block apply and, for macro stars, the LDS of a workgroup at that width
        for L, d in zip(lv[1:], mg.levels[1:]):
            w, m = d.patch_apply_block_width(), int(np.diff(L.patch_ptr).max())
            say("  level %d: storage %s, largest patch %d dofs, block width %d%s%s"
                % (d.id, d.patch_storage_dtype(), m, w, "" if args.lds_bytes is None else " (LDS budget %d)" % args.lds_bytes,
                   ", %d bytes of LDS per workgroup" % (w * 8 * ((m + 1) & ~1)) if m > 160 and w >= 2 else ""))
    # the product: distinct columns per group of 1024 blocks (what the de-duplicated product stages in LDS; counted here from the
    # host operator), its block width, and the expectation from bytes at ncol columns -- (operator bytes + ncol x vector bytes) /
    # (ncol x (operator bytes + vector bytes)); operator bytes = values, 2-byte local indices and the groups' column lists, vector
    # bytes = one x gather per distinct column of a group and the result
    for L, d in zip(lv[1:], mg.levels[1:]):
        col, bs = np.asarray(L.A.colidx, dtype=np.int64), d.bs
        pad = np.full(-len(col) % 1024, -1, dtype=np.int64)
        grp = np.sort(np.concatenate([col, pad]).reshape(-1, 1024), axis=1)
        uniq = 1 + (np.diff(grp, axis=1) != 0).sum(axis=1) - (grp[:, 0] < 0)          # (the pad value is not a column)
        ob, vb = float(len(col) * (8 * bs * bs + 2) + 4 * uniq.sum()), float(8 * bs * uniq.sum() + 8 * d.n)
        say("  level %d product: %d blocks of bs %d, distinct columns per group of 1024 blocks max %d mean %.1f, block width %d%s, "
            "expected ratio from bytes %s" % (d.id, len(col), bs, uniq.max(), uniq.mean(), d.spmv_block_width(),
                                              "" if args.lds_bytes is None else " (LDS budget %d)" % args.lds_bytes,
                                              " ".join("%d: %.3f" % (c, (ob + c * vb) / (c * (ob + vb))) for c in NCOLS[1:])))
    rng = np.random.default_rng(0)

    def timed(fn, reps):
        ctx.sync()
        t0 = time.time()
        for _ in range(reps):
            fn()
        ctx.sync()
        return 1e3 * (time.time() - t0) / reps

    if args.fused:
        fused_ab(args, say, ctx, lv, mg, k, NCOLS, rng, timed)
        mg.close()
        ctx.close()
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    work = []      # (label, stored bytes or None, {ncol: callable})
    for L, dl in zip(lv[1:], mg.levels[1:]):
        X = {c: ctx.mat(rng.standard_normal((dl.n, c))) for c in NCOLS}
        Y = {c: ctx.mat(dl.n, c) for c in NCOLS}
        work.append(("level %d apply  " % dl.id, dl.factor_bytes(),
                     {c: (lambda dl=dl, c=c, X=X, Y=Y: dl.patch_apply_block(X[c], Y[c])) for c in NCOLS}))
        work.append(("level %d product" % dl.id, dl.nnzb * (8 * dl.bs * dl.bs + 4),
                     {c: (lambda dl=dl, c=c, X=X, Y=Y: dl.spmv_block(X[c], Y[c])) for c in NCOLS}))
    fine = lv[-1]
    Bf = rng.standard_normal((fine.n, max(NCOLS)))
    Bf[fine.bc_dofs] = 0.0
    B = {c: ctx.mat(Bf[:, :c]) for c in NCOLS}
    Xf = {c: ctx.mat(fine.n, c) for c in NCOLS}
    work.append(("full cycle      ", None, {c: (lambda c=c: mg.fcycle_block(B[c], Xf[c])) for c in NCOLS}))
    res = {(w[0], c, on): [] for w in work for c in NCOLS for on in (True, False)}
    for on in (True, False):                        # warm-up: every shape, both modes (the lazy workspaces are allocated here)
        ctx.set_block_kernels(on)
        for label, _, fns in work:
            for c in NCOLS:
                fns[c]()
    ctx.sync()
    for _ in range(args.rounds):
        for on in (True, False):
            ctx.set_block_kernels(on)
            for label, _, fns in work:
                for c in NCOLS:
                    res[(label, c, on)].append(timed(fns[c], args.cycles if label.startswith("full") else args.reps))
    ctx.set_block_kernels(True)
    say()
    say("best ms per call over %d rounds (%d calls each, cycles %d), modes alternating; on = batched kernels, off = looped:"
        % (args.rounds, args.reps, args.cycles))
    say("  %-18s ncol       on      off   on/off   on/(ncol x single)   stored TB/s (on)" % "")
    for label, nbytes, _ in work:
        single = min(res[(label, 1, False)])
        for c in NCOLS:
            on, off = min(res[(label, c, True)]), min(res[(label, c, False)])
            say("  %-18s %4d %8.4f %8.4f   %6.3f   %18.3f   %s"
                % (label, c, on, off, on / off, on / (c * single), "%16.3f" % (nbytes / (on * 1e-3) / 1e12) if nbytes else ""))
    say()
    say("spread over the rounds (max - min, ms), finest level apply at %d columns: on %.4f, off %.4f"
        % ((NCOLS[-1],) + tuple(max(res[(work[-3][0], NCOLS[-1], on)]) - min(res[(work[-3][0], NCOLS[-1], on)]) for on in (True, False))))
    say("spread over the rounds (max - min, ms), finest level product at %d columns: on %.4f, off %.4f"
        % ((NCOLS[-1],) + tuple(max(res[(work[-2][0], NCOLS[-1], on)]) - min(res[(work[-2][0], NCOLS[-1], on)]) for on in (True, False))))
    say("every round, ms per block apply / block product (on/off) -- is batched faster than looped in EVERY round?")
    for label, _, _ in work:
        if "apply" in label or "product" in label:
            for c in NCOLS[1:]:
                pairs = list(zip(res[(label, c, True)], res[(label, c, False)]))
                say("  %-18s %4d  %s  %s" % (label, c, " ".join("%.4f/%.4f" % t for t in pairs),
                                             "faster in every round" if all(a < b for a, b in pairs) else "NOT faster in every round"))
    mg.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def fused_ab(args, say, ctx, lv, mg, k, NCOLS, rng, timed):
    """Context.set_block_fused on / off alternating: smooth_block(k) per level and the full cycle at every ncol"""
    say()
    say("block fused iteration, k = %d; per level (dofs, patches, largest patch, mode on, class of stage 1):" % k)
    for L, d in zip(lv[1:], mg.levels[1:]):
        m = int(np.diff(L.patch_ptr).max())
        cls = ("interleaved copy" if m <= 32 and d.condensed() == 0 and d.patch_storage_dtype() == "f64" else
               "dense stars" if d.patch_apply_block_batched() and d.condensed() == 0 and m <= 160 else
               "pieces of %d" % d.patch_apply_block_width() if d.patch_apply_block_width() >= 2 else "none")
        say("  level %d: %d dofs, %d patches, %d dofs, mode %d, %s" % (d.id, d.n, len(L.patch_ptr) - 1, m, d.smooth_block_mode(k), cls))
    work = []
    for L, dl in zip(lv[1:], mg.levels[1:]):
        Bm = {c: ctx.mat(rng.standard_normal((dl.n, c))) for c in NCOLS}
        Xm = {c: ctx.mat(dl.n, c) for c in NCOLS}
        work.append(("level %d smoother " % dl.id, dl.smooth_block_mode(k),
                     {c: (lambda dl=dl, c=c, Bm=Bm, Xm=Xm: dl.smooth_block(k, Bm[c], Xm[c], nonzero_guess=False)) for c in NCOLS}))
    fine = lv[-1]
    Bf = rng.standard_normal((fine.n, max(NCOLS)))
    Bf[fine.bc_dofs] = 0.0
    B = {c: ctx.mat(Bf[:, :c]) for c in NCOLS}
    Xf = {c: ctx.mat(fine.n, c) for c in NCOLS}
    work.append(("full cycle       ", None, {c: (lambda c=c: mg.fcycle_block(B[c], Xf[c])) for c in NCOLS}))
    res = {(w[0], c, on): [] for w in work for c in NCOLS for on in (True, False)}
    for on in (True, False):                        # warm-up: every shape, both modes (the lazy workspaces are allocated here)
        ctx.set_block_fused(on)
        for label, _, fns in work:
            for c in NCOLS:
                fns[c]()
    ctx.sync()
    for _ in range(args.rounds):
        for on in (True, False):
            ctx.set_block_fused(on)
            for label, _, fns in work:
                for c in NCOLS:
                    res[(label, c, on)].append(timed(fns[c], args.cycles if label.startswith("full") else args.reps))
    ctx.set_block_fused(True)
    say()
    say("best ms per call over %d rounds (%d calls each, cycles %d), modes alternating; on = block fused iteration, off = these "
        "levels loop whole smoother calls (every other block kernel on):" % (args.rounds, args.reps, args.cycles))
    say("  %-18s ncol       on      off   on/off   on/(ncol x single)" % "")
    for label, mode, _ in work:
        single = min(res[(label, 1, False)])
        for c in NCOLS:
            on, off = min(res[(label, c, True)]), min(res[(label, c, False)])
            say("  %-18s %4d %8.4f %8.4f   %6.3f   %18.3f%s" % (label, c, on, off, on / off, on / (c * single),
                                                              "" if mode is None or mode == 2 else "   (mode %d: not the fused form)" % mode))
    say()
    say("every round, ms per call (on/off) -- is the block fused form faster than looping in EVERY round?")
    for label, _, _ in work:
        for c in NCOLS[1:]:
            pairs = list(zip(res[(label, c, True)], res[(label, c, False)]))
            say("  %-18s %4d  %s  %s" % (label, c, " ".join("%.4f/%.4f" % t for t in pairs),
                                         "faster in every round" if all(a < b for a, b in pairs) else "NOT faster in every round"))


if __name__ == "__main__":
    main()
