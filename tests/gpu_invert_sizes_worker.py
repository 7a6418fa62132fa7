"""Worker of tests/test_gpu_invert_sizes.py: factors the synthetic levels of tests/invert_cases.py under the environment switches
the parent set (they are read once per process) and saves what the device holds to argv[1] (npz); argv[2:] are the jobs,
"BS:all" or "BS:cap,cap,...".  No comparison here -- the parent holds the references.

Per level (key prefix "<bs>_<cap>_"): check = patch_check() of the first factorisation; inv = every patch_inverse, row-major, one
after the other; same = per patch, whether a second factor() stored the identical bits; y = patch_apply of the seeded vector."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_level(hip, A, sizes, x):
    from tests import invert_cases as ic
    ctx = hip.Context(0)
    ctx.set_condense_min_bytes(-1)                       # no level decides to condense
    dl = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
    ptr, pd = ic.patch_arrays(sizes)
    dl.set_patches(ptr, pd)
    dl.factor()
    check = np.array(dl.patch_check(), dtype=np.float64)
    inv = [dl.patch_inverse(p, n) for p, n in enumerate(sizes)]
    dl.factor()
    same = np.array([np.array_equal(inv[p], dl.patch_inverse(p, n)) for p, n in enumerate(sizes)])
    dx, dy = ctx.vec(x), ctx.vec(ic.NDOF)
    dl.patch_apply(dx, dy)
    y = dy.get()
    del dx, dy
    dl.close()
    ctx.close()
    return {"check": check, "inv": np.concatenate([X.ravel() for X in inv]), "same": same, "y": y}


def main():
    from alfi_amd import hip
    from tests import invert_cases as ic
    levels, x, out = ic.levels(), ic.apply_input(), {}
    for job in sys.argv[2:]:
        bs, caps = job.split(":")
        bs = int(bs)
        A = ic.operator(bs)
        for cap in (list(levels) if caps == "all" else [int(c) for c in caps.split(",")]):
            for k, v in run_level(hip, A, levels[cap], x).items():
                out["%d_%d_%s" % (bs, cap, k)] = v
    np.savez(sys.argv[1], **out)
    print("OK", len(out) // 4, "levels", flush=True)


if __name__ == "__main__":
    main()
