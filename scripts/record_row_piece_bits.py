"""Records tests/golden/row_piece_bits.npz: the results of every kernel that streams a stored row piece of a dense patch
inverse (csrc/row_piece.h), bit for bit, on inputs that are closed formulas in integer arithmetic.  Public Python API only, so
the script runs on any tree that has the API; tests/test_gpu_row_piece_bits.py imports the cases from here and compares.

    python scripts/record_row_piece_bits.py [OUT.npz]          (needs the GPU; default OUT: tests/golden/row_piece_bits.npz)

Inputs.  Operator: banded BSR, bs 2 and 3, block (i, j) for |i - j| <= 6 with entries ((7 i + 13 j + 3 a + 5 b) mod 17 - 8) / 16,
diagonal blocks plus 64 I (dyadic, exact in FP64; diagonally dominant: the probe flags nothing).  Vector: x_i = ((11 i) mod 31 -
15) / 8.  Patches: windows of consecutive free dofs, patch p starting ``step`` blocks after patch p - 1; two Dirichlet dofs
(dof 1 and dof n - 2).  The operator of a case has as many block rows as its windows need.
The sweeps (case 10) need patches of whole nodes, so their windows are the sizes of their case rounded up to whole nodes, over
the nodes that hold no Dirichlet dof; a third set of windows (bs 3, 126 .. 159 dofs) takes the workgroup-per-small-patch sweep
through its 128-row pieces.

Recorded per case: the result vector of patch_apply and the SHA-256 of every patch's patch_inverse bytes.  Case 11 (condensed
levels) takes its operators from the host generator, so its INPUTS (BSR arrays, Dirichlet dofs, patches, groups) are stored too and
the test builds the level from the stored arrays.

The file is written with fixed zip time stamps: a second run reproduces it byte for byte."""
import hashlib
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "row_piece_bits.npz")
BAND = 6
SIZES_1 = [33, 34, 35, 36, 63, 64, 33, 48, 50]
CYCLE_2 = [65, 66, 67, 111, 127, 128, 36]
CYCLE_3 = [129, 130, 131, 153, 157, 158, 159, 160, 64]
# the two lists of tests/test_gpu_macro_storage.py: two workgroups per patch with the 513-dof patch, one without it
# sweeps of a workgroup per SMALL patch (<= 64 nodes, <= 160 dofs) that reach the 128-row pieces: bs 3 only (129 dofs are 65 nodes
# of bs 2, which the workgroup-per-macro-star sweep takes); whole nodes: 129, 141, 150, 159, 126 dofs
SIZES_10M = [128, 141, 150, 159, 126]
SIZES_5 = {2: [161, 162, 163, 164, 255, 256, 257, 385, 513, 150], 1: [161, 162, 163, 164, 255, 256, 257, 385, 150]}


def cycle(sizes, count):
    return [sizes[p % len(sizes)] for p in range(count)]


def banded_operator(nb, bs):
    from alfi_amd.problem import BSR
    i = np.repeat(np.arange(nb), 2 * BAND + 1)
    j = i + np.tile(np.arange(-BAND, BAND + 1), nb)
    keep = (j >= 0) & (j < nb)
    i, j = i[keep], j[keep]
    a, b = np.arange(bs)[:, None], np.arange(bs)[None, :]
    vals = (((7 * i + 13 * j)[:, None, None] + 3 * a + 5 * b) % 17 - 8) / 16.0
    vals[i == j] += 64.0 * np.eye(bs)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nb))])
    return BSR(nb, nb, bs, rowptr, j, vals)


def vector(n):
    return ((11 * np.arange(n)) % 31 - 15) / 8.0


def window_case(sizes, bs, step=1, whole_nodes=False):
    """(A, bc_dofs, patch_ptr, patch_dofs) of the windows of ``sizes`` dofs, ``step`` blocks apart"""
    if whole_nodes:
        nn = [(s + bs - 1) // bs for s in sizes]
        nb = max(1 + p * step + m for p, m in enumerate(nn)) + 1
        dofs = [np.arange((1 + p * step) * bs, (1 + p * step + m) * bs) for p, m in enumerate(nn)]
    else:
        nfree = max(p * step * bs + s for p, s in enumerate(sizes))
        nb = (nfree + 2 + bs - 1) // bs + 1
    n = nb * bs
    bc = np.array([1, n - 2], dtype=np.int32)
    if not whole_nodes:
        free = np.setdiff1d(np.arange(n), bc)
        dofs = [free[p * step * bs:p * step * bs + s] for p, s in enumerate(sizes)]
    ptr = np.concatenate([[0], np.cumsum([len(d) for d in dofs])]).astype(np.int64)
    return banded_operator(nb, bs), bc, ptr, np.concatenate(dofs).astype(np.int32)


def make_level(ctx, A, bc, ptr, dofs, storage=None, macro=False, reverse=False, groups=None):
    from alfi_amd import hip
    dl = hip.Level(ctx, A, bc)
    dl.set_patches(ptr, dofs)
    dl.set_patch_groups(groups)                  # None: dense inverses, no search for groups
    if storage is not None:
        (dl.set_macro_patch_storage if macro else dl.set_patch_storage)(storage)
    if reverse:                                  # eliminate every patch in the reverse of its order (the ranked gather)
        sizes = np.diff(ptr)
        dl.set_patch_canonical_order(np.concatenate([np.arange(s)[::-1] for s in sizes]).astype(np.int32))
    dl.factor()
    return dl


def apply(ctx, dl, n):
    dx, dy = ctx.vec(vector(n)), ctx.vec(n)
    dl.patch_apply(dx, dy)
    return dy.get()


def hashes(dl, ptr):
    out = np.empty((len(ptr) - 1, 32), dtype=np.uint8)
    for p in range(len(ptr) - 1):
        inv = dl.patch_inverse(p, int(ptr[p + 1] - ptr[p]))
        out[p] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(inv).tobytes()).digest(), dtype=np.uint8)
    return out


def additive(ctx, out, key, storage=None, macro=False, reverse=False, split=False):
    """one additive case for bs 2 and 3: result vector and inverse hashes under ``key``; split: the range launches at an odd cut
    must give the unsplit vector (case 9)"""
    for bs in (2, 3):
        A, bc, ptr, dofs = windows_of(key, bs)
        dl = make_level(ctx, A, bc, ptr, dofs, storage, macro, reverse)
        try:
            assert dl.patch_storage_dtype() == ("f32" if storage == "f32" else "f64") and dl.condensed() == 0
            n = A.nbrows * bs
            y = apply(ctx, dl, n)
            if split:
                npatch = len(ptr) - 1
                cut = npatch // 2 | 1
                dx, dy = ctx.vec(vector(n)), ctx.vec(n)
                dl.patch_apply_split(cut, dx, dy)
                assert np.array_equal(dy.get(), y), "%s bs %d: the launches [0, %d) and [%d, %d) differ from the full one" \
                    % (key, bs, cut, cut, npatch)
            out["%s.bs%d.y" % (key, bs)] = y
            out["%s.bs%d.sha" % (key, bs)] = hashes(dl, ptr)
        finally:
            dl.close()


# ---- the cases; next to each the kernel it reaches through launch_patch_apply_range --------------------------------------------
# key -> (sizes, blocks from one window to the next, windows of whole nodes)
WINDOWS = {"c01": (SIZES_1, 1, False), "c02": (cycle(CYCLE_2, 1001), 1, False), "c03": (cycle(CYCLE_3, 257), 1, False),
           "c04": (CYCLE_3, 1, False), "c05w1": (SIZES_5[1], 7, False), "c05w2": (SIZES_5[2], 7, False),
           "c10s": (SIZES_1, 1, True), "c10m": (SIZES_10M, 1, True), "c10b": (CYCLE_3, 1, True)}
for _twin, _of in (("c06", "c01"), ("c06r", "c01"), ("c06w4", "c02"), ("c07", "c03"), ("c08w1", "c05w1"), ("c08w2", "c05w2")):
    WINDOWS[_twin] = WINDOWS[_of]               # cases 6-8: the FP32 twins of cases 1, 2, 3 and 5


def windows_of(key, bs):
    sizes, step, whole = WINDOWS[key]
    return window_case(sizes, bs, step, whole)


def case01(ctx, out, fx=None):      # patch_apply_kernel<double, ., 1>: every patch <= 64 dofs
    additive(ctx, out, "c01")


def case02(ctx, out, fx=None):      # patch_apply_kernel<double, ., 4>: 65 .. 128 dofs, more than 1000 patches
    additive(ctx, out, "c02")


def case03(ctx, out, fx=None):      # patch_apply_kernel<double, ., 8>: above 128 dofs, more than 256 patches; + case 9
    additive(ctx, out, "c03", split=True)


def case04(ctx, out, fx=None):      # big_apply_kernel<double>: above 64 dofs, at most 256 patches
    additive(ctx, out, "c04")


def case05(ctx, out, fx=None):      # big_apply_kernel<double>: above 160 dofs, one workgroup per patch and two
    additive(ctx, out, "c05w1")
    additive(ctx, out, "c05w2")


def case06(ctx, out, fx=None):      # patch_apply_kernel<float, ., 1>; and once eliminated in reverse order (the ranked gather)
    additive(ctx, out, "c06", storage="f32")
    additive(ctx, out, "c06r", storage="f32", reverse=True)
    additive(ctx, out, "c06w4", storage="f32")      # patch_apply_kernel<float, ., 4>: the twin of case 2


def case07(ctx, out, fx=None):      # patch_apply_kernel<float, ., 8>; + case 9
    additive(ctx, out, "c07", storage="f32", split=True)


def case08(ctx, out, fx=None):      # big_apply_kernel<float>
    additive(ctx, out, "c08w1", storage="f32", macro=True)
    additive(ctx, out, "c08w2", storage="f32", macro=True)


def case10(ctx, out, fx=None):      # mult_wg_apply (up to 64 nodes and 160 dofs: c10s below 128 rows, c10m above) and big_mult_patch
                                    # (beyond: c10b): one symmetrised sweep
    for key, sizes_bs in (("c10s", (2, 3)), ("c10m", (3,)), ("c10b", (2, 3))):
        for bs in sizes_bs:
            A, bc, ptr, dofs = windows_of(key, bs)
            big = max(np.diff(ptr)) > 160 or max(np.diff(ptr)) // bs > 64
            assert big == (key == "c10b")
            dl = make_level(ctx, A, bc, ptr, dofs)
            try:
                dl.set_multiplicative(np.arange(len(ptr) - 1), True)
                out["%s.bs%d.y" % (key, bs)] = apply(ctx, dl, A.nbrows * bs)
            finally:
                dl.close()


COND = {"2d": (2, 2, 2), "3d": (1, 1, 2)}      # the 2d-P2 and 3d-P2 set-ups of tests/test_gpu_condensed.py: (N, nref, k)
COND_INPUTS = ("bs", "rowptr", "colidx", "vals", "bc", "ptr", "dofs", "groups")


def condensed_inputs(name):
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, TwoDimLidDrivenCavityProblem
    from alfi_amd.sv import build_sv_hierarchy
    N, nref, k = COND[name]
    prob = TwoDimLidDrivenCavityProblem(N) if name == "2d" else ThreeDimLidDrivenCavityProblem(N)
    L = build_sv_hierarchy(prob, nref, k, Re=100.0)[0][-1]
    return {"bs": np.int64(L.A.bs), "rowptr": L.A.rowptr, "colidx": L.A.colidx, "vals": L.A.vals,
            "bc": np.asarray(L.bc_dofs, dtype=np.int32), "ptr": np.asarray(L.patch_ptr, dtype=np.int64),
            "dofs": np.asarray(L.patch_dofs, dtype=np.int32), "groups": np.asarray(L.patch_groups, dtype=np.int32)}


def case11(ctx, out, fx=None):      # cond_sigma_kernel / cond_gsigma_kernel: big_rows over the stored inverse of the Schur complement
    from alfi_amd.problem import BSR
    for name in sorted(COND):
        key = "c11%s" % name
        inp = {f: fx["%s.in.%s" % (key, f)] for f in COND_INPUTS} if fx is not None else condensed_inputs(name)
        bs, nb = int(np.asarray(inp["bs"]).reshape(-1)[0]), len(inp["rowptr"]) - 1
        A = BSR(nb, nb, bs, inp["rowptr"], inp["colidx"], inp["vals"])
        dl = make_level(ctx, A, inp["bc"], inp["ptr"], inp["dofs"], groups=inp["groups"])
        try:
            assert dl.condensed() == 1
            out["%s.y" % key] = apply(ctx, dl, nb * bs)
        finally:
            dl.close()
        for f in COND_INPUTS:
            out["%s.in.%s" % (key, f)] = np.asarray(inp[f])


CASES = {"c01": case01, "c02": case02, "c03": case03, "c04": case04, "c05": case05, "c06": case06, "c07": case07, "c08": case08,
         "c10": case10, "c11": case11}     # (case 9 rides on cases 3 and 7)
PER_WAVEFRONT = "@per-wavefront"           # suffix of case 10's keys under ALFI_MULT_PERSISTENT=0


def run_cases(names, fx=None):
    from alfi_amd import hip
    ctx = hip.Context(0)
    out = {}
    try:
        for name in names:
            CASES[name](ctx, out, fx)
    finally:
        ctx.close()
    return out


def sweeps_per_wavefront():
    """case 10 in a fresh process under ALFI_MULT_PERSISTENT=0 (the library reads the switch once per process)"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sweeps.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweeps-only", path], cwd=ROOT,
                           env=dict(os.environ, ALFI_MULT_PERSISTENT="0"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        with np.load(path) as z:
            return {k + PER_WAVEFRONT: z[k] for k in z.files}


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and sorted names: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(argv):
    if len(argv) == 3 and argv[1] == "--sweeps-only":
        write_npz(argv[2], run_cases(["c10"]))
        return 0
    path = argv[1] if len(argv) > 1 else FIXTURE
    out = run_cases(sorted(CASES))
    out.update(sweeps_per_wavefront())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    write_npz(path, out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
