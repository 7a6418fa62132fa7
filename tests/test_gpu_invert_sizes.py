"""Every dense patch-inversion kernel at every size it serves, with the pivoted repair out of the picture.  -m gpu; one worker
subprocess per environment setting (tests/gpu_invert_sizes_worker.py), the references on the host (tests/invert_cases.py).

alfi_patches_factor follows every fast inversion with a residual probe and a pivoted re-inversion of the patches that fail it
(kernels_check.hip), so a wrong inversion kernel is repaired and every comparison further down still passes; the only trace is
flagged > 0.  Here every level must come out with flagged == repaired == 0 AND every stored inverse within
invert_cases.tolerance() (32 x the error of LAPACK's own float64 inverse, ~5.4e-14, seven orders below the probe) of an
extended-precision reference, entrywise relative to max |X_ref|; a second factor() must store the same bits; and the additive
apply of those inverses is held to a componentwise float64 error bound.

Which kernel a level reaches is decided by its largest patch and ALFI_INVERT_MFMA (launch_patch_invert_arrays,
launch_patch_invert_mfma, alfi_patches_factor) -- kernel_of() below repeats that dispatch to NAME the instantiation in failure
messages and in the printed table, it selects nothing:

  max_np          default, ALFI_TEST_LARGE_PATHS=1     ALFI_INVERT_MFMA=0             ALFI_INVERT_MFMA=2
  <= 8, 16, 32    invert_small_kernel<8 | 16 | 32>     the same                       the same
  33 .. 64        patch_invert_big_kernel<7>           patch_invert_big_kernel<7>     patch_invert_mfma_kernel<4>
  65 .. 96        patch_invert_big_kernel<7>           patch_invert_big_kernel<7>     patch_invert_mfma_kernel<6>
  97 .. 112       patch_invert_big_kernel<7>           patch_invert_big_kernel<7>     patch_invert_mfma_kernel<8>
  113 .. 128      patch_invert_mfma_kernel<8>          patch_invert_big_kernel<10>    patch_invert_mfma_kernel<8>
  129 .. 160      patch_invert_mfma_kernel<10>         patch_invert_big_kernel<10>    patch_invert_mfma_kernel<10>
  > 160           launch_big_factor (64-wide pivot blocks + Newton-Schulz polish)

The apply (launch_patch_apply_range): max_np <= 32 the interleaved copy (patch_apply_il_kernel<4 | 7 | 8 | 12 | 16>), 33 .. 64
patch_apply_kernel with one wave, above 64 big_apply_kernel (these levels have <= 256 patches) -- under ALFI_TEST_LARGE_PATHS=1
patch_apply_kernel with four (65 .. 128) or eight (129 .. 160) waves instead; above 160 big_apply_kernel always.

Measured on an MI355X (worst max |X - X_ref| / max |X_ref| per kernel family over all settings, levels, sizes and both block
sizes; the run-time tolerance it was compared with came out as 5.61e-14 on that machine; flagged == repaired == 0 everywhere,
worst probe residual 2.8e-14):

  invert_small_kernel<8>         2.2e-16        patch_invert_mfma_kernel<4>    1.2e-15
  invert_small_kernel<16>        5.1e-16        patch_invert_mfma_kernel<6>    1.8e-15
  invert_small_kernel<32>        6.0e-16        patch_invert_mfma_kernel<8>    2.2e-15
  patch_invert_big_kernel<7>     2.1e-15        patch_invert_mfma_kernel<10>   3.0e-15
  patch_invert_big_kernel<10>    2.8e-15        launch_big_factor              3.2e-15

The apply stayed below 1 % of its bound (worst |y - y_ref| / bound 9.4e-3).  Each setting takes ~3 s, the references ~6 s once."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import invert_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# under the defaults both block sizes run every level; the gather is the only BS-templated step, so under the other settings
# bs = 2 runs one level per inversion family only
FULL = ("3:all", "2:all")
REDUCED = ("3:all", "2:32,112,160")
SETTINGS = [("default", {}, FULL),
            ("mfma0", {"ALFI_INVERT_MFMA": "0"}, REDUCED),
            ("mfma2", {"ALFI_INVERT_MFMA": "2"}, REDUCED),
            ("large-paths", {"ALFI_TEST_LARGE_PATHS": "1"}, REDUCED)]


def kernel_of(env, cap):
    """The inversion kernel a level of largest patch ``cap`` reaches under ``env`` (see the table above)."""
    if cap <= 32:
        return "invert_small_kernel<%d>" % ic.small_width(cap)
    if cap > 160:
        return "launch_big_factor"
    mode = int(env.get("ALFI_INVERT_MFMA", "1"))
    if mode != 0 and (cap > 112 or mode == 2):
        return "patch_invert_mfma_kernel<%d>" % (4 if cap <= 64 else 6 if cap <= 96 else 8 if cap <= 128 else 10)
    return "patch_invert_big_kernel<%d>" % (7 if cap <= 112 else 10)


@pytest.fixture(scope="module")
def tol():
    """The run-time tolerance; computing it fills the cache of references (both operators, every size) once per module."""
    return ic.tolerance()


@pytest.fixture(scope="module")
def applied():
    """{(bs, n): (X_ref x[D_n], |X_ref| |x[D_n]|)} in longdouble, shared by all settings."""
    x = ic.apply_input().astype(np.longdouble)
    return {(bs, n): (ic.reference(bs, n) @ x[ic.dofs(n)], np.abs(ic.reference(bs, n)) @ np.abs(x[ic.dofs(n)]))
            for bs in (3, 2) for n in ic.sizes_in_use()}


def jobs_of(spec):
    levels = ic.levels()
    for job in spec:
        bs, caps = job.split(":")
        for cap in (list(levels) if caps == "all" else [int(c) for c in caps.split(",")]):
            yield int(bs), cap, levels[cap]


@pytest.mark.parametrize("name,env,spec", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_every_inversion_kernel_at_every_size(name, env, spec, tol, applied, tmp_path):
    f = str(tmp_path / "inv.npz")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_invert_sizes_worker.py"), f] + list(spec),
                         env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    res = np.load(f)
    fails, family = [], {}
    for bs, cap, sizes in jobs_of(spec):
        where = "%s, bs %d, max_np %d (%s)" % (name, bs, cap, kernel_of(env, cap))
        key = "%d_%d_" % (bs, cap)
        worst, flagged, repaired, after = res[key + "check"]
        # the condition that takes the safety net away: nothing flagged, nothing re-inverted
        if not (flagged == 0 and repaired == 0):
            fails.append("%s: probe flagged %d, repaired %d patches (worst residual %.3e)" % (where, flagged, repaired, worst))
        inv, same, at, lvl_err = res[key + "inv"], res[key + "same"], 0, 0.0
        for p, n in enumerate(sizes):
            X, Xr = inv[at:at + n * n].reshape(n, n), ic.reference(bs, n)
            at += n * n
            err = float(np.abs(X - Xr).max() / np.abs(Xr).max())
            lvl_err = max(lvl_err, err if np.isfinite(err) else np.inf)
            if not err <= tol:
                fails.append("%s: patch %d, n %d: max |X - X_ref| / max |X_ref| = %.3e > %.3e" % (where, p, n, err, tol))
            if not same[p]:
                fails.append("%s: patch %d, n %d: a second factor() stored other bits" % (where, p, n))
        assert at == len(inv)
        family[kernel_of(env, cap)] = max(family.get(kernel_of(env, cap), 0.0), lvl_err)
        # the apply: y_i = sum over the patches holding dof i of (X_p x[D_p])_i; an n-term float64 dot product and an m_i-term
        # sum on top of the inverses' own error stay below (tol + (max_np + m_i + 2) 2^-53) sum_p sum_c |X_p[r, c]| |x_c|
        yr, mag, m = np.zeros(ic.NDOF, np.longdouble), np.zeros(ic.NDOF, np.longdouble), np.zeros(ic.NDOF, np.int64)
        for n in sizes:
            d = ic.dofs(n)
            yr[d] += applied[bs, n][0]
            mag[d] += applied[bs, n][1]
            m[d] += 1
        y = res[key + "y"]
        bound = (tol + (cap + m + 2) * 2.0 ** -53) * mag
        diff = np.abs(y - yr)
        bad = np.flatnonzero(~(diff <= bound))
        ratio = float((diff[m > 0] / bound[m > 0]).max())
        for i in bad[:5]:
            fails.append("%s: apply, dof %d (in %d patches): |y - y_ref| = %.3e > %.3e%s"
                         % (where, i, m[i], diff[i], bound[i], "" if m[i] else " (in no patch: must be exactly 0)"))
        print("%-11s bs %d max_np %3d %-28s probe worst %.2e  inverse %.2e  apply / bound %.2e"
              % (name, bs, cap, kernel_of(env, cap), worst, lvl_err, ratio))
    for k, v in sorted(family.items()):
        print("%-11s %-28s worst entrywise error %.3e (tolerance %.3e)" % (name, k, v, tol))
    assert not fails, "%d failures; the first:\n" % len(fails) + "\n".join(fails[:40])
