"""One level walked through the storage states of its patch factors: condensed by the library, dense FP64, dense FP32 (star and
macro request), condensed on the caller's groups, the interleaved small-patch copy.  After every step the level is compared, bit
for bit, with a fresh level put directly into the same state: patch_inverse of every patch, patch_apply of one fixed random vector
and patch_check().  That the fresh levels are right is what the storage, condensation and inversion suites establish.  -m gpu.

Shapes: (a) ldc3d on the 2 x 2 x 2 base mesh refined once, [P2+FB]^3 finest level (125 stars of at most 153 dofs), on a context
with set_condense_min_bytes(0); (b) the synthetic big-patch set of tests/test_gpu_macro_storage.py (windows of 150 .. 513 dofs)
with a work-buffer cap that gives several ranges and one patch above the cap; (c) 2-D lid-driven cavity N = 4 (stars of at most 32
dofs: the interleaved copy)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG_SIZES = [161, 162, 163, 164, 255, 256, 257, 385, 513, 150]        # SIZES[2] of tests/test_gpu_macro_storage.py


@pytest.fixture(scope="module")
def p2():
    from alfi_amd.problem import ThreeDimLidDrivenCavityProblem, build_hierarchy
    return build_hierarchy(ThreeDimLidDrivenCavityProblem(2), 1, 2, Re=1000.0)


def _state(ctx, dl, ptr, x):
    """(every patch inverse, the apply of x, the probe's figures)"""
    inv = [dl.patch_inverse(p, int(ptr[p + 1] - ptr[p])) for p in range(len(ptr) - 1)]
    dx, dy = ctx.vec(x), ctx.vec(len(x))
    dl.patch_apply(dx, dy)
    return inv, dy.get(), dl.patch_check()


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(u, v) for u, v in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) \
        and a[2] == b[2]


def _fresh(ctx, L, ptr, dofs, x, prepare):
    """the state of a new level that `prepare` puts directly where it belongs before its only factorisation"""
    from alfi_amd import hip
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    try:
        dl.set_patches(ptr, dofs)
        prepare(dl)
        dl.factor()
        return _state(ctx, dl, ptr, x), dl.condensed(), dl.patch_storage_dtype(), dl.factor_bytes()
    finally:
        dl.close()


def test_star_level_walk(p2):
    from alfi_amd import hip
    L = p2[0][-1]
    ptr, dofs = np.asarray(L.patch_ptr), L.patch_dofs
    npatch = len(ptr) - 1
    assert npatch == 125 and int(np.diff(ptr).max()) == 153
    x = np.random.default_rng(21).standard_normal(L.n)
    ref_ctx = hip.Context(0)
    ref_ctx.set_condense_min_bytes(0)
    try:
        own, mode, dt, _ = _fresh(ref_ctx, L, ptr, dofs, x, lambda dl: None)
        assert mode == 2 and dt == "f64"
        dense, mode, dt, _ = _fresh(ref_ctx, L, ptr, dofs, x, lambda dl: dl.set_patch_groups(None))
        assert mode == 0 and dt == "f64"
        f32, mode, dt, _ = _fresh(ref_ctx, L, ptr, dofs, x, lambda dl: dl.set_patch_storage("f32"))
        assert mode == 0 and dt == "f32"
        given, mode, dt, _ = _fresh(ref_ctx, L, ptr, dofs, x, lambda dl: dl.set_patch_groups(dl.find_patch_groups()))
        assert mode == 1 and dt == "f64"
    finally:
        ref_ctx.close()
    assert not _same(own, dense) and not _same(dense, f32)
    ctx = hip.Context(0)
    ctx.set_condense_min_bytes(0)
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    try:
        dl.set_patches(ptr, dofs)
        dl.factor()                                                      # 1
        s1 = _state(ctx, dl, ptr, x)
        assert dl.condensed() == 2 and _same(s1, own)
        dl.set_multiplicative(np.arange(npatch), False)                  # 2
        dl.set_multiplicative(None, False)
        s2 = _state(ctx, dl, ptr, x)
        assert dl.condensed() == 0 and dl.patch_storage_dtype() == "f64" and _same(s2, dense)
        dl.set_patch_storage("f32")                                      # 3
        dl.factor()
        s3 = _state(ctx, dl, ptr, x)
        assert dl.condensed() == 0 and dl.patch_storage_dtype() == "f32" and _same(s3, f32)
        assert ctx.f32_work_bytes() > 0
        dl.update_values(L.A.vals)                                       # 4
        dl.factor()
        assert dl.patch_storage_dtype() == "f32" and _same(_state(ctx, dl, ptr, x), s3)
        dl.set_patch_storage("f64")                                      # 5
        dl.factor()
        assert dl.condensed() == 0 and dl.patch_storage_dtype() == "f64" and _same(_state(ctx, dl, ptr, x), s2)
        assert ctx.f32_work_bytes() == 0
        dl.set_patch_groups(dl.find_patch_groups())                      # 6
        dl.factor()
        s6 = _state(ctx, dl, ptr, x)
        assert dl.condensed() == 1 and _same(s6, s1) and _same(s6, given)
        dl.set_patch_groups(None)                                        # 7
        dl.factor()
        assert dl.condensed() == 0 and _same(_state(ctx, dl, ptr, x), s2)
        dl.set_patches(ptr, dofs)                                        # 8
        dl.factor()
        assert dl.condensed() == 2 and _same(_state(ctx, dl, ptr, x), s1)
    finally:
        dl.close()
        ctx.close()


def test_big_patch_walk(p2):
    from alfi_amd import _hostlib, hip
    L = p2[0][-1]
    rng = np.random.default_rng(2)
    free = np.setdiff1d(np.arange(L.n), L.bc_dofs)
    ptr, dofs = [0], []
    for sz in BIG_SIZES:
        start = int(rng.integers(0, len(free) - sz))
        dofs.append(free[start:start + sz])                 # a window of consecutive free dofs: ascending, coupled
        ptr.append(ptr[-1] + sz)
    ptr, dofs = np.array(ptr, dtype=np.int64), np.concatenate(dofs).astype(np.int32)
    pbytes = 8 * np.diff(_hostlib.plan_patch_layout(L.n, ptr, dofs)["inv_ptr"])
    largest, cap = int(pbytes.max()), int(pbytes.sum()) // 4
    assert 3 * int(pbytes.min()) < cap < largest             # ranges of several patches, and one patch above the cap
    x = np.random.default_rng(3).standard_normal(L.n)

    def macro_f32(dl):
        dl.set_patch_groups(None)
        dl.set_macro_patch_storage("f32")
    ref_ctx = hip.Context(0)
    ref_ctx.set_f32_work_bytes(cap)
    try:
        f64, mode, dt, bytes64 = _fresh(ref_ctx, L, ptr, dofs, x, lambda dl: dl.set_patch_groups(None))
        assert mode == 0 and dt == "f64"
        f32, mode, dt, bytes32 = _fresh(ref_ctx, L, ptr, dofs, x, macro_f32)
        assert mode == 0 and dt == "f32"
    finally:
        ref_ctx.close()
    assert bytes32 < 0.55 * bytes64 and not _same(f32, f64)
    ctx = hip.Context(0)
    ctx.set_f32_work_bytes(cap)
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    try:
        dl.set_patches(ptr, dofs)
        macro_f32(dl)
        for want, ref, nbytes in (("f32", f32, bytes32), ("f64", f64, bytes64), ("f32", f32, bytes32)):
            dl.set_macro_patch_storage(want)
            dl.factor()
            assert dl.patch_storage_dtype() == want and dl.condensed() == 0 and dl.factor_bytes() == nbytes, want
            assert _same(_state(ctx, dl, ptr, x), ref), want
            held = ctx.f32_work_bytes()
            print("%s: work buffer %d bytes (cap %d, largest patch %d)" % (want, held, cap, largest))
            assert 0 < held <= max(cap, largest) if want == "f32" else held == 0
    finally:
        dl.close()
        ctx.close()


def test_small_patch_walk():
    from alfi_amd import hip
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, build_hierarchy
    lv, _ = build_hierarchy(TwoDimLidDrivenCavityProblem(4), 1, 2, Re=10.0)
    L = lv[-1]
    ptr, dofs = np.asarray(L.patch_ptr), L.patch_dofs
    assert int(np.diff(ptr).max()) <= 32
    x = np.random.default_rng(22).standard_normal(L.n)
    ctx = hip.Context(0)
    dl = hip.Level(ctx, L.A, L.bc_dofs)
    try:
        fresh, mode, dt, nbytes = _fresh(ctx, L, ptr, dofs, x, lambda dl: None)
        assert mode == 0 and dt == "f64"
        dl.set_patches(ptr, dofs)
        dl.factor()
        s = _state(ctx, dl, ptr, x)
        assert _same(s, fresh)
        with pytest.raises(hip.AlfiHipError) as e:
            dl.set_patch_storage("f32")
        assert e.value.code == hip.E_ARG
        assert dl.patch_storage_dtype() == "f64" and dl.factor_bytes() == nbytes and _same(_state(ctx, dl, ptr, x), s)
        dl.update_values(L.A.vals)
        dl.factor()
        assert dl.patch_storage_dtype() == "f64" and dl.condensed() == 0 and _same(_state(ctx, dl, ptr, x), s)
    finally:
        dl.close()
        ctx.close()
