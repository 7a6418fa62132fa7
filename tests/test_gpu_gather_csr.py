"""``Context.gather_csr`` (alfi_vec_gather_csr: dst node i = sum_k w_k src node c_k, bs doubles per node) against a NumPy row
loop (-m gpu, one process).

Bound: the kernel adds a row's products in CSR order by fused multiply-adds, the reference in the same order with separate
roundings; either is within len(row) (eps / 2) (|W| |x|) of the exact sum to first order (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1), so they differ by at most len(row) eps (|W| |x|), entry by entry.  One-entry rows of weight 1.0 must copy bit for bit (the sign of a zero included), empty rows give
+0.0, and two calls give the same bits (fixed summation order)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NSRC = 300                                   # source nodes
LENGTHS = (0, 1, 2, 9, 200)


@pytest.fixture(scope="module")
def ctx():
    from alfi_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _rows(nrows, seed):
    """Seeded random CSR: row lengths from LENGTHS, weights in [-1, 1]; every third one-entry row has weight exactly 1.0."""
    rng = np.random.default_rng(seed)
    lens = rng.choice(LENGTHS, nrows) if nrows else np.zeros(0, dtype=np.int64)
    if nrows >= 63:
        lens[:5] = LENGTHS                   # every length present
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, NSRC, ptr[-1])
    w = rng.uniform(-1.0, 1.0, ptr[-1])
    ones = np.flatnonzero(lens == 1)[::3]
    w[ptr[ones]] = 1.0
    return ptr, col, w, ones


def _reference(ptr, col, w, x, bs):
    """(ref, |W| |x|) by a loop over the rows, the entries in CSR order."""
    X = x.reshape(-1, bs)
    ref, mag = np.zeros((len(ptr) - 1, bs)), np.zeros((len(ptr) - 1, bs))
    for i in range(len(ptr) - 1):
        for k in range(ptr[i], ptr[i + 1]):
            ref[i] += w[k] * X[col[k]]
            mag[i] += abs(w[k]) * np.abs(X[col[k]])
    return ref, mag


@pytest.mark.parametrize("bs", [1, 2, 3])
@pytest.mark.parametrize("nrows", [0, 1, 63, 64, 65, 1000])
def test_gather_csr_against_row_loop(ctx, bs, nrows):
    ptr, col, w, ones = _rows(nrows, 1000 * bs + nrows)
    x = np.random.default_rng(7).uniform(-1.0, 1.0, NSRC * bs)
    x[:2 * bs] = [-0.0, 0.0] * bs            # zeros of either sign among the sources
    if nrows and ones.size:
        col[ptr[ones[0]]] = 0                # a weight-1.0 row that copies them
    src, dst = ctx.vec(x), ctx.vec(np.full(max(nrows * bs, 1), 7.0))
    dptr, dcol, dw = ctx.ivec(ptr), ctx.ivec(col), ctx.vec(w if w.size else np.zeros(1))
    ctx.gather_csr(dst, src, dptr, dcol, dw, bs)
    got = dst.get()
    if nrows == 0:
        assert got[0] == 7.0                 # a no-op
        return
    got = got.reshape(nrows, bs)
    ref, mag = _reference(ptr, col, w, x, bs)
    lens = np.diff(ptr)
    err = np.abs(got - ref)
    print("bs %d, %d rows: max error %.2e, max of error / (len eps |W||x|) %.2f"
          % (bs, nrows, err.max(), (err / np.maximum(lens[:, None] * EPS * mag, 1e-300)).max()))
    assert (err <= lens[:, None] * EPS * mag).all()
    X = x.reshape(-1, bs)
    assert got[ones].tobytes() == X[col[ptr[ones]]].tobytes()           # weight 1.0: a copy, bit for bit
    empty = got[lens == 0]
    assert empty.tobytes() == np.zeros_like(empty).tobytes()            # empty rows: +0.0
    dst2 = ctx.vec(np.full(nrows * bs, -3.0))
    ctx.gather_csr(dst2, src, dptr, dcol, dw, bs)
    assert dst2.get().tobytes() == got.tobytes()                        # the same bits again


def test_gather_csr_of_pairs_from_an_8_byte_aligned_source(ctx):
    """bs = 2 from and into views at an odd offset: no 16-byte access may be made; the same bits as the aligned call."""
    from alfi_amd import hip
    ptr, col, w, _ = _rows(65, 5)
    x = np.random.default_rng(8).uniform(-1.0, 1.0, NSRC * 2)
    dptr, dcol, dw = ctx.ivec(ptr), ctx.ivec(col), ctx.vec(w)
    src, dst = ctx.vec(x), ctx.vec(130)
    ctx.gather_csr(dst, src, dptr, dcol, dw, 2)
    src1, dst1 = ctx.vec(np.concatenate([[0.0], x])), ctx.vec(131)
    ctx.gather_csr(hip.view(dst1, 1, 130), hip.view(src1, 1, NSRC * 2), dptr, dcol, dw, 2)
    assert dst1.get()[1:].tobytes() == dst.get().tobytes()


def test_gather_csr_refuses_bad_arguments(ctx):
    """bs = 0 and NULL arrays with nrows > 0: AlfiHipError, the destination untouched."""
    from alfi_amd import hip
    ptr, col, w, _ = _rows(4, 3)
    src, dst = ctx.vec(np.ones(NSRC)), ctx.vec(np.full(4, 7.0))
    dptr, dcol, dw = ctx.ivec(ptr), ctx.ivec(col), ctx.vec(w if w.size else np.zeros(1))
    with pytest.raises(hip.AlfiHipError):
        ctx.gather_csr(dst, src, dptr, dcol, dw, 0)
    call = ctx.lib.alfi_vec_gather_csr
    null = ctypes.c_void_p(None)
    for args in ((null, src.ptr, dptr.ptr, dcol.ptr, dw.ptr), (dst.ptr, null, dptr.ptr, dcol.ptr, dw.ptr),
                 (dst.ptr, src.ptr, null, dcol.ptr, dw.ptr), (dst.ptr, src.ptr, dptr.ptr, null, dw.ptr),
                 (dst.ptr, src.ptr, dptr.ptr, dcol.ptr, null)):
        with pytest.raises(hip.AlfiHipError):
            ctx.check(call(ctx.h, *args, 4, 1))
    with pytest.raises(hip.AlfiHipError):
        ctx.check(call(ctx.h, dst.ptr, src.ptr, dptr.ptr, dcol.ptr, dw.ptr, -1, 1))
    assert call(ctx.h, null, null, null, null, null, 0, 1) == 0          # nrows == 0: a no-op whatever the pointers
    ctx.sync()
    assert (dst.get() == 7.0).all()
