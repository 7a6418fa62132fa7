"""The level product of a PARTITIONED level on every kernel it can take (level_spmv, csrc/api_level.hip), in one process on one
GPU, against plain references; and the scalar CSR product (csr_spmv_kernel).  -m gpu

Transport: the callback (Context.set_comm) with send and receive buffers of the test's own, as many send nodes as ghosts, and a
callback that copies the send buffer into the receive buffer on the ctx's stream -- ghost g receives x_own[send_nodes[g]], an
exchange with a known answer.  No patches (set_overlap(nb_interior, 0)).

Cases: tests/partitioned_product_cases.py; tests/test_partitioned_product.py proves on the host that each has the edge it is
listed for (forced and natural boundaries of the aligned chunk table; the cut of the de-duplicated and of the plain equal-chunk
kernel at lane 63, on a group, mid-chunk and on a chunk boundary; views that start at k % 64 of 0, 1, 8, 48, 61 and 63, of 63, 64
and 256 blocks, empty ones, rows across view chunks with carry runs of one, two and three).

Per case, partition and block size:
exact      values, x and b integers in [-8, 8] held in doubles: every partial sum is exact whatever the order, so spmv and residual
           must be np.array_equal to an int64 NumPy product of the owned rows with (x_own | x_own[send_nodes]) -- a dropped, doubled
           or misplaced block shows.  After update_values(2 vals) the product doubles (all three descriptors follow).
floating   standard-normal data against SciPy in FP64 at 1e-13 relative to the max-norm of the reference product (the SpMV bound
           of tests/test_gpu_parity.py): a narrowed accumulator shows.  A second call gives the same bits.
ghosts     x goes in with NaN in its ghost slots; afterwards its owned part is unchanged and the ghost slots hold
           x_own[send_nodes] bit for bit; the callback saw [FWD] without overlap, [FWD_BEGIN, FWD_END] with it.
untouched  y is pre-filled with a sentinel; the rows >= n_own keep it in both modes.
bitwise    (non-aligned uploads without overlap) the owned rows equal, bit for bit, the product of an unpartitioned Level of the
           same operator with the full x: the same kernel and chunks, only the block bound differs.  (This is the check that
           failed first, at large / nb_owned 5, bs 3: the last owned row was summed on at lane 63 through the idle lanes behind
           the cut, another rounding order.  The CUT form of the two equal-chunk kernels closes it at its last block.)"""
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alfi_amd import dist, hip
from tests import partitioned_product_cases as pc

SENTINEL = -7.25
NO_BC = np.zeros(0, dtype=np.int32)


class SelfExchange(object):
    """the callback transport of one ctx: send buffer -> receive buffer of the level that asks, on the ctx's stream"""

    def __init__(self, ctx):
        self.ctx, self.bufs, self.ops = ctx, {}, []
        self.cb = dist.CommFn(self._callback)
        self.dred = ctx.vec(64)                         # the buffer all-reduces would use (none happen here)
        ctx.set_comm(self.cb, self.dred.ptr.value, 64)

    def _callback(self, user, op, level_id, offset, count):
        try:
            self.ops.append(op)
            if op in (dist.COMM_HALO_FWD, dist.COMM_HALO_FWD_BEGIN):
                send, recv, n = self.bufs[level_id]
                if n:
                    self.ctx.copy(recv, send, n=n)
            return 0
        except Exception:                               # never let an exception cross the C boundary
            traceback.print_exc()
            return -1


@pytest.fixture(scope="module")
def env():
    ctx = hip.Context(0)
    try:
        yield ctx, SelfExchange(ctx)
    finally:
        ctx.close()


def _int_product(rowptr, colidx, vals, x, bs):
    """A x in int64, all block rows (every one non-empty)"""
    prod = np.einsum("kij,kj->ki", vals, x.reshape(-1, bs)[colidx])
    return np.add.reduceat(prod, rowptr[:-1].astype(np.int64), axis=0).ravel()


def _full(x_own, sn, bs):
    """(x_own | x_own[send_nodes]): what the exchange leaves in x"""
    return np.concatenate([x_own, x_own.reshape(-1, bs)[sn].ravel()])


def _partitioned_level(env, A, name, nb_owned, nb_interior):
    ctx, ex = env
    bs, nghost = A.bs, A.nbrows - nb_owned
    sn = pc.send_nodes(name, nb_owned)
    L = hip.Level(ctx, A, NO_BC)
    try:
        send, recv = ctx.vec(max(nghost * bs, 1)), ctx.vec(max(nghost * bs, 1))
        ex.bufs[L.id] = (send, recv, nghost * bs)
        L.set_partition(nb_owned, True, sn, send.ptr.value, recv.ptr.value, nghost)
        if nb_interior is not None:
            L.set_overlap(nb_interior, 0)
    except Exception:
        L.close()
        raise
    return L, sn


def _run(env, L, x_own, b, mode):
    """one spmv / residual with NaN ghosts in x and a sentinel-filled y: (y, x afterwards, the ops the callback saw)"""
    ctx, ex = env
    n, n_own = L.n, L.n_own
    dx = ctx.vec(np.concatenate([x_own, np.full(n - n_own, np.nan)]))
    dy = ctx.vec(np.full(n, SENTINEL))
    del ex.ops[:]
    if mode == 0:
        L.spmv(dx, dy)
    else:
        L.residual(ctx.vec(b), dx, dy)
    ctx.sync()
    return dy.get(), dx.get(), list(ex.ops)


@pytest.mark.parametrize("bs", [2, 3])
@pytest.mark.parametrize("name,nb_owned,nb_interior", pc.CASES)
def test_partitioned_product(env, name, nb_owned, nb_interior, bs):
    ctx, ex = env
    nb, rowptr, colidx = pc.structure(name, nb_interior)
    n, n_own, nnzb = nb * bs, nb_owned * bs, len(colidx)
    rng = np.random.default_rng(7 * nb_owned + bs)
    ivals = rng.integers(-8, 9, (nnzb, bs, bs))
    ix, ib = rng.integers(-8, 9, n_own), rng.integers(-8, 9, n)
    fvals = rng.standard_normal((nnzb, bs, bs))
    fx, fb = rng.standard_normal(n_own), rng.standard_normal(n)
    want_ops = [dist.COMM_HALO_FWD] if nb_interior is None else [dist.COMM_HALO_FWD_BEGIN, dist.COMM_HALO_FWD_END]
    tag = (name, nb_owned, nb_interior, bs)

    def check(L, sn, x_own, b, ref, exact):
        """both modes against ref = (A x)[:n_own]; returns the residual"""
        x_full = _full(x_own, sn, bs)
        for mode in (0, 1):
            y, x_after, ops = _run((ctx, ex), L, x_own, b, mode)
            want = ref if mode == 0 else b[:n_own] - ref
            if exact:
                assert np.array_equal(y[:n_own], want), (tag, mode)
            else:
                err, bound = np.abs(y[:n_own] - want).max(), 1e-13 * np.abs(ref).max()
                print("%s mode %d: error %.3e bound %.3e" % (tag, mode, err, bound))
                assert err < bound, (tag, mode, err, bound)
                y2, _, _ = _run((ctx, ex), L, x_own, b, mode)
                assert np.array_equal(y, y2), (tag, mode)                                  # the same bits again
            assert np.all(y[n_own:] == SENTINEL), (tag, mode)                              # rows >= n_own untouched
            assert np.array_equal(x_after[:n_own], x_own), (tag, mode)                     # owned part of x unchanged
            assert np.array_equal(x_after, x_full), (tag, mode)                            # ghosts: their owners' values, no NaN left
            assert ops == want_ops, (tag, mode, ops)
        return y

    # exact pass, then doubled values
    L, sn = _partitioned_level((ctx, ex), pc.operator(name, nb_interior, bs, ivals.astype(np.float64)), name, nb_owned, nb_interior)
    try:
        ref = _int_product(rowptr, colidx, ivals, _full(ix, sn, bs), bs)[:n_own]
        assert np.abs(ref).max() > 0
        check(L, sn, ix.astype(np.float64), ib.astype(np.float64), ref.astype(np.float64), True)
        L.update_values(2.0 * ivals)
        check(L, sn, ix.astype(np.float64), ib.astype(np.float64), 2.0 * ref, True)
    finally:
        ex.bufs.pop(L.id, None)
        L.close()

    # floating pass
    A = pc.operator(name, nb_interior, bs, fvals)
    L, sn = _partitioned_level((ctx, ex), A, name, nb_owned, nb_interior)
    try:
        x_full = _full(fx, sn, bs)
        ref = (A.to_scipy() @ x_full)[:n_own]
        y_res = check(L, sn, fx, fb, ref, False)
        y_mult = _run((ctx, ex), L, fx, fb, 0)[0]
    finally:
        ex.bufs.pop(L.id, None)
        L.close()

    # bitwise against the unpartitioned level: non-aligned uploads without overlap
    if nb_interior is None and pc.upload_kernel(rowptr) != "aligned":
        U = hip.Level(ctx, A, NO_BC)
        try:
            dx, dy = ctx.vec(x_full), ctx.vec(n)
            U.spmv(dx, dy)
            assert np.array_equal(dy.get()[:n_own], y_mult[:n_own]), tag
            U.residual(ctx.vec(fb), dx, dy)
            assert np.array_equal(dy.get()[:n_own], y_res[:n_own]), tag
        finally:
            U.close()


@pytest.mark.parametrize("bs", [2, 3])
def test_plain_equal_chunk_product_unpartitioned(env, bs):
    """bsr_spmv_flat_kernel in equal chunks without de-duplication (a row longer than a chunk, fewer than 1024 blocks), no partition"""
    ctx, _ = env
    nb, rowptr, colidx = pc.structure("plain")
    assert pc.upload_kernel(rowptr) == "plain"
    n, nnzb = nb * bs, len(colidx)
    rng = np.random.default_rng(40 + bs)
    ivals, ix, ib = rng.integers(-8, 9, (nnzb, bs, bs)), rng.integers(-8, 9, n), rng.integers(-8, 9, n)
    fvals, fx, fb = rng.standard_normal((nnzb, bs, bs)), rng.standard_normal(n), rng.standard_normal(n)
    for vals, x, b, exact in ((ivals.astype(np.float64), ix.astype(np.float64), ib.astype(np.float64), True), (fvals, fx, fb, False)):
        A = pc.operator("plain", None, bs, vals)
        L = hip.Level(ctx, A, NO_BC)
        try:
            dx, db, dy = ctx.vec(x), ctx.vec(b), ctx.vec(n)
            for mode in (0, 1):
                if mode == 0:
                    L.spmv(dx, dy)
                else:
                    L.residual(db, dx, dy)
                y = dy.get()
                if exact:
                    ref = _int_product(rowptr, colidx, ivals, ix, bs)
                    assert np.array_equal(y, ref if mode == 0 else ib - ref), (bs, mode)
                else:
                    ref = A.to_scipy() @ x
                    err, bound = np.abs(y - (ref if mode == 0 else b - ref)).max(), 1e-13 * np.abs(ref).max()
                    print("plain bs %d mode %d: error %.3e bound %.3e" % (bs, mode, err, bound))
                    assert err < bound, (bs, mode, err, bound)
                assert np.array_equal(dx.get(), x)
        finally:
            L.close()


@pytest.mark.parametrize("kind", sorted(pc.CSR_CASES))
def test_scalar_csr_product(env, kind):
    """hip.Csr.mult, the four modes on exact-integer data (any order of the sums gives the same doubles), and on standard-normal
    data against SciPy within the rounding of the two sums: the kernel's (at most the longest row's terms per lane and five
    levels of lane tree) plus SciPy's (the longest row), (2 x longest row + 6) x 2^-53 x max_i sum_j |a_ij| |x_j|"""
    import scipy.sparse as sp
    ctx, _ = env
    nrows, ncols, indptr, indices = pc.csr_structure(kind)
    rng = np.random.default_rng(60)
    ivals, ix = rng.integers(-8, 9, len(indices)), rng.integers(-8, 9, ncols)
    ib, iy0 = rng.integers(-8, 9, nrows), rng.integers(-8, 9, nrows)
    M = sp.csr_matrix((ivals.astype(np.float64), indices, indptr), shape=(nrows, ncols))
    ref = sp.csr_matrix((ivals.astype(np.int64), indices, indptr), shape=(nrows, ncols)) @ ix.astype(np.int64)
    assert np.abs(ref).max() > 0
    C = hip.Csr(ctx, M)
    try:
        dx, db = ctx.vec(ix.astype(np.float64)), ctx.vec(ib.astype(np.float64))
        for mode, alpha, want in ((0, 5.0, ref), (1, 3.0, ib - 3 * ref), (1, -2.0, ib + 2 * ref), (2, 5.0, iy0 + ref),
                                  (3, -3.0, -3 * ref)):
            dy = ctx.vec(iy0.astype(np.float64))
            C.mult(dx, dy, b=db if mode == 1 else None, alpha=alpha, mode=mode)
            assert np.array_equal(dy.get(), want), (kind, mode, alpha)
            assert np.array_equal(dx.get(), ix) and np.array_equal(db.get(), ib)
    finally:
        C.close()
    fvals, fx = rng.standard_normal(len(indices)), rng.standard_normal(ncols)
    M = sp.csr_matrix((fvals, indices, indptr), shape=(nrows, ncols))
    bound = (2 * np.diff(indptr).max() + 6) * 2.0 ** -53 * (abs(M) @ np.abs(fx)).max()
    C = hip.Csr(ctx, M)
    try:
        dy = ctx.vec(np.full(nrows, SENTINEL))
        C.mult(ctx.vec(fx), dy)
        err = np.abs(dy.get() - M @ fx).max()
        print("csr %s: error %.3e bound %.3e" % (kind, err, bound))
        assert err <= bound, (kind, err, bound)
    finally:
        C.close()
