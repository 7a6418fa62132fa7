"""CPU checks of the cases of tests/test_gpu_partitioned_product.py: from the dispatch rules restated in
tests/partitioned_product_cases.py (the whole-row packing of build_chunk_tables with its forced boundary, make_row_view's kbase /
nnzb / chunk_row, aligned / de-duplicated / plain), every case has the edge it is listed for and takes the kernel it is meant to
take, and the interior rows of the views cases hold owned columns only.  A case that stops exercising its edge fails here."""
import numpy as np
import pytest

from tests import partitioned_product_cases as pc

CHUNK = pc.SPMV_CHUNK


def _rowptr(name, nb_interior=None):
    return pc.structure(name, nb_interior)[1]


def test_every_operator_is_what_the_level_product_needs():
    """square, every block row non-empty, sorted distinct columns in range; the kernel of the upload; one partition list per case"""
    kernels = {"small": "aligned", "large": "dedup", "plain": "plain", "views-aligned": "aligned", "views-large": "dedup"}
    sizes = {"small": (256, 2041), "large": (1200, 3379), "plain": (324, 696), "views-aligned": (354, 3260), "views-large": (860, 3488)}
    assert set(pc.PARTITIONS) == set(kernels) == set(sizes)
    for name, nb_owned, nb_interior in pc.CASES:
        nb, rowptr, colidx = pc.structure(name, nb_interior)
        assert (nb, int(rowptr[-1])) == sizes[name] and len(rowptr) == nb + 1 and len(colidx) == rowptr[-1]
        assert np.diff(rowptr).min() >= 1 and colidx.min() >= 0 and colidx.max() < nb
        for i in range(nb):
            assert np.all(np.diff(colidx[rowptr[i]:rowptr[i + 1]]) > 0), (name, i)
        assert pc.upload_kernel(rowptr) == kernels[name]
        assert 0 < nb_owned <= nb
        sn = pc.send_nodes(name, nb_owned)
        assert len(sn) == nb - nb_owned and (len(sn) == 0 or (sn.min() >= 0 and sn.max() < nb_owned))
        # the ghost values matter: an owned row that the exchange has to serve holds a ghost column
        r0 = nb_interior if nb_interior is not None else 0
        if nb_owned < nb and r0 < nb_owned:
            assert colidx[rowptr[r0]:rowptr[nb_owned]].max() >= nb_owned, (name, nb_owned, nb_interior)
    # the rules themselves at their edges
    assert pc.upload_kernel(np.array([0, 256, 512])) == "aligned" and pc.upload_kernel(np.array([0, 257, 258])) == "plain"
    assert pc.upload_kernel(np.array([0, 257, 1023])) == "plain" and pc.upload_kernel(np.array([0, 257, 1024])) == "dedup"
    assert pc.upload_kernel(np.array([0, 256, 512, 768, 1024])) == "aligned"
    many = np.arange(0, (1 << 21) + 1, 256)                             # 2^21 blocks in rows of 256: the last aligned size
    assert pc.is_aligned(many) and not pc.is_aligned(np.append(many, many[-1] + 1))


def test_small_forced_and_natural_boundaries():
    """aligned A_own: the chunk table rebuilt with a boundary in front of the first ghost row"""
    rowptr = _rowptr("small")
    assert rowptr[:16].tolist() == [0, 200, 256, 257, 513, 768, 770, 833, 897, 962, 1092, 1218, 1258, 1288, 1308, 1318]
    natural, start, before = pc.chunk_tables(rowptr)
    assert natural == [0, 2, 3, 4, 5, 9, 11, 67, 152, 237] and before == -1
    assert np.diff(start).tolist() == [256, 1, 256, 255, 194, 256, 256, 255, 255, 57] and max(np.diff(start)) <= CHUNK
    #        nb_owned: (forced, chunks of A_own, chunks of the table, blocks of the last owned chunk)
    want = {1: (True, 1, 10, 200), 2: (False, 1, 10, 256), 3: (False, 2, 10, 1), 6: (True, 5, 11, 2), 7: (True, 5, 11, 65),
            256: (False, 10, 10, 57)}
    assert sorted(want) == sorted(o for o, _ in pc.PARTITIONS["small"])
    for nb_owned, (forced, nown, ntable, last) in want.items():
        chunk_row, start, before = pc.chunk_tables(rowptr, nb_owned)
        assert forced == (nb_owned < len(rowptr) - 1 and nb_owned not in natural)
        assert (before, len(chunk_row)) == (nown, ntable), nb_owned
        assert start[before] == rowptr[nb_owned] and start[before] - start[before - 1] == last     # A_own ends where the ghosts begin
        assert np.diff(start).max() <= CHUNK and np.diff(start).min() >= 1
        assert [int(rowptr[r]) for r in chunk_row] == start[:-1]                                   # whole rows
        if nb_owned < len(rowptr) - 1:
            assert chunk_row[before] == nb_owned
    # 65 blocks: the second wave iteration of the last owned chunk has one live lane; 1 and 2 blocks: one iteration, 1 / 2 lanes
    assert want[7][3] == 64 + 1


def test_large_and_plain_cuts_of_the_equal_chunk_kernels():
    """non-aligned A_own: the upload's kernel and chunks with the block count cut to nnz_own"""
    rowptr = _rowptr("large")
    assert rowptr[:9].tolist() == [0, 320, 384, 512, 768, 1023, 1024, 2124, 2187]
    #        nb_owned: (nnz_own, carry runs of the cut range)
    want = {5: (1023, [(0, 1)]), 6: (1024, [(0, 1)]), 7: (2124, [(0, 1), (6, 4)]), 8: (2187, [(0, 1), (6, 4)]),
            61: (2240, [(0, 1), (6, 4)]), 125: (2304, [(0, 1), (6, 4)]), 1200: (3379, [(0, 1), (6, 4)])}
    assert sorted(want) == sorted(o for o, _ in pc.PARTITIONS["large"])
    for nb_owned, (nnz_own, runs) in want.items():
        kbase, nnzb, chunk_row = pc.row_view(rowptr, 0, nb_owned)
        assert (kbase, nnzb) == (0, nnz_own) and pc.carry_runs(rowptr, 0, nnzb) == runs, nb_owned
        # the same chunks as the whole upload's, fewer of them
        assert chunk_row == pc.row_view(rowptr, 0, len(rowptr) - 1)[2][:len(chunk_row)]
    assert 1023 % 64 == 63 and 1023 % CHUNK == 255                      # lane 63 of the last iteration dead
    assert 1024 == pc.SPMV_WG                                          # exactly one group
    assert 2124 % CHUNK == 76 and 2124 % 64 == 12                      # the five-chunk row closed by the end of the range, mid-chunk
    assert (2124 - 1) // CHUNK - 1024 // CHUNK + 1 == 5
    assert 2187 % 64 == 11 and 2304 == 9 * CHUNK and 3379 % CHUNK == 51
    assert 2240 % 64 == 0 and 2240 % CHUNK == 192                      # the first block past the cut at lane 0 of a later iteration

    rowptr = _rowptr("plain")
    assert rowptr[:5].tolist() == [0, 300, 305, 375, 376] and np.all(np.diff(rowptr)[4:] == 1) and rowptr[-1] < pc.SPMV_WG
    want = {1: (300, 2, [(0, 1)]), 3: (375, 2, [(0, 1)]), 324: (696, 3, [(0, 1)])}
    assert sorted(want) == sorted(o for o, _ in pc.PARTITIONS["plain"])
    for nb_owned, (nnz_own, nchunks, runs) in want.items():
        kbase, nnzb, chunk_row = pc.row_view(rowptr, 0, nb_owned)
        assert (kbase, nnzb, len(chunk_row)) == (0, nnz_own, nchunks) and pc.carry_runs(rowptr, 0, nnzb) == runs


def _views(name, nb_owned, nb_interior):
    rowptr = _rowptr(name, nb_interior)
    vi, vb = pc.row_view(rowptr, 0, nb_interior), pc.row_view(rowptr, nb_interior, nb_owned)
    return rowptr, vi, vb, pc.carry_runs(rowptr, vi[0], vi[1]), pc.carry_runs(rowptr, vb[0], vb[1])


@pytest.mark.parametrize("name", ["views-aligned", "views-large"])
def test_interior_rows_hold_owned_columns_only(name):
    """what set_overlap verifies before it builds the views; and the row lengths do not depend on nb_interior"""
    for nb_owned, nb_interior in pc.PARTITIONS[name]:
        nb, rowptr, colidx = pc.structure(name, nb_interior)
        assert np.array_equal(rowptr, _rowptr(name, 0))
        assert 0 <= nb_interior <= nb_owned < nb
        assert nb_interior == 0 or colidx[:rowptr[nb_interior]].max() < nb_owned
        vi, vb = pc.row_view(rowptr, 0, nb_interior), pc.row_view(rowptr, nb_interior, nb_owned)
        assert vi[0] == 0 and vb[0] == vi[1] and vi[1] + vb[1] == rowptr[nb_owned]          # the two views tile the owned blocks
        for kbase, nnzb, chunk_row in (vi, vb):                                             # chunk_row: the row of a chunk's first block
            assert len(chunk_row) == -(-nnzb // CHUNK)
            for c, r in enumerate(chunk_row):
                assert rowptr[r] <= kbase + c * CHUNK < rowptr[r + 1]


def test_views_of_the_aligned_upload():
    name, nb_owned = "views-aligned", pc.VIEWS_ALIGNED_OWNED
    rowptr = _rowptr(name, 0)
    assert rowptr[nb_owned] == 3220 and rowptr[:15].tolist() == [0, 200, 400, 600, 800, 1000, 1200, 1263, 1264, 1456, 1520, 1720,
                                                                 1920, 2120, 2320]
    assert sorted(i for _, i in pc.PARTITIONS[name]) == [0, 1, 6, 12, nb_owned]
    _, vi, vb, ri, rb = _views(name, nb_owned, 0)
    assert vi[1] == 0 and vi[2] == [] and vb[:2] == (0, 3220)                            # interior view empty
    _, vi, vb, ri, rb = _views(name, nb_owned, nb_owned)
    assert vb[1] == 0 and vb[2] == [] and vi[:2] == (0, 3220)                            # boundary view empty
    _, vi, vb, ri, rb = _views(name, nb_owned, 1)
    assert vi == (0, 200, [0]) and ri == [] and vb[0] == 200 and 200 % 64 == 8           # one short chunk
    _, vi, vb, ri, rb = _views(name, nb_owned, 6)
    assert vb[0] == 1200 and 1200 % 64 == 48 and vi[1] == 1200
    # the 200-block rows cross the views' chunk boundaries: both views run a fix-up that the aligned upload never needs
    assert ri == [(1, 1), (2, 1), (3, 1), (5, 1)]
    assert rb[:3] == [(10, 1), (12, 1), (13, 1)] and 1200 + CHUNK == rowptr[9]           # (a view chunk that ends on a row start)
    assert pc.upload_kernel(rowptr) == "aligned"
    _, vi, vb, ri, rb = _views(name, nb_owned, 12)
    assert vb[0] == 1920 and 1920 % 64 == 0 and 1920 % CHUNK == 128 and rb[:2] == [(13, 1), (51, 1)]


def test_views_of_the_large_upload():
    name, nb_owned = "views-large", pc.VIEWS_LARGE_OWNED
    rowptr = _rowptr(name, 0)
    assert rowptr[:11].tolist() == [0, 63, 64, 256, 513, 768, 769, 1469, 1533, 1538, 1838] and rowptr[nb_owned] == 3438
    assert sorted(i for _, i in pc.PARTITIONS[name]) == [0, 1, 2, 3, 4, 7, nb_owned]
    _, vi, vb, ri, rb = _views(name, nb_owned, 0)
    assert vi[1] == 0 and vb[:2] == (0, 3438) and rb[:4] == [(3, 1), (6, 2), (8, 1), (9, 1)]
    _, vi, vb, ri, rb = _views(name, nb_owned, nb_owned)
    assert vb[1] == 0 and vi[:2] == (0, 3438)
    _, vi, vb, ri, rb = _views(name, nb_owned, 1)
    assert vb[0] == 63 and 63 % 64 == 63 and vi == (0, 63, [0]) and ri == []
    assert rb[:4] == [(3, 1), (4, 1), (6, 3), (9, 1)]                                    # the 700-block row: a carry run of three
    _, vi, vb, ri, rb = _views(name, nb_owned, 2)
    assert vb[0] == 64 and vi == (0, 64, [0]) and ri == []                               # exactly one wave iteration
    _, vi, vb, ri, rb = _views(name, nb_owned, 3)
    assert vb[0] == 256 and vi == (0, 256, [0]) and ri == []                             # exactly one full chunk
    _, vi, vb, ri, rb = _views(name, nb_owned, 4)
    assert vb[0] == 513 and 513 % 64 == 1 and vi[2] == [0, 3, 3] and ri == [(3, 1)]      # the 257-block row across a view chunk
    _, vi, vb, ri, rb = _views(name, nb_owned, 7)
    assert vb[0] == 1469 and 1469 % 64 == 61 and ri == [(3, 1), (6, 2)]                  # the 700-block row inside the interior view
    assert rb[0] == (9, 1)


def test_scalar_csr_cases_take_every_lane_width():
    assert (pc.csr_lanes(6, 1), pc.csr_lanes(601, 100), pc.csr_lanes(24, 1), pc.csr_lanes(2401, 100)) == (2, 8, 8, 32)
    assert sorted(set(pc.CSR_CASES.values())) == [2, 8, 32]
    for kind, lanes in pc.CSR_CASES.items():
        nrows, ncols, indptr, indices = pc.csr_structure(kind)
        lens = np.diff(indptr)
        assert pc.csr_lanes(int(indptr[-1]), nrows) == lanes, kind
        assert lens.min() == 0 and lens.max() > lanes                   # empty rows, rows longer than the lane group
        assert (nrows * lanes) % 256 != 0 and nrows * lanes > 256       # more than one workgroup, the last one part filled
        assert indices.min() >= 0 and indices.max() < ncols
        for i in range(nrows):
            assert np.all(np.diff(indices[indptr[i]:indptr[i + 1]]) > 0)
    assert pc.csr_structure("narrow-edge")[2][-1] == 6 * 130 and pc.csr_structure("mid-edge")[2][-1] == 24 * 40
