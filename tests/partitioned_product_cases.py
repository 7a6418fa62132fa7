"""Operators and partitions for the level product of a PARTITIONED level (level_spmv, csrc/api_level.hip), with the rules that
decide which kernel each of its three descriptors takes restated in Python.  Host only (numpy + alfi_amd.problem); shared by
tests/test_partitioned_product.py (which proves that every case has the edge it is listed for) and
tests/test_gpu_partitioned_product.py (which runs them).

A partitioned level forms its product from three descriptors of one upload:

A_own          block rows [0, nb_owned).  Aligned upload (every row <= 256 blocks, <= 2^21 blocks): the whole-row chunk table is
               rebuilt with a boundary forced in front of the first ghost row (chunk_tables(rowptr, break_row)) and cut to the
               chunks before it.  Otherwise the upload's own equal-chunk kernel -- de-duplicated from 1024 blocks, plain below --
               with the block count cut to nnz_own = rowptr[nb_owned], wherever in a chunk or a 64-block group that falls.
A_int, A_bnd   (set_overlap) rows [0, nb_interior) and [nb_interior, nb_owned) as equal chunks of 256 blocks counted from
               kbase = rowptr[r0] (row_view): never aligned, never de-duplicated, own carries and fix-up launch.

Every operator is a square BSR, every block row non-empty, columns sorted and distinct; the values come from the caller.

small          rows of 200, 56, 1, 256, 255, 2, 63, 64, 65, 130, 126, 40, 30, 20, 10 blocks, then 241 rows of 3 (256 rows, so that
               a row of 256 distinct columns exists; 2041 blocks), columns random over all rows.  Aligned.
large          block_dedup_cases.structure("pattern", "ragged"): rows start at 0, 320, 384, 512, 768, 1023, 1024, 2124, 2187, then
               rows of one block.  Equal chunks, de-duplicated.
plain          rows of 300, 5, 70, 1, then 320 rows of 1 (324 rows, 696 blocks): a row longer than a chunk but fewer than 1024
               blocks -- equal chunks WITHOUT de-duplication.  Also run unpartitioned.
views-aligned  rows of 200 x6, 63, 1, 192, 64, 200 x4, 300 rows of 3 (314 owned rows), 40 ghost rows of 1.  Aligned upload.
views-large    rows of 63, 1, 192, 257, 255, 1, 700, 64, 5, 300, 800 rows of 2 (810 owned rows), 50 ghost rows of 1.
               De-duplicated upload.
In the two views cases the rows in front of nb_interior draw their columns from the owned rows only (set_overlap verifies that
claim), every other row from all rows: the structure depends on nb_interior, the row lengths do not.

CSR_CASES: scalar CSR matrices for csr_spmv_kernel (hip.Csr.mult), one and more per lane width of launch_csr_spmv.
"""
import functools

import numpy as np

from tests import block_dedup_cases as dc

SPMV_CHUNK = dc.SPMV_CHUNK                 # csrc/common.h: blocks per wave
SPMV_WG = dc.SPMV_WG                       # blocks per workgroup (a de-duplication group)
SPMV_ALIGNED_MAX = 1 << 21                 # blocks; beyond, equal chunks whatever the rows

SMALL_ROWS = (200, 56, 1, 256, 255, 2, 63, 64, 65, 130, 126, 40, 30, 20, 10) + (3,) * 241
PLAIN_ROWS = (300, 5, 70, 1) + (1,) * 320
VIEWS_ALIGNED_ROWS = (200,) * 6 + (63, 1, 192, 64) + (200,) * 4 + (3,) * 300 + (1,) * 40
VIEWS_ALIGNED_OWNED = 314
VIEWS_LARGE_ROWS = (63, 1, 192, 257, 255, 1, 700, 64, 5, 300) + (2,) * 800 + (1,) * 50
VIEWS_LARGE_OWNED = 810

# name -> partitions (nb_owned, nb_interior or None: no set_overlap)
PARTITIONS = {
    "small": [(1, None), (2, None), (3, None), (6, None), (7, None), (256, None)],
    "large": [(5, None), (6, None), (7, None), (8, None), (61, None), (125, None), (1200, None)],
    "plain": [(1, None), (3, None), (324, None)],
    "views-aligned": [(VIEWS_ALIGNED_OWNED, i) for i in (0, VIEWS_ALIGNED_OWNED, 1, 6, 12)],
    "views-large": [(VIEWS_LARGE_OWNED, i) for i in (0, VIEWS_LARGE_OWNED, 1, 2, 3, 4, 7)],
}
CASES = [(name, nb_owned, nb_interior) for name, parts in PARTITIONS.items() for nb_owned, nb_interior in parts]


def _rows_structure(lens, seed, owned_only_before=0, nb_owned=None):
    """rowptr / colidx of rows of these lengths: sorted distinct random columns, over [0, nb_owned) for the rows in front of
    ``owned_only_before``, over all rows otherwise"""
    nb = len(lens)
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(nb_owned if i < owned_only_before else nb, m, replace=False)) for i, m in enumerate(lens)]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate(rows).astype(np.int32)
    rowptr.setflags(write=False)
    colidx.setflags(write=False)
    return nb, rowptr, colidx


@functools.lru_cache(maxsize=None)
def structure(name, nb_interior=None):
    """(nb, rowptr int32, colidx int32); nb_interior matters for the views cases only"""
    if name == "small":
        return _rows_structure(SMALL_ROWS, 11)
    if name == "large":
        return dc.structure("pattern", "ragged")
    if name == "plain":
        return _rows_structure(PLAIN_ROWS, 12)
    if name == "views-aligned":
        return _rows_structure(VIEWS_ALIGNED_ROWS, 13, int(nb_interior or 0), VIEWS_ALIGNED_OWNED)
    if name == "views-large":
        return _rows_structure(VIEWS_LARGE_ROWS, 14, int(nb_interior or 0), VIEWS_LARGE_OWNED)
    raise KeyError(name)


def operator(name, nb_interior, bs, vals):
    """the BSR with the caller's values, an (nnzb, bs, bs) array"""
    from alfi_amd.problem import BSR
    nb, rowptr, colidx = structure(name, nb_interior)
    assert vals.shape == (len(colidx), bs, bs)
    return BSR(nb, nb, bs, rowptr, colidx, vals)


def send_nodes(name, nb_owned):
    """the self-exchange: ghost g receives owned node send_nodes[g] (one entry per ghost row)"""
    nb = structure(name, 0)[0]
    return np.random.default_rng(1000 + nb_owned).integers(0, nb_owned, nb - nb_owned).astype(np.int32)


# ---- the dispatch rules (csrc/api_ctx.hip: build_chunk_tables; kernels_vec.hip: build_spmv_dedup, launch_bsr_spmv_bs) ------------
def is_aligned(rowptr):
    return int(rowptr[-1]) <= SPMV_ALIGNED_MAX and int(np.diff(rowptr).max()) <= SPMV_CHUNK


def upload_kernel(rowptr):
    """'aligned' (whole-row chunks, one launch), 'dedup' or 'plain' (equal chunks + fix-up, with / without staged gathers)"""
    if is_aligned(rowptr):
        return "aligned"
    return "dedup" if dc.dedups(rowptr) else "plain"


def chunk_tables(rowptr, break_row=-1):
    """build_chunk_tables on an aligned operator: greedy packing of whole rows into chunks of <= 256 blocks, a boundary forced in
    front of break_row.  (chunk_row, chunk_start with the end appended, number of chunks in front of break_row or -1)"""
    nbrows = len(rowptr) - 1
    chunk_row, start, before = [], [], -1
    i = 0
    while i < nbrows:
        start.append(int(rowptr[i]))
        chunk_row.append(i)
        if i == break_row:
            before = len(start) - 1
        e = i
        while e < nbrows and rowptr[e + 1] - rowptr[i] <= SPMV_CHUNK and (e == i or e != break_row):
            e += 1
        i = e
    if break_row >= nbrows:
        before = len(start)
    start.append(int(rowptr[nbrows]))
    return chunk_row, start, before


def row_view(rowptr, r0, r1):
    """make_row_view: (kbase, nnzb, chunk_row) of block rows [r0, r1) as equal chunks counted from kbase = rowptr[r0]; with
    r0 = 0 and r1 the owned rows also the cut equal-chunk A_own"""
    kbase, nnzb = int(rowptr[r0]), int(rowptr[r1] - rowptr[r0])
    chunk_row, row = [], r0
    for c in range(-(-nnzb // SPMV_CHUNK)):
        k = kbase + c * SPMV_CHUNK
        while rowptr[row + 1] <= k:
            row += 1
        chunk_row.append(row)
    return kbase, nnzb, chunk_row


def carry_runs(rowptr, kbase, nnzb):
    """the fix-up's work on blocks [kbase, kbase + nnzb) in equal chunks: [(row, number of consecutive chunks that leave a carry
    for it)], in chunk order.  A chunk leaves a carry when blocks of the range follow it and the first of them starts no row."""
    starts = set(int(r) for r in rowptr)
    runs = []
    prev = None
    for c in range(-(-nnzb // SPMV_CHUNK)):
        kend = kbase + (c + 1) * SPMV_CHUNK
        row = None
        if kend < kbase + nnzb and kend not in starts:
            row = int(np.searchsorted(rowptr, kend - 1, side="right")) - 1
        if row is not None:
            if prev == row:
                runs[-1] = (row, runs[-1][1] + 1)
            else:
                runs.append((row, 1))
        prev = row
    return runs


# ---- scalar CSR (kernels_vec.hip: launch_csr_spmv) --------------------------------------------------------------------------
def csr_lanes(nnz, nrows):
    """lanes per row of csr_spmv_kernel: by the average row length"""
    avg = nnz / nrows
    return 32 if avg > 24 else (8 if avg > 6 else 2)


def _csr_lens(kind):
    rng = np.random.default_rng(21)
    if kind == "narrow":                   # 301 rows x 2 lanes = 602 threads: three workgroups, the last one part filled
        lens = rng.integers(1, 9, 301)
        lens[[0, 5, 300]] = 0
        lens[17] = 40                      # 20 passes of the lane pair
    elif kind == "narrow-edge":            # average exactly 6: still two lanes
        lens = np.full(130, 6)
        lens[0], lens[1] = 0, 12
    elif kind == "mid":                    # 70 rows x 8 lanes = 560 threads
        lens = rng.integers(7, 21, 70)
        lens[[3, 69]] = 0
        lens[40] = 100
    elif kind == "mid-edge":               # average exactly 24: still eight lanes
        lens = np.full(40, 24)
        lens[0], lens[1] = 0, 48
    elif kind == "wide":                   # 19 rows x 32 lanes = 608 threads
        lens = rng.integers(30, 61, 19)
        lens[[0, 18]] = 0
        lens[7] = 150                      # five passes of the lane group, the last of 22 lanes
        lens[8] = 33                       # one lane in the second pass
    else:
        raise KeyError(kind)
    return lens.astype(np.int64)


CSR_CASES = {"narrow": 2, "narrow-edge": 2, "mid": 8, "mid-edge": 8, "wide": 32}     # kind -> lanes per row
CSR_NCOLS = 160


@functools.lru_cache(maxsize=None)
def csr_structure(kind):
    """(nrows, ncols, indptr, indices): sorted distinct random columns"""
    lens = _csr_lens(kind)
    rng = np.random.default_rng(22)
    indices = np.concatenate([np.sort(rng.choice(CSR_NCOLS, m, replace=False)) for m in lens] + [np.zeros(0, dtype=np.int64)])
    indptr = np.concatenate([[0], np.cumsum(lens)])
    return len(lens), CSR_NCOLS, indptr.astype(np.int32), indices.astype(np.int32)
