// Block right-hand sides (alfi_*_block, include/alfi_hip.h): the arithmetic of column lists, chunks and lazily grown workspaces.
// Host only, no HIP: api_block.hip includes it, and so can a stand-alone program built with host sanitizers.
//
// A block operand is column-major: column c of X is X + c * ldx, ldx >= n and even (16-byte aligned columns), nx columns in all.
// A call names the columns it works on -- cols[0 .. ncol), distinct entries of [0, nx); NULL = 0, 1, ..., ncol - 1 -- so that a
// caller drops converged columns without moving data.  One launch takes at most BLOCK_NV columns: a longer list is cut into
// chunks of BLOCK_NV, the last one shorter.
#pragma once
#include <cstdint>

constexpr int BLOCK_NV = 4;      // right-hand sides per stream of the stored values (piece_dot, row_piece.h)

// the columns of one launch: a kernel argument, passed by value
struct BlockCols {
  int n;
  int c[BLOCK_NV];
};

// NULL when (n, ncol, cols, nx, ldx) describe a block operand, else what is wrong with them
inline const char* block_operand_error(int64_t n, int ncol, const int* cols, int nx, int64_t ldx) {
  if (ncol < 1) return "ncol < 1";
  if (nx < ncol) return "more columns listed than the operand has";
  if (ldx < n) return "leading dimension below the vector length";
  if (ldx & 1) return "odd leading dimension";
  if (!cols) return nullptr;
  for (int i = 0; i < ncol; ++i) {
    if (cols[i] < 0 || cols[i] >= nx) return "column index out of range";
    for (int j = 0; j < i; ++j)
      if (cols[j] == cols[i]) return "column listed twice";
  }
  return nullptr;
}

// do the column-major operands X (ldx) and Y (ldy), nx columns of n entries each, share a byte?
inline bool block_operands_overlap(const double* X, int64_t ldx, const double* Y, int64_t ldy, int nx, int64_t n) {
  if (nx < 1 || n < 1) return false;
  const uintptr_t x0 = (uintptr_t)X, x1 = x0 + sizeof(double) * (size_t)((nx - 1) * ldx + n);
  const uintptr_t y0 = (uintptr_t)Y, y1 = y0 + sizeof(double) * (size_t)((nx - 1) * ldy + n);
  return x0 < y1 && y0 < x1;
}

// chunks of a list of ncol columns
inline int block_chunks(int ncol) { return (ncol + BLOCK_NV - 1) / BLOCK_NV; }

// chunk k of the list (cols NULL: the identity list): the columns [BLOCK_NV k, min(ncol, BLOCK_NV (k + 1)))
inline BlockCols block_chunk(int ncol, const int* cols, int k) {
  BlockCols b;
  const int first = k * BLOCK_NV;
  b.n = ncol - first < BLOCK_NV ? ncol - first : BLOCK_NV;
  if (b.n < 0) b.n = 0;
  for (int i = 0; i < BLOCK_NV; ++i) {
    const int q = first + (i < b.n ? i : 0);          // unused slots repeat the chunk's first column: always a valid index
    b.c[i] = b.n == 0 ? 0 : cols ? cols[q] : q;
  }
  return b;
}

// A per-level workspace that holds `have` column slots and is asked to serve a call of ncol columns: the slots it has to hold
// afterwards.  Grow-only, never more than one chunk.
inline int block_slots_needed(int have, int ncol) {
  const int want = ncol < BLOCK_NV ? ncol : BLOCK_NV;
  return want > have ? want : have;
}

// ---- levels whose batch is narrower than a chunk (condensed factors: the LDS of a workgroup holds NV copies of its operands) ----
// The widest batch of the condensed apply whose one-vector kernels ask for lds_front / lds_back bytes of LDS: the largest NV of
// 4, 3, 2 with NV * max(lds_front, lds_back) <= budget_bytes; 0: not even two columns fit, the level loops.
inline int block_cond_width(int64_t lds_front, int64_t lds_back, int64_t budget_bytes) {
  const int64_t per = lds_front > lds_back ? lds_front : lds_back;
  if (per <= 0 || budget_bytes <= 0) return 0;
  for (int nv = BLOCK_NV; nv >= 2; --nv)
    if (nv * per <= budget_bytes) return nv;
  return 0;
}

// ---- dense macro-star inverses (patches above SMALL_PATCH_MAX dofs; kernels_block_big.hip) -------------------------------------
// The block form of big_apply_kernel keeps x_p of its nv columns in dynamic LDS, interleaved entry by entry and sized by the
// level's largest patch (rounded up to even), not by the largest patch there can be:
inline int64_t block_big_lds(int max_np, int nv) { return (int64_t)nv * 8 * ((max_np + 1) & ~1); }
// The widest batch of such a level: the largest nv of 4, 3, 2 with block_big_lds(max_np, nv) <= budget_bytes (the ctx's
// block_lds_bytes, the same budget as the condensed apply's); 0: not even two columns fit, the level loops.  At the default
// 64 KiB: max_np <= 2048 gives 4, <= 2730 gives 3, <= 4096 gives 2.
inline int block_big_width(int max_np, int64_t budget_bytes) {
  if (max_np <= 0 || budget_bytes <= 0) return 0;
  for (int nv = BLOCK_NV; nv >= 2; --nv)
    if (block_big_lds(max_np, nv) <= budget_bytes) return nv;
  return 0;
}
// Macro-star levels of fewer patches than this loop the single apply.  The one reason: tests/test_gpu_block_rhs.py
// (test_looped_applies_are_the_single_apply) pins that a level of 4 patches with one of 161 dofs reports "not batched", and
// existing tests do not change; 8 is the smallest level the block kernel is tested on.  Nothing about speed was measured for it.
constexpr int64_t BIG_BLOCK_MIN_PATCHES = 8;

// ---- the de-duplicated level product (operators whose single product is bsr_spmv_dedup_kernel; kernels_block.hip) -------------
// The block form stages the distinct x entries of a workgroup's group of blocks for its nv columns in dynamic LDS, bs doubles per
// entry and column, sized by the operator's fullest group (max_uniq distinct columns, at most the 1024 blocks of a group):
inline int64_t block_dedup_lds(int max_uniq, int bs, int nv) { return (int64_t)nv * 8 * bs * max_uniq; }
// The widest batch of such an operator: the largest nv of 4, 3, 2 with block_dedup_lds(max_uniq, bs, nv) <= budget_bytes (the
// ctx's block_lds_bytes, the budget of the applies above); 0: not even two columns fit, the product loops.  At the default
// 64 KiB: bs 2 always gives 4; bs 3 gives 4 up to 682 distinct columns, 3 up to 910, 2 up to 1024 (always).
inline int block_dedup_width(int max_uniq, int bs, int64_t budget_bytes) {
  if (max_uniq <= 0 || bs <= 0 || budget_bytes <= 0) return 0;
  for (int nv = BLOCK_NV; nv >= 2; --nv)
    if (block_dedup_lds(max_uniq, bs, nv) <= budget_bytes) return nv;
  return 0;
}

// A chunk of b.n columns on a level of batch width `width` is taken in pieces of at most `width` columns, the last one shorter
// (a width below 2: a column at a time).  A piece of one column is the single-vector path.
inline int block_piece_width(int width) { return width < 1 ? 1 : width > BLOCK_NV ? BLOCK_NV : width; }
inline int block_pieces(int n, int width) {
  const int w = block_piece_width(width);
  return n < 1 ? 0 : (n + w - 1) / w;
}
// piece k of the chunk: its columns [w k, min(b.n, w (k + 1))); unused slots repeat the piece's first column
inline BlockCols block_piece(const BlockCols& b, int width, int k) {
  const int w = block_piece_width(width), first = k * w;
  BlockCols q;
  q.n = b.n - first < w ? b.n - first : w;
  if (q.n < 0 || k < 0) q.n = 0;
  for (int i = 0; i < BLOCK_NV; ++i) q.c[i] = q.n == 0 ? b.c[0] : b.c[first + (i < q.n ? i : 0)];
  return q;
}

// ---- the FGMRES(k) smoother on a chunk of 2 .. BLOCK_NV columns (alfi_smooth_fgmres_block; api_block.hip) ----------------------
// Three ways.  LOOP: whole single smoother calls, column after column.  LOCKSTEP: the general path of the single call with one
// block apply and one block product per iteration.  FUSED: the block form of the four-launch iteration (kernels_block_fused.hip)
// -- as many launches per iteration as one column takes.
enum BlockSmoothMode { BLOCK_SMOOTH_LOOP = 0, BLOCK_SMOOTH_LOCKSTEP = 1, BLOCK_SMOOTH_FUSED = 2 };
// what the rule reads of a level, its ctx and k
struct BlockSmoothFacts {
  bool block_kernels;      // alfi_ctx_set_block_kernels
  bool block_fused;        // alfi_ctx_set_block_fused
  bool partitioned;        // the level is partitioned
  bool fused_iteration;    // the single call takes the four-launch iteration (smoother_takes_fused_iteration)
  bool applies_il;         // stage 1 of the level's apply streams the interleaved copy of small-patch inverses
  int apply_waves;         // waves per patch of the batched apply of dense inverses, 0: none (block_apply_waves)
  int piece_width;         // the widest batch of condensed factors or dense macro stars, 0: their apply loops
};
// Where the single call takes the general path the chunk goes in lockstep.  Where it takes the four-launch iteration the chunk
// takes its block form if stage 1 of the level's apply has a batched form -- the interleaved copy, dense inverses through
// patch_apply_block_kernel, or condensed factors / macro stars in pieces of at least two columns -- and loops otherwise
// (condensed levels in the chunked form, macro-star levels of fewer than BIG_BLOCK_MIN_PATCHES patches, the few-patches detour).
inline int block_smooth_mode(const BlockSmoothFacts& f) {
  if (!f.block_kernels || f.partitioned) return BLOCK_SMOOTH_LOOP;
  if (!f.fused_iteration) return BLOCK_SMOOTH_LOCKSTEP;
  if (!f.block_fused) return BLOCK_SMOOTH_LOOP;
  return f.applies_il || f.apply_waves != 0 || f.piece_width >= 2 ? BLOCK_SMOOTH_FUSED : BLOCK_SMOOTH_LOOP;
}
// The reduction partials of the block fused iteration: per column slot two sets (the dot partials are still being read while the
// norm partials are written) of red_blocks rows of red_maxv doubles each -- the ctx's red_partial and red_partial2, once per slot.
inline int64_t block_partial_set(int red_blocks, int red_maxv) { return (int64_t)red_blocks * red_maxv; }
inline int64_t block_partial_per_slot(int red_blocks, int red_maxv) { return 2 * block_partial_set(red_blocks, red_maxv); }
// Dot vectors of an instantiation of the product with dots: j + 1 rounded up to 4, 8 or 16 (a guard skips the rest), 0: too many
inline int block_dot_vectors(int nvec) { return nvec < 1 || nvec > 16 ? 0 : nvec <= 4 ? 4 : nvec <= 8 ? 8 : 16; }
