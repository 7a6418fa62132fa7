// C ABI of libalfi_hip.so (include/alfi_hip.h), block right-hand sides on a level: patch apply, product, residual and the FGMRES(k)
// smoother for the columns of a column-major operand (block_cols.h).  Serial levels only.
//
// Column c of every block result is the single-vector call's result on column c bit for bit.  A list of more than BLOCK_NV
// columns is taken BLOCK_NV at a time.  Where a level has a batched kernel (kernels_block.hip: dense inverses through
// patch_apply_kernel, the flat product) a chunk of two or more columns is ONE launch that streams the stored values once;
// condensed factors of at least COND_PER_PATCH_MIN patches (kernels_block_cond.hip), dense macro-star inverses of at least
// BIG_BLOCK_MIN_PATCHES patches (kernels_block_big.hip) and the de-duplicated product (kernels_block.hip) take a chunk in pieces
// of as many columns as fit the LDS budget (block_cond_width, block_big_width, block_dedup_width); everything else -- and every
// chunk or piece of one column -- is the single-vector code, column after column.  The smoother goes one of three ways
// (block_smooth_mode, block_cols.h): the general path in lockstep, the block form of the four-launch iteration
// (kernels_block_fused.hip), or whole single smoother calls column after column.
//
// Single call = one-column chunk.  The host drivers exist once, written for a chunk: the smoother's general path
// (smooth_fgmres_general, api_smoother.hip), the V- and the full cycle (api_cycles.hip) and the outer FGMRES (saddle_solve_chunk,
// api_saddle.hip).  The single entry points call them with one column on the level's or saddle's own workspace, the block entry
// points chunk after chunk on the block workspace -- two instances of one type (KrylovWs, krylov_ws.h), because captured cycles
// hold the addresses of the single one.  This file owns those workspaces and the slot buffers (SlotBuf): one ensure and one
// release per type, and the functions that say what is released when.
#include "api_internal.h"
#include "block_cols.h"

int alfi_ctx_set_block_kernels(alfi_ctx* ctx, int on) {
  if (!ctx) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL context");
  ctx->block_kernels = on != 0;
  return 0;
}
int alfi_ctx_set_block_fused(alfi_ctx* ctx, int on) {
  if (!ctx) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL context");
  ctx->block_fused = on != 0;
  return 0;
}

// ---- which way a level goes ----------------------------------------------------------------------------------------------------
// waves per patch of the batched apply of dense inverses, 0: the level holds none, or its apply loops
static int block_apply_waves(const alfi_level* L) {
  if (!L->ctx->block_kernels || !L->factored || L->jacobi || L->mult || level_is_partitioned(L)) return 0;
  if (L->held != HELD_F64 && L->held != HELD_F32) return 0;            // condensed factors: block_cond_apply_width
  const int W = patch_apply_dense_waves(L, L->held == HELD_F32);
  return patch_apply_block_waves_ok(W) ? W : 0;
}
// Condensed factors: the widest batch of the level (block_cond_width, block_cols.h), 0: its apply loops.  What batches is the
// workgroup-per-patch form (kernels_block_cond.hip): a level of fewer than COND_PER_PATCH_MIN patches takes the chunked form
// and loops; so does a level whose LDS does not fit two columns into the ctx's budget.
static int block_cond_apply_width(const alfi_level* L) {
  if (!L->ctx->block_kernels || !L->factored || L->jacobi || L->mult || level_is_partitioned(L)) return 0;
  if (L->held != HELD_COND || L->npatch < COND_PER_PATCH_MIN) return 0;
  if (L->lay.sum_n > INT32_MAX / BLOCK_NV) return 0;      // (piece_apply takes the stride between two columns' slots as an int)
  return block_cond_width(L->cplan.lds_front, L->cplan.lds_back, L->ctx->block_lds_bytes);
}
// Dense macro-star inverses (a patch above SMALL_PATCH_MAX dofs, FP64 or the single-precision copy: big_apply_kernel): the
// widest batch of the level (block_big_width, block_cols.h), 0: its apply loops -- levels of fewer than BIG_BLOCK_MIN_PATCHES
// patches, and levels whose x_p does not fit the ctx's budget twice.  (The few-patches detour of smaller stars through the same
// single kernel, patch_apply_dense_waves, loops as before.)
static int block_big_apply_width(const alfi_level* L) {
  if (!L->ctx->block_kernels || !L->factored || L->jacobi || L->mult || level_is_partitioned(L)) return 0;
  if (L->held != HELD_F64 && L->held != HELD_F32) return 0;
  if (L->lay.max_np <= SMALL_PATCH_MAX || L->npatch < BIG_BLOCK_MIN_PATCHES) return 0;
  if (L->lay.stage_len > INT32_MAX / BLOCK_NV) return 0;  // (piece_apply takes the stride between two columns' slots as an int)
  return block_big_width(L->lay.max_np, L->ctx->block_lds_bytes);
}
// the width of the levels that take a chunk in pieces: condensed factors or dense macro stars (a level holds one of the two)
static int block_piece_apply_width(const alfi_level* L) {
  return L->held == HELD_COND ? block_cond_apply_width(L) : block_big_apply_width(L);
}
// the widest batch of the level's apply: BLOCK_NV for dense inverses that batch, the condensed or macro-star width, 0: it loops
static int block_apply_width(const alfi_level* L) {
  return block_apply_waves(L) != 0 ? BLOCK_NV : block_piece_apply_width(L);
}
// the widest batch of the level's product: BLOCK_NV on flat and whole-row operators, what fits the ctx's LDS budget on
// de-duplicated ones (bsr_spmv_block_width, kernels_block.hip), 0: it loops
static int block_spmv_width(const alfi_level* L) {
  if (!L->ctx->block_kernels || level_is_partitioned(L)) return 0;
  const int w = bsr_spmv_block_width(L->A_own, L->ctx->block_lds_bytes);
  return w >= 2 ? w : 0;
}

int alfi_patch_apply_block_info(alfi_level* L, int* batched) {
  if (!L || !batched) return alfi_set_error(L ? L->ctx : nullptr, ALFI_E_ARG, "alfi_patch_apply_block_info: NULL argument");
  *batched = block_apply_width(L) >= 2 ? 1 : 0;
  return 0;
}
int alfi_patch_apply_block_width(alfi_level* L, int* width) {
  if (!L || !width) return alfi_set_error(L ? L->ctx : nullptr, ALFI_E_ARG, "alfi_patch_apply_block_width: NULL argument");
  *width = block_apply_width(L);
  return 0;
}
// LDS a workgroup of a block kernel may ask for -- one budget for the condensed apply, the macro stars' and the de-duplicated
// product (default 64 KiB: no launch needs its limit raised), clamped to what the device gives one workgroup
int alfi_ctx_set_block_lds_bytes(alfi_ctx* ctx, int64_t bytes) {
  if (!ctx) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL context");
  int limit = 0;
  ALFI_HIP_CHECK(ctx, hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  ctx->block_lds_bytes = (int)std::min<int64_t>(std::max<int64_t>(bytes, 0), limit);
  return 0;
}
// Which way alfi_smooth_fgmres_block(L, k, ...) goes on a chunk of two or more columns (block_smooth_mode, block_cols.h): the
// general path in lockstep (one block apply and one block product per iteration), the block form of the four-launch iteration,
// or a loop over whole smoother calls.
static bool level_applies_il(const alfi_level* L) { return L->il_valid && L->held == HELD_F64; }   // launch_patch_apply_range
static int block_smoother_mode(alfi_level* L, int k) {
  BlockSmoothFacts f;
  f.block_kernels = L->ctx->block_kernels;
  f.block_fused = L->ctx->block_fused;
  f.partitioned = level_is_partitioned(L);
  f.fused_iteration = smoother_takes_fused_iteration(L, k);
  f.applies_il = L->factored && level_applies_il(L);
  f.apply_waves = block_apply_waves(L);
  f.piece_width = block_piece_apply_width(L);
  return block_smooth_mode(f);
}
static bool block_smoother_lockstep(alfi_level* L, int k) { return block_smoother_mode(L, k) == BLOCK_SMOOTH_LOCKSTEP; }
int alfi_smooth_fgmres_block_mode(alfi_level* L, int k, int* mode) {
  if (!L || !mode || k < 1) return alfi_set_error(L ? L->ctx : nullptr, ALFI_E_ARG, "alfi_smooth_fgmres_block_mode: bad argument");
  *mode = block_smoother_mode(L, k);
  return 0;
}
int alfi_smooth_fgmres_block_info(alfi_level* L, int k, int* lockstep) {
  if (!L || !lockstep || k < 1) return alfi_set_error(L ? L->ctx : nullptr, ALFI_E_ARG, "alfi_smooth_fgmres_block_info: bad argument");
  *lockstep = block_smoother_lockstep(L, k) ? 1 : 0;
  return 0;
}
int alfi_spmv_block_info(alfi_level* L, int* batched) {
  if (!L || !batched) return alfi_set_error(L ? L->ctx : nullptr, ALFI_E_ARG, "alfi_spmv_block_info: NULL argument");
  *batched = block_spmv_width(L) >= 2 ? 1 : 0;
  return 0;
}
int alfi_spmv_block_width(alfi_level* L, int* width) {
  if (!L || !width) return alfi_set_error(L ? L->ctx : nullptr, ALFI_E_ARG, "alfi_spmv_block_width: NULL argument");
  *width = block_spmv_width(L);
  return 0;
}

// ---- the workspaces of the host drivers (krylov_ws.h) -----------------------------------------------------------------------
int krylov_ws_ensure(alfi_ctx* ctx, KrylovWs* ws, int slots, int K, int64_t n) {
  if (ws->K == K && ws->slots == slots) return 0;      // (n is fixed while the level or saddle lives)
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  krylov_ws_release(ws);
  ws->ldv = krylov_ldv(n);
  const KrylovWsDoubles d = krylov_ws_doubles(slots, K, ws->ldv);
  ALFI_CHECK(dev_alloc(ctx, &ws->V, d.V));
  ALFI_CHECK(dev_alloc(ctx, &ws->Z, d.Z));
  ALFI_CHECK(dev_alloc(ctx, &ws->w, d.w));
  ALFI_CHECK(dev_alloc(ctx, &ws->hs, d.hs));
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(ws->hs, 0, sizeof(double) * (size_t)d.hs, ctx->stream));
  ws->K = K;
  ws->slots = slots;
  return 0;
}
void krylov_ws_release(KrylovWs* ws) {
  dev_free(ws->V);
  dev_free(ws->Z);
  dev_free(ws->w);
  dev_free(ws->hs);
  *ws = KrylovWs();
}

int slot_buf_resize(alfi_ctx* ctx, SlotBuf* buf, int slots, int64_t per) {
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  slot_buf_release(buf);
  ALFI_CHECK(dev_alloc(ctx, &buf->p, slots * per));
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(buf->p, 0, sizeof(double) * (size_t)std::max<int64_t>(slots * per, 1), ctx->stream));
  buf->slots = slots;
  buf->per = per;
  return 0;
}
int slot_buf_ensure(alfi_ctx* ctx, SlotBuf* buf, int ncol, int64_t per) {
  const int need = slot_buf_needed(*buf, ncol);
  return need == buf->slots ? 0 : slot_buf_resize(ctx, buf, need, per);      // (0 slots: not allocated yet; ncol >= 1)
}
void slot_buf_release(SlotBuf* buf) {
  dev_free(buf->p);
  *buf = SlotBuf();
}

// the staging length and sum_n are the old patch set's: the next block apply allocates the two again
void block_release_patch_buffers(alfi_level* L) {
  slot_buf_release(&L->blk_stage);
  slot_buf_release(&L->blk_ctmp);
}
void release_workspaces(alfi_level* L) {
  block_release_patch_buffers(L);
  for (SlotBuf* b : {&L->blk_carry, &L->blk_part, &L->blk_mg_b, &L->blk_mg_x, &L->blk_mg_r}) slot_buf_release(b);
  krylov_ws_release(&L->ws);
  krylov_ws_release(&L->blk_ws);
}
void release_workspaces(alfi_saddle* S) {
  slot_buf_release(&S->blk_tmp_u);
  krylov_ws_release(&S->ws);
  krylov_ws_release(&S->blk_ws);
}

// the level's block Krylov workspace for a chunk of ncol columns: grow-only in slots, with the single workspace's K (the
// Hessenberg layout the kernels index with is HsLayout of it)
static int ensure_block_smoother(alfi_level* L, int ncol) {
  return krylov_ws_ensure(L->ctx, &L->blk_ws, block_slots_needed(L->blk_ws.slots, ncol), L->ws.K, L->n);
}

// ---- the block forms on one chunk (1 .. BLOCK_NV columns), unchecked --------------------------------------------------------------
// Y[:, oc[i]] = patch solves of X[:, ic[i]]
int block_patch_apply(alfi_level* L, const BlockCols& ic, const BlockCols& oc, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  alfi_ctx* ctx = L->ctx;
  ctx->cur_tag = L->id;
  const int W = ic.n > 1 ? block_apply_waves(L) : 0;
  if (W != 0) {
    ALFI_CHECK(slot_buf_ensure(ctx, &L->blk_stage, ic.n, L->lay.stage_len));
    return launch_patch_apply_block(L, W, ic, oc, X, ldx, Y, ldy, L->blk_stage.p);
  }
  // condensed factors, dense macro stars: the chunk in pieces of the level's width, a piece of one column through the single apply
  const int width = ic.n > 1 ? block_piece_apply_width(L) : 0;
  for (int k = 0; k < block_pieces(ic.n, width); ++k) {
    const BlockCols pi = block_piece(ic, width, k), po = block_piece(oc, width, k);
    if (pi.n == 1) {
      ALFI_CHECK(level_patch_apply(L, X + pi.c[0] * ldx, Y + po.c[0] * ldy));
      continue;
    }
    ALFI_CHECK(slot_buf_ensure(ctx, &L->blk_stage, pi.n, L->lay.stage_len));
    if (L->held != HELD_COND) {
      ALFI_CHECK(launch_big_apply_block(L, pi, po, X, ldx, Y, ldy, L->blk_stage.p));
      continue;
    }
    ALFI_CHECK(slot_buf_ensure(ctx, &L->blk_ctmp, pi.n, L->lay.sum_n));
    ALFI_CHECK(launch_cond_apply_block(L, pi, po, X, ldx, Y, ldy, L->blk_stage.p, L->blk_ctmp.p));
  }
  return 0;
}

// Y[:, oc[i]] = A X[:, ic[i]] (mode 0) or B[:, ic[i]] - A X[:, ic[i]] (mode 1)
int block_spmv(alfi_level* L, const BlockCols& ic, const BlockCols& oc, const double* X, int64_t ldx, double* Y, int64_t ldy,
               const double* B, int64_t ldb, int mode) {
  alfi_ctx* ctx = L->ctx;
  ctx->cur_tag = L->id;
  // the chunk in pieces of the product's width (BLOCK_NV: one piece), a piece of one column through the single product
  const int width = ic.n > 1 ? block_spmv_width(L) : 0;
  for (int k = 0; k < block_pieces(ic.n, width); ++k) {
    const BlockCols pi = block_piece(ic, width, k), po = block_piece(oc, width, k);
    if (pi.n == 1) {
      ALFI_CHECK(level_spmv(L, X + pi.c[0] * ldx, Y + po.c[0] * ldy, mode ? B + pi.c[0] * ldb : nullptr, mode));
      continue;
    }
    const DevBSR& A = L->A_own;
    if (!A.aligned) {
      const int64_t nchunks = (A.nnzb + SPMV_CHUNK - 1) / SPMV_CHUNK;
      ALFI_CHECK(slot_buf_ensure(ctx, &L->blk_carry, pi.n, nchunks * A.bs));
    }
    ProfScope prof(ctx, ALFI_EV_MATMULT);   // to the end of the piece
    ALFI_CHECK(launch_bsr_spmv_block(ctx, A, pi, po, X, ldx, Y, ldy, B, ldb, 1.0, mode, L->blk_carry.p));
  }
  return 0;
}

// alfi_smooth_fgmres on the columns of one chunk of 2 .. BLOCK_NV columns, on a level where the single call takes the four-launch
// iteration (smooth_fgmres_fused, api_smoother.hip) and stage 1 of the apply has a batched form: the same launches per
// iteration for all columns -- stage 1 (on condensed and macro-star levels: per piece of the level's width), sum + scale,
// product with dots, projection with norm partials.  ProfScope classes as in the single path.
static int block_smooth_fgmres_fused(alfi_level* L, int k, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx,
                                     int nonzero_guess) {
  alfi_ctx* ctx = L->ctx;
  const int nc = cols.n;
  ALFI_CHECK(ensure_block_smoother(L, nc));
  ALFI_CHECK(slot_buf_ensure(ctx, &L->blk_part, nc, block_partial_per_slot(RED_BLOCKS, RED_MAXV)));
  ALFI_CHECK(slot_buf_ensure(ctx, &L->blk_stage, nc, L->lay.stage_len));
  if (L->held == HELD_COND) ALFI_CHECK(slot_buf_ensure(ctx, &L->blk_ctmp, nc, L->lay.sum_n));
  const int64_t ldv = L->blk_ws.ldv;
  const BlockCols slots = block_chunk(nc, nullptr, 0);
  // r0 = b - A x, or x = 0 and r0 = b in the launch of the norm partials
  if (nonzero_guess) ALFI_CHECK(block_spmv(L, cols, slots, X, ldx, L->blk_ws.w, ldv, B, ldb, 1));
  {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_first_norm_block(L, cols, nonzero_guess ? nullptr : B, ldb, X, ldx));
  }
  const int G = red_blocks_for(L->n);
  const bool il = level_applies_il(L);
  const int W = il ? 0 : block_apply_waves(L), width = il || W != 0 ? BLOCK_NV : block_piece_apply_width(L);
  const double* stage[BLOCK_NV];
  for (int s = 0; s < BLOCK_NV; ++s) stage[s] = L->blk_stage.slot(s < nc ? s : 0);
  for (int j = 0; j < k; ++j) {
    // stage 1: slot s's staged patch solves of w_s
    if (il) {
      ALFI_CHECK(launch_patch_apply_il_block(L, nc, L->blk_ws.w, ldv, L->blk_stage.p));
    } else if (W != 0) {
      ALFI_CHECK(launch_patch_apply_block(L, W, slots, slots, L->blk_ws.w, ldv, nullptr, 0, L->blk_stage.p));
    } else {
      for (int q = 0; q < block_pieces(nc, width); ++q) {
        const BlockCols pi = block_piece(slots, width, q);
        double* st = L->blk_stage.slot(pi.c[0]);
        if (pi.n == 1) {      // (at most one piece of a chunk has one column: the single apply into the level's own buffer)
          ALFI_CHECK(launch_patch_apply_range(L, 0, L->npatch, L->blk_ws.wv(pi.c[0])));
          stage[pi.c[0]] = L->stage;
        } else if (L->held != HELD_COND) {
          ALFI_CHECK(launch_big_apply_block(L, pi, pi, L->blk_ws.w, ldv, nullptr, 0, st));
        } else {
          ALFI_CHECK(launch_cond_apply_block(L, pi, pi, L->blk_ws.w, ldv, nullptr, 0, st, L->blk_ctmp.p));
        }
      }
    }
    {
      ProfScope prof(ctx, ALFI_EV_PATCH_SCATTER);
      ALFI_CHECK(launch_patch_sum_scale_block(L, nc, stage, j == 0 ? 0 : 1, G, j));      // z_j, v_j, H column j-1
    }
    int nb = 0;
    {
      ProfScope prof(ctx, ALFI_EV_MATMULT);
      ALFI_CHECK(launch_bsr_spmv_dot_block(L, nc, j, &nb));                               // w = A z_j, V^T w partials
    }
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_multi_axpy_norm_block(L, nc, j, nb));                               // h, w -= V h, |w|^2 partials
  }
  ProfScope prof(ctx, ALFI_EV_BLAS1);   // to the end of the function
  return launch_fgmres_finish_update_block(L, cols, k, G, X, ldx);                        // H column k-1, y, x += Z y
}

// alfi_smooth_fgmres on the columns of one chunk, one of the three ways of block_smooth_mode; a chunk of one column is the
// single call.  LOCKSTEP is the single call's general path (smooth_fgmres_general, api_smoother.hip) on the block workspace.
int block_smooth_fgmres(alfi_level* L, int k, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx,
                        int nonzero_guess) {
  ALFI_CHECK(ensure_fgmres_workspace(L, k));
  L->ctx->cur_tag = L->id;
  const int mode = cols.n == 1 ? BLOCK_SMOOTH_LOOP : block_smoother_mode(L, k);
  if (mode == BLOCK_SMOOTH_FUSED) return block_smooth_fgmres_fused(L, k, cols, B, ldb, X, ldx, nonzero_guess);
  if (mode == BLOCK_SMOOTH_LOOP) {
    for (int i = 0; i < cols.n; ++i) ALFI_CHECK(alfi_smooth_fgmres(L, k, B + cols.c[i] * ldb, X + cols.c[i] * ldx, nonzero_guess));
    return 0;
  }
  ALFI_CHECK(ensure_block_smoother(L, cols.n));
  return smooth_fgmres_general(L, L->blk_ws, k, cols, B, ldb, X, ldx, nonzero_guess);
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------
// what every block call checks before it touches the device (L: the level whose vectors the operands' columns are)
int check_block_call(alfi_level* L, const char* what, int ncol, const int* cols, int nx, const BlockOperand* ops, int nops) {
  if (!L) return alfi_set_error(nullptr, ALFI_E_ARG, "%s: NULL level", what);
  if (level_is_partitioned(L)) return alfi_set_error(L->ctx, ALFI_E_ARG, "%s on a partitioned level (serial levels only)", what);
  return check_block_operands(L->ctx, what, L->n, ncol, cols, nx, ops, nops);
}
// the operands' part of it, for columns of n entries
int check_block_operands(alfi_ctx* ctx, const char* what, int64_t n, int ncol, const int* cols, int nx, const BlockOperand* ops,
                         int nops) {
  for (int a = 0; a < nops; ++a) {
    if (!ops[a].p) return alfi_set_error(ctx, ALFI_E_ARG, "%s: NULL operand", what);
    if (const char* err = block_operand_error(n, ncol, cols, nx, ops[a].ld)) return alfi_set_error(ctx, ALFI_E_ARG, "%s: %s", what, err);
  }
  for (int a = 0; a < nops; ++a)
    for (int b = 0; b < nops; ++b)
      if (a != b && ops[a].written && block_operands_overlap(ops[a].p, ops[a].ld, ops[b].p, ops[b].ld, nx, n))
        return alfi_set_error(ctx, ALFI_E_ARG, "%s: an operand that is written overlaps another one", what);
  return 0;
}

int alfi_patch_apply_block(alfi_level* L, int ncol, const int* cols, int nx, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  const BlockOperand ops[2] = {{X, ldx, false}, {Y, ldy, true}};
  ALFI_CHECK(check_block_call(L, "alfi_patch_apply_block", ncol, cols, nx, ops, 2));
  if (!level_pc_ready(L)) return alfi_set_error(L->ctx, ALFI_E_STATE, "alfi_patch_apply_block before alfi_patches_factor");
  for (int q = 0; q < block_chunks(ncol); ++q) {
    const BlockCols c = block_chunk(ncol, cols, q);
    ALFI_CHECK(block_patch_apply(L, c, c, X, ldx, Y, ldy));
  }
  return 0;
}

int alfi_spmv_block(alfi_level* L, int ncol, const int* cols, int nx, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  const BlockOperand ops[2] = {{X, ldx, false}, {Y, ldy, true}};
  ALFI_CHECK(check_block_call(L, "alfi_spmv_block", ncol, cols, nx, ops, 2));
  for (int q = 0; q < block_chunks(ncol); ++q) {
    const BlockCols c = block_chunk(ncol, cols, q);
    ALFI_CHECK(block_spmv(L, c, c, X, ldx, Y, ldy, nullptr, 0, 0));
  }
  return 0;
}

int alfi_residual_block(alfi_level* L, int ncol, const int* cols, int nx, const double* B, int64_t ldb, const double* X, int64_t ldx,
                        double* R, int64_t ldr) {
  const BlockOperand ops[3] = {{B, ldb, false}, {X, ldx, false}, {R, ldr, true}};
  ALFI_CHECK(check_block_call(L, "alfi_residual_block", ncol, cols, nx, ops, 3));
  for (int q = 0; q < block_chunks(ncol); ++q) {
    const BlockCols c = block_chunk(ncol, cols, q);
    ALFI_CHECK(block_spmv(L, c, c, X, ldx, R, ldr, B, ldb, 1));
  }
  return 0;
}

int alfi_smooth_fgmres_block(alfi_level* L, int k, int ncol, const int* cols, int nx, const double* B, int64_t ldb, double* X,
                             int64_t ldx, int nonzero_guess) {
  const BlockOperand ops[2] = {{B, ldb, false}, {X, ldx, true}};
  ALFI_CHECK(check_block_call(L, "alfi_smooth_fgmres_block", ncol, cols, nx, ops, 2));
  if (k < 1) return alfi_set_error(L->ctx, ALFI_E_ARG, "k must be >= 1");
  if (!level_pc_ready(L)) return alfi_set_error(L->ctx, ALFI_E_STATE, "alfi_smooth_fgmres_block before alfi_patches_factor");
  for (int q = 0; q < block_chunks(ncol); ++q)
    ALFI_CHECK(block_smooth_fgmres(L, k, block_chunk(ncol, cols, q), B, ldb, X, ldx, nonzero_guess));
  return 0;
}
