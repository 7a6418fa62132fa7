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

// ---- lazily grown workspaces ---------------------------------------------------------------------------------------------------
// *buf holds *slots column slots of `per` doubles (0 slots: not allocated yet) and is asked to serve ncol >= 1 columns
// (block_slots_needed: grow-only).  `per` is fixed while the buffer lives: the staging length until the next alfi_patches_set,
// which frees blk_stage and blk_ctmp; the chunk count of the level's operator, which is set at alfi_level_create for good.
static int grow_slots(alfi_ctx* ctx, double** buf, int* slots, int ncol, int64_t per) {
  const int need = block_slots_needed(*slots, ncol);
  if (need == *slots) return 0;
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  dev_free(*buf);
  *buf = nullptr;
  *slots = 0;
  ALFI_CHECK(dev_alloc(ctx, buf, need * per));
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(*buf, 0, sizeof(double) * (size_t)std::max<int64_t>(need * per, 1), ctx->stream));
  *slots = need;
  return 0;
}

void free_block_smoother(alfi_level* L) {
  dev_free(L->blk_V);
  dev_free(L->blk_Z);
  dev_free(L->blk_w);
  dev_free(L->blk_hs);
  dev_free(L->blk_part);
  L->blk_V = L->blk_Z = L->blk_w = L->blk_hs = L->blk_part = nullptr;
  L->blk_kmax = L->blk_ws_slots = L->blk_part_slots = 0;
}

// one Krylov workspace per slot, with the level's own kmax (the Hessenberg layout the kernels index with is HsLayout(kmax))
static int ensure_block_smoother(alfi_level* L, int ncol) {
  alfi_ctx* ctx = L->ctx;
  const int need = block_slots_needed(L->blk_ws_slots, ncol), K = L->kmax;
  if (L->blk_kmax == K && need == L->blk_ws_slots) return 0;     // (0 slots: not allocated yet)
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  free_block_smoother(L);
  HsLayout hl(K);
  ALFI_CHECK(dev_alloc(ctx, &L->blk_V, (int64_t)need * (K + 1) * L->ldv));
  ALFI_CHECK(dev_alloc(ctx, &L->blk_Z, (int64_t)need * K * L->ldv));
  ALFI_CHECK(dev_alloc(ctx, &L->blk_w, (int64_t)need * L->ldv));
  ALFI_CHECK(dev_alloc(ctx, &L->blk_hs, (int64_t)need * hl.total));
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->blk_hs, 0, sizeof(double) * (size_t)need * hl.total, ctx->stream));
  L->blk_kmax = K;
  L->blk_ws_slots = need;
  return 0;
}

// ---- the block forms on one chunk (1 .. BLOCK_NV columns), unchecked --------------------------------------------------------------
// Y[:, oc[i]] = patch solves of X[:, ic[i]]
int block_patch_apply(alfi_level* L, const BlockCols& ic, const BlockCols& oc, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  alfi_ctx* ctx = L->ctx;
  ctx->cur_tag = L->id;
  const int W = ic.n > 1 ? block_apply_waves(L) : 0;
  if (W != 0) {
    ALFI_CHECK(grow_slots(ctx, &L->blk_stage, &L->blk_stage_slots, ic.n, L->lay.stage_len));
    return launch_patch_apply_block(L, W, ic, oc, X, ldx, Y, ldy, L->blk_stage);
  }
  // condensed factors, dense macro stars: the chunk in pieces of the level's width, a piece of one column through the single apply
  const int width = ic.n > 1 ? block_piece_apply_width(L) : 0;
  for (int k = 0; k < block_pieces(ic.n, width); ++k) {
    const BlockCols pi = block_piece(ic, width, k), po = block_piece(oc, width, k);
    if (pi.n == 1) {
      ALFI_CHECK(level_patch_apply(L, X + pi.c[0] * ldx, Y + po.c[0] * ldy));
      continue;
    }
    ALFI_CHECK(grow_slots(ctx, &L->blk_stage, &L->blk_stage_slots, pi.n, L->lay.stage_len));
    if (L->held != HELD_COND) {
      ALFI_CHECK(launch_big_apply_block(L, pi, po, X, ldx, Y, ldy, L->blk_stage));
      continue;
    }
    ALFI_CHECK(grow_slots(ctx, &L->blk_ctmp, &L->blk_ctmp_slots, pi.n, L->lay.sum_n));
    ALFI_CHECK(launch_cond_apply_block(L, pi, po, X, ldx, Y, ldy, L->blk_stage, L->blk_ctmp));
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
      ALFI_CHECK(grow_slots(ctx, &L->blk_carry, &L->blk_carry_slots, pi.n, nchunks * A.bs));
    }
    ProfScope prof(ctx, ALFI_EV_MATMULT);   // to the end of the piece
    ALFI_CHECK(launch_bsr_spmv_block(ctx, A, pi, po, X, ldx, Y, ldy, B, ldb, 1.0, mode, L->blk_carry));
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
  ALFI_CHECK(grow_slots(ctx, &L->blk_part, &L->blk_part_slots, nc, block_partial_per_slot(RED_BLOCKS, RED_MAXV)));
  ALFI_CHECK(grow_slots(ctx, &L->blk_stage, &L->blk_stage_slots, nc, L->lay.stage_len));
  if (L->held == HELD_COND) ALFI_CHECK(grow_slots(ctx, &L->blk_ctmp, &L->blk_ctmp_slots, nc, L->lay.sum_n));
  const int64_t ldv = L->ldv;
  const BlockCols slots = block_chunk(nc, nullptr, 0);
  // r0 = b - A x, or x = 0 and r0 = b in the launch of the norm partials
  if (nonzero_guess) ALFI_CHECK(block_spmv(L, cols, slots, X, ldx, L->blk_w, ldv, B, ldb, 1));
  {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_first_norm_block(L, cols, nonzero_guess ? nullptr : B, ldb, X, ldx));
  }
  const int G = red_blocks_for(L->n);
  const bool il = level_applies_il(L);
  const int W = il ? 0 : block_apply_waves(L), width = il || W != 0 ? BLOCK_NV : block_piece_apply_width(L);
  const double* stage[BLOCK_NV];
  for (int s = 0; s < BLOCK_NV; ++s) stage[s] = L->blk_stage + (s < nc ? s : 0) * L->lay.stage_len;
  for (int j = 0; j < k; ++j) {
    // stage 1: slot s's staged patch solves of w_s
    if (il) {
      ALFI_CHECK(launch_patch_apply_il_block(L, nc, L->blk_w, ldv, L->blk_stage));
    } else if (W != 0) {
      ALFI_CHECK(launch_patch_apply_block(L, W, slots, slots, L->blk_w, ldv, nullptr, 0, L->blk_stage));
    } else {
      for (int q = 0; q < block_pieces(nc, width); ++q) {
        const BlockCols pi = block_piece(slots, width, q);
        double* st = L->blk_stage + pi.c[0] * L->lay.stage_len;
        if (pi.n == 1) {      // (at most one piece of a chunk has one column: the single apply into the level's own buffer)
          ALFI_CHECK(launch_patch_apply_range(L, 0, L->npatch, L->blk_w + pi.c[0] * ldv));
          stage[pi.c[0]] = L->stage;
        } else if (L->held != HELD_COND) {
          ALFI_CHECK(launch_big_apply_block(L, pi, pi, L->blk_w, ldv, nullptr, 0, st));
        } else {
          ALFI_CHECK(launch_cond_apply_block(L, pi, pi, L->blk_w, ldv, nullptr, 0, st, L->blk_ctmp));
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

// alfi_smooth_fgmres on the columns of one chunk: the general path of api_smoother.hip in lockstep -- slot s of the block
// workspace belongs to column cols.c[s]; per iteration ONE block apply and ONE block product for all slots, the BLAS-1 and
// Hessenberg launches slot by slot (each slot's chain of launches, which hands its reduction partials from one launch to the
// next through the ctx's two partial buffers, is finished before the next slot's begins).  Levels on which the single call
// takes the four-launch iteration take its block form above, or are smoothed column by column (block_smooth_mode).
int block_smooth_fgmres(alfi_level* L, int k, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx,
                        int nonzero_guess) {
  alfi_ctx* ctx = L->ctx;
  ALFI_CHECK(ensure_fgmres_workspace(L, k));
  ctx->cur_tag = L->id;
  const int mode = cols.n == 1 ? BLOCK_SMOOTH_LOOP : block_smoother_mode(L, k);
  if (mode == BLOCK_SMOOTH_FUSED) return block_smooth_fgmres_fused(L, k, cols, B, ldb, X, ldx, nonzero_guess);
  if (mode == BLOCK_SMOOTH_LOOP) {
    for (int i = 0; i < cols.n; ++i) ALFI_CHECK(alfi_smooth_fgmres(L, k, B + cols.c[i] * ldb, X + cols.c[i] * ldx, nonzero_guess));
    return 0;
  }
  ALFI_CHECK(ensure_block_smoother(L, cols.n));
  const int K = L->kmax, nc = cols.n;
  const int64_t n = L->n, ldv = L->ldv, vs = (int64_t)(K + 1) * ldv, zs = (int64_t)K * ldv;
  HsLayout hl(K);
  const BlockCols slots = block_chunk(nc, nullptr, 0);
  auto Vs = [&](int s) { return L->blk_V + s * vs; };
  auto Zs = [&](int s) { return L->blk_Z + s * zs; };
  auto ws = [&](int s) { return L->blk_w + s * ldv; };
  auto hss = [&](int s) { return L->blk_hs + (int64_t)s * hl.total; };
  // r0 = b - A x, beta = |r0|, v0 = r0 / beta
  if (nonzero_guess) {
    ALFI_CHECK(block_spmv(L, cols, slots, X, ldx, L->blk_w, ldv, B, ldb, 1));
  } else {
    for (int s = 0; s < nc; ++s) {
      ALFI_HIP_CHECK(ctx, hipMemsetAsync(X + cols.c[s] * ldx, 0, sizeof(double) * n, ctx->stream));
      ProfScope prof(ctx, ALFI_EV_BLAS1);
      ALFI_CHECK(launch_copy(ctx, ws(s), B + cols.c[s] * ldb, n));
    }
  }
  const int G = red_blocks_for(n);
  const bool fused = G <= 256 && k + 1 <= 16;      // the consumer of a reduced value sums the partials itself (api_smoother.hip)
  for (int s = 0; s < nc; ++s) {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_norm_partials(ctx, ws(s), n));
    ALFI_CHECK(launch_norm_init_finish(ctx, ctx->red_partial, G, hss(s), K));
    ALFI_CHECK(launch_scale_by_inv(ctx, Vs(s), ws(s), hss(s) + hl.beta, n));
  }
  for (int j = 0; j < k; ++j) {
    ALFI_CHECK(block_patch_apply(L, slots, slots, L->blk_V + j * ldv, vs, L->blk_Z + j * ldv, zs));   // z_j = M^-1 v_j
    ALFI_CHECK(block_spmv(L, slots, slots, L->blk_Z + j * ldv, zs, L->blk_w, ldv, nullptr, 0, 0));    // w = A z_j
    for (int s = 0; s < nc; ++s) {
      double *hs = hss(s), *hdots = hs + hl.hd, *w = ws(s);
      ProfScope prof(ctx, ALFI_EV_BLAS1);   // to the end of the loop body
      ALFI_CHECK(launch_multi_dot(ctx, Vs(s), ldv, j + 1, w, fused ? nullptr : hdots, n));
      ALFI_CHECK(launch_multi_axpy_norm(ctx, Vs(s), ldv, j + 1, hdots, w, n, ctx->red_partial2, fused ? G : 0));
      if (j + 1 < k)
        ALFI_CHECK(launch_hessenberg_scale(ctx, ctx->red_partial2, G, hdots, hs, j, K, Vs(s) + (int64_t)(j + 1) * ldv, w, n, nullptr));
      else
        ALFI_CHECK(launch_hessenberg_update(ctx, ctx->red_partial2, G, hdots, hs, j, K, nullptr));
    }
  }
  for (int s = 0; s < nc; ++s) {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_fgmres_finish(ctx, hss(s), k, K));
    ALFI_CHECK(launch_update_solution(ctx, X + cols.c[s] * ldx, Zs(s), ldv, k, hss(s) + hl.y, n));
  }
  return 0;
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
