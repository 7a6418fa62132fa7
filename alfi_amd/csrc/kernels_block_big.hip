// Block right-hand sides on dense macro-star inverses (patches above SMALL_PATCH_MAX dofs, FP64 or the single-precision copy):
// big_apply_kernel of kernels_bigpatch.hip for NV = 2 .. 4 vectors per stream of the stored inverse.
//
// The contract is that of kernels_block.hip: column c of the result is the single-vector apply on column c BIT FOR BIT.  The
// kernel is its one-vector original with the per-vector state held NV times: 256 threads, ``split`` consecutive workgroups per
// patch (big_split, patch_plan.h -- the function the single launcher reads), the same pieces to the same waves, the same walk,
// BIG_U loads in flight, nontemporal loads of the inverse, the same store policy.  A row's sum is the ascending columns of its
// column group, then the groups by shuffles in a fixed order (piece_dot, row_piece.h): it depends on the patch alone, not on
// ``split``, the launch or NV.
//
// LDS: x_p of the NV columns interleaved entry by entry (xs[i * NV + c], what the NV piece_dot reads), DYNAMIC and sized by the
// level's largest patch -- block_big_lds(max_np, NV) bytes (block_cols.h), which is what the width rule budgets --, not by
// PATCH_MAX: four columns of a 2048-dof level take 64 KiB, of a 4096-dof level 128 KiB.
#include "common.h"
#include "row_piece.h"
#include "block_cols.h"
#include "cond_apply.h"

// stage[c * stage_len + stage_ptr[p] + r] = sum_j inv_p[r][j] * X[cols.c[c] * ldx + dofs_p[j]]
// S = float: a patch has (n + 1) & ~1 staging slots per column, and the sums of its pad rows are not stored (GUARDED, as in the
// single kernel).
template <typename S, bool NT, int NV>
__global__ __launch_bounds__(256) void big_apply_block_kernel(int64_t p0, int64_t npatch, const int64_t* __restrict__ patch_ptr,
                                                               const int32_t* __restrict__ patch_dofs,
                                                               const int64_t* __restrict__ inv_ptr,
                                                               const int64_t* __restrict__ stage_ptr, const S* __restrict__ inv,
                                                               const double* __restrict__ X, int64_t ldx, BlockCols cols,
                                                               double* __restrict__ stage, int stage_len, int split) {
  constexpr int V = RowPiece<S>::V;
  constexpr PieceStore ST = V == 2 ? PieceStore::PAIR : PieceStore::GUARDED;
  extern __shared__ __attribute__((aligned(16))) double big_blk_xs[];
  double* xs = big_blk_xs;          // n x NV
  const int64_t p = p0 + blockIdx.x / split;
  const int part = blockIdx.x % split, nwave = 4 * split;
  if (p >= npatch) return;
  const int64_t off = patch_ptr[p];
  const int n = (int)(patch_ptr[p + 1] - off);
  for (int i = threadIdx.x; i < n; i += 256) {
    const int64_t d = patch_dofs[off + i];
#pragma unroll
    for (int c = 0; c < NV; ++c) xs[i * NV + c] = X[(int64_t)cols.c[c] * ldx + d];
  }
  __syncthreads();
  const int wave = part * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const S* T = inv + inv_ptr[p];
  double* out = stage + stage_ptr[p];
  walk_pieces<V>(RowPiece<S>::ld(n), [=](auto R, int row0, int piece) {
    if (piece % nwave == wave)
      piece_apply<S, R / V, NT, BIG_U, false, ST, NV>(T + (int64_t)row0 * n, R, n, xs, lane, out + row0, stage_len, n - row0);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------------------------------------------------
template <typename S, int NV>
static int launch_big_block_nv(alfi_level* L, const S* inv, const int64_t* inv_ptr, const BlockCols& cols, const double* X,
                               int64_t ldx, double* stage) {
  alfi_ctx* ctx = L->ctx;
  const int split = big_split(L->npatch, L->lay.max_np);
  const size_t lds = (size_t)block_big_lds(L->lay.max_np, NV);
  const dim3 grid((unsigned)(L->npatch * split)), block(256);
  // (a budget above the default, alfi_ctx_set_block_lds_bytes, is what brings a launch here above 64 KiB)
  if (lds > 64 * 1024)
    ALFI_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&big_apply_block_kernel<S, true, NV>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((big_apply_block_kernel<S, true, NV>), grid, block, lds, ctx->stream, (int64_t)0, L->npatch, L->patch_ptr,
                     L->patch_dofs, inv_ptr, L->stage_ptr, inv, X, ldx, cols, stage, (int)L->lay.stage_len, split);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
template <typename S>
static int launch_big_block_s(alfi_level* L, const S* inv, const int64_t* inv_ptr, const BlockCols& cols, const double* X, int64_t ldx,
                              double* stage) {
  switch (cols.n) {
    case 2: return launch_big_block_nv<S, 2>(L, inv, inv_ptr, cols, X, ldx, stage);
    case 3: return launch_big_block_nv<S, 3>(L, inv, inv_ptr, cols, X, ldx, stage);
    default: return launch_big_block_nv<S, 4>(L, inv, inv_ptr, cols, X, ldx, stage);
  }
}

// Both stages of the additive apply for the 2 .. BLOCK_NV columns of cols on a serial level that holds dense inverses (FP64 or
// FP32) with a patch above SMALL_PATCH_MAX dofs: the whole level in one launch.  stage: cols.n x lay.stage_len doubles.  The
// caller has checked that block_big_lds(max_np, cols.n) is within the ctx's budget (block_big_width), which
// alfi_ctx_set_block_lds_bytes keeps within the device's limit, and that cols.n x stage_len fits an int.
int launch_big_apply_block(alfi_level* L, const BlockCols& cols, const BlockCols& ocols, const double* X, int64_t ldx, double* Y,
                           int64_t ldy, double* stage) {
  alfi_ctx* ctx = L->ctx;
  if (cols.n < 2 || cols.n > BLOCK_NV || ocols.n != cols.n)
    return alfi_set_error(ctx, ALFI_E_ARG, "a macro-star block launch takes 2 .. %d columns", BLOCK_NV);
  if ((L->held != HELD_F64 && L->held != HELD_F32) || L->lay.max_np <= SMALL_PATCH_MAX || L->lay.stage_len > INT32_MAX / BLOCK_NV)
    return alfi_set_error(ctx, ALFI_E_STATE, "macro-star block apply on a level without dense macro-star inverses");
  if (block_big_lds(L->lay.max_np, cols.n) > ctx->block_lds_bytes)
    return alfi_set_error(ctx, ALFI_E_STATE, "macro-star block apply: %d columns of %d dofs do not fit the LDS budget", cols.n,
                          L->lay.max_np);
  if (L->npatch > 0) {
    ProfScope prof(ctx, ALFI_EV_PATCH_APPLY);
    if (L->held == HELD_F32) ALFI_CHECK(launch_big_block_s<float>(L, L->inv32, L->inv32_ptr, cols, X, ldx, stage));
    else ALFI_CHECK(launch_big_block_s<double>(L, L->inv, L->inv_ptr, cols, X, ldx, stage));
  }
  if (!Y) return 0;     // stage 1 alone: the caller sums the staged columns itself (kernels_block_fused.hip)
  return launch_patch_sum_block(L, cols, ocols, X, ldx, Y, ldy, stage);
}
