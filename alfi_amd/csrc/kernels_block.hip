// Block right-hand sides: the three bandwidth-bound kernels of a level -- additive apply of dense patch inverses, dof-wise sum,
// flat BSR product -- for up to BLOCK_NV = 4 vectors per stream of the stored values (block_cols.h has the operand layout).
//
// The contract: column c of a block result is the single-vector kernel's result on column c BIT FOR BIT.  Every kernel here is
// its single-vector original (kernels_patch.hip, kernels_vec.hip) with the per-vector state -- accumulators, partial sums,
// carries -- held NV times: per right-hand side the same products and the same sums in the same order, the explicit
// __builtin_fma where the original has one, and plain + where it has that (an expression is written the way the original
// writes it, so that the compiler contracts both or neither).  What is loaded once for the NV vectors: the stored inverse, the
// operator values, every index array.
#include "common.h"
#include "row_piece.h"
#include "block_cols.h"

static_assert(SMALL_PATCH_MAX % RowPiece<float>::V == 0, "the partial sums of the pad rows have slots");
constexpr int BLOCK_APPLY_U = 8;      // 16-byte loads in flight per lane: the single apply's ALFI_APPLY_U (never the order of the sums)

// ---------------------------------------------------------------------------------------------------------------------
// additive apply, stage 1 (patch_apply_kernel): a workgroup of W waves per patch, wave w takes the w-th share of the columns of
// every row piece.  stage[c * stage_len + stage_ptr[p] + r] = sum_j inv_p[r][j] * X[cols.c[c] * ldx + dofs_p[j]].
// LDS: xs[n][NV] interleaved (piece_dot) + part[W][NV][160]: 45 KiB at W = 8, NV = 4 (the single kernel holds 11 KiB).
// Measured, finest levels of configs 3 and 4 at NV = 4: 5.7 / 5.4 TB/s of stored bytes against 6.0 / 6.6 for one vector
// (profiles/block_rhs.txt); nothing here is tuned yet.
// ---------------------------------------------------------------------------------------------------------------------
template <typename S, bool NT, int W, int NV>
__global__ __launch_bounds__(64 * W) void patch_apply_block_kernel(int64_t p0, int64_t p1, const int64_t* __restrict__ patch_ptr,
                                                                   const int32_t* __restrict__ patch_dofs,
                                                                   const int64_t* __restrict__ inv_ptr,
                                                                   const int64_t* __restrict__ stage_ptr, const S* __restrict__ inv,
                                                                   const double* __restrict__ X, int64_t ldx, BlockCols cols,
                                                                   double* __restrict__ stage, int64_t stage_len) {
  constexpr int V = RowPiece<S>::V, MAX_NP = SMALL_PATCH_MAX;
  constexpr PieceStore ST = V == 2 ? PieceStore::PAIR : PieceStore::ALL;
  __shared__ __attribute__((aligned(16))) double xs[MAX_NP * NV];
  __shared__ __attribute__((aligned(16))) double part[W][NV][MAX_NP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = p0 + blockIdx.x;
  if (p >= p1) return;
  const int64_t off = patch_ptr[p];
  const int n = (int)(patch_ptr[p + 1] - off);
  for (int i = threadIdx.x; i < n; i += 64 * W) {
    const int64_t d = patch_dofs[off + i];
#pragma unroll
    for (int c = 0; c < NV; ++c) xs[i * NV + c] = X[(int64_t)cols.c[c] * ldx + d];
  }
  __syncthreads();
  const S* T = inv + inv_ptr[p];
  const int ca = (int)(((int64_t)wave * n) / W), cn = (int)(((int64_t)(wave + 1) * n) / W) - ca;
  double* out = &part[wave][0][0];
  walk_pieces<V>(RowPiece<S>::ld(n), [=](auto R, int row0, int) {
    piece_apply<S, R / V, NT, BLOCK_APPLY_U, true, ST, NV>(T + (int64_t)row0 * n + (int64_t)ca * R, R, cn, xs + ca * NV, lane,
                                                            out + row0, MAX_NP, 0);
  });
  __syncthreads();
  const int lds = (n + 1) & ~1;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    double* dst = stage + (int64_t)c * stage_len + stage_ptr[p];
    for (int i = threadIdx.x; i < lds; i += 64 * W) {
      double d = part[0][c][i];
#pragma unroll
      for (int w = 1; w < W; ++w) d += part[w][c][i];
      dst[i] = d;
    }
  }
}

// stage 2 (patch_sum_kernel): the dof-wise sum in the fixed order of dof_pos, the partition-of-unity weight, the Dirichlet copy
template <int NV>
__global__ __launch_bounds__(256) void patch_sum_block_kernel(int64_t n, const int32_t* __restrict__ dof_ptr,
                                                              const int32_t* __restrict__ dof_pos, const double* __restrict__ stage,
                                                              int64_t stage_len, const uint8_t* __restrict__ bc_mask,
                                                              const double* __restrict__ X, int64_t ldx, double* __restrict__ Y,
                                                              int64_t ldy, BlockCols cols, BlockCols ocols, int pou) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) s[c] = 0.0;
  const int32_t q0 = dof_ptr[i], q1 = dof_ptr[i + 1];
  for (int32_t q = q0; q < q1; ++q) {
    const int32_t pos = dof_pos[q];
#pragma unroll
    for (int c = 0; c < NV; ++c) s[c] += stage[(int64_t)c * stage_len + pos];
  }
  const bool bc = bc_mask[i] != 0;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    if (pou && q1 - q0 > 1) s[c] /= (double)(q1 - q0);
    Y[(int64_t)ocols.c[c] * ldy + i] = bc ? X[(int64_t)cols.c[c] * ldx + i] : s[c];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// flat BSR product (bsr_spmv_flat_kernel): one colflag load and one set of value loads per block serve the NV x gathers; the
// NV partial sums p[c][] and carries go through the same segmented scan.  carry_out: (NV, nchunks, BS).
// Left out on purpose: the single kernel's workgroup -> chunk remap over the XCDs (its xcd_map argument).  It changes which
// workgroup takes which chunk, never a result; the large operators it was measured on de-duplicate their columns and take
// bsr_spmv_dedup_block_kernel (kernels_block_dedup.hip), which keeps it.
// ---------------------------------------------------------------------------------------------------------------------
typedef double blk_d2 __attribute__((ext_vector_type(2)));
template <int BS, bool NT, bool ALIGNED, int NV>
__global__ __launch_bounds__(256) void bsr_spmv_flat_block_kernel(int64_t kbase, int64_t nnzb, int64_t nchunks,
                                                                  const int64_t* __restrict__ chunk_start,
                                                                  const int32_t* __restrict__ colflag,
                                                                  const double* __restrict__ vals,
                                                                  const int32_t* __restrict__ chunk_row,
                                                                  const double* __restrict__ X, int64_t ldx, double* __restrict__ Y,
                                                                  int64_t ldy, const double* __restrict__ B, int64_t ldb,
                                                                  BlockCols cols, BlockCols ocols, double alpha, int mode,
                                                                  double* __restrict__ carry_out, int32_t* __restrict__ carry_row) {
  constexpr int BB = BS * BS;
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;
  const int64_t kend_all = ALIGNED ? chunk_start[chunk + 1] : kbase + nnzb;
  const int64_t base = ALIGNED ? chunk_start[chunk] : kbase + chunk * SPMV_CHUNK;
  int R = chunk_row[chunk];  // block row of lane 0's block
  int Rlast = R;
  double carry[NV][BS];
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int r = 0; r < BS; ++r) carry[c][r] = 0.0;
  auto store_row = [&](int row, const double(&s)[NV][BS]) {
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      double* y = Y + (int64_t)ocols.c[c] * ldy;
      const double* b = B + (int64_t)cols.c[c] * ldb;
#pragma unroll
      for (int r = 0; r < BS; ++r) {
        const int64_t i = (int64_t)row * BS + r;
        y[i] = mode == 0 ? s[c][r] : b[i] - alpha * s[c][r];
      }
    }
  };
#pragma unroll
  for (int u = 0; u < SPMV_U; ++u) {
    if (ALIGNED && base + u * 64 >= kend_all) break;     // wave-uniform: the chunk is shorter than SPMV_CHUNK
    const int64_t k = base + u * 64 + lane;
    const bool valid = k < kend_all;
    const int32_t cf = valid ? (NT ? __builtin_nontemporal_load(colflag + k) : colflag[k]) : 0;
    const bool head = cf < 0;
    const int64_t col = cf & 0x7fffffff;
    double p[NV][BS];
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int r = 0; r < BS; ++r) p[c][r] = 0.0;
    if (valid) {
      const double* v = vals + (k >> 6) * (64 * BB);
      const int kl = (int)(k & 63);        // position inside the 64-block group (== lane unless the view starts mid-group)
      double a[BB];
#pragma unroll
      for (int q = 0; q < BB / 2; ++q) {   // pair planes: one aligned 16-byte load per lane
        const blk_d2* pq = reinterpret_cast<const blk_d2*>(v + q * 128) + kl;
        const blk_d2 t = NT ? __builtin_nontemporal_load(pq) : *pq;
        a[2 * q] = t.x;
        a[2 * q + 1] = t.y;
      }
      if (BB & 1) {
        const double* pl = v + (BB / 2) * 128 + kl;
        a[BB - 1] = NT ? __builtin_nontemporal_load(pl) : *pl;
      }
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        const double* x = X + (int64_t)cols.c[c] * ldx;
        double xv[BS];
#pragma unroll
        for (int cc = 0; cc < BS; ++cc) xv[cc] = x[col * BS + cc];
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
          for (int cc = 0; cc < BS; ++cc) p[c][r] = __builtin_fma(a[r * BS + cc], xv[cc], p[c][r]);
      }
    }
    const unsigned long long hm = __ballot(head);
    if (u > 0) {
      // lane 0 starts a new row: the row carried over from the previous iteration is complete
      if ((hm & 1ull) && lane == 0) store_row(Rlast, carry);
      R = Rlast + (int)(hm & 1ull);
    }
    const int row = R + __popcll(hm & ((2ull << lane) - 2ull));  // row starts at lanes 1 .. lane
    // segmented inclusive scan; f = a row start lies at or before this lane (in this iteration)
    int f = head ? 1 : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      double tp[NV][BS];
#pragma unroll
      for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int r = 0; r < BS; ++r) tp[c][r] = __shfl_up(p[c][r], d);
      const int tf = __shfl_up(f, d);
      if (lane >= d && !f) {
#pragma unroll
        for (int c = 0; c < NV; ++c)
#pragma unroll
          for (int r = 0; r < BS; ++r) p[c][r] += tp[c][r];
        f = tf;
      }
    }
    if (!f) {
#pragma unroll
      for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int r = 0; r < BS; ++r) p[c][r] += carry[c][r];
    }
    // rows ending inside this iteration (the next lane starts a new one); lane 63's row is carried on
    if (lane < 63 && ((hm >> (lane + 1)) & 1ull)) store_row(row, p);
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int r = 0; r < BS; ++r) carry[c][r] = __shfl(p[c][r], 63);
    Rlast = __shfl(row, 63);
  }
  if (ALIGNED) {
    if (lane == 0 && kend_all > base) store_row(Rlast, carry);
    return;
  }
  const int64_t kend = base + SPMV_CHUNK;
  if (lane == 0) {
    const bool closed = kend >= kend_all || colflag[kend] < 0;
    if (closed) {
      store_row(Rlast, carry);
      carry_row[chunk] = -1;
    } else {
#pragma unroll
      for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int r = 0; r < BS; ++r) carry_out[((int64_t)c * nchunks + chunk) * BS + r] = carry[c][r];
      carry_row[chunk] = Rlast;
    }
  }
}

template <int BS, int NV>
__global__ __launch_bounds__(256) void bsr_spmv_fixup_block_kernel(int64_t nchunks, const double* __restrict__ carry,
                                                                   const int32_t* __restrict__ carry_row, double* __restrict__ Y,
                                                                   int64_t ldy, BlockCols ocols, double alpha, int mode) {
  const int64_t c0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c0 >= nchunks) return;
  const int32_t R = carry_row[c0];
  if (R < 0 || (c0 > 0 && carry_row[c0 - 1] == R)) return;  // only the first chunk of a run adds, in chunk order
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    double* y = Y + (int64_t)ocols.c[c] * ldy;
    double s[BS];
#pragma unroll
    for (int r = 0; r < BS; ++r) s[r] = 0.0;
    for (int64_t cc = c0; cc < nchunks && carry_row[cc] == R; ++cc)
#pragma unroll
      for (int r = 0; r < BS; ++r) s[r] += carry[((int64_t)c * nchunks + cc) * BS + r];
#pragma unroll
    for (int r = 0; r < BS; ++r) y[(int64_t)R * BS + r] += mode == 0 ? s[r] : -alpha * s[r];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------------------------------------------------
template <typename S, int W>
static void launch_apply_block_nv(alfi_level* L, const S* inv, const int64_t* inv_ptr, const double* X, int64_t ldx,
                                  const BlockCols& cols, double* stage) {
  alfi_ctx* ctx = L->ctx;
  const dim3 grid((unsigned)L->npatch), block(64 * W);
#define ALFI_BAPPLY(NVV)                                                                                                  \
  hipLaunchKernelGGL((patch_apply_block_kernel<S, true, W, NVV>), grid, block, 0, ctx->stream, (int64_t)0, L->npatch,      \
                     L->patch_ptr, L->patch_dofs, inv_ptr, L->stage_ptr, inv, X, ldx, cols, stage, L->lay.stage_len)
  switch (cols.n) {
    case 1: ALFI_BAPPLY(1); break;
    case 2: ALFI_BAPPLY(2); break;
    case 3: ALFI_BAPPLY(3); break;
    default: ALFI_BAPPLY(4); break;
  }
#undef ALFI_BAPPLY
}
template <typename S>
static int launch_apply_block_w(alfi_level* L, int W, const S* inv, const int64_t* inv_ptr, const double* X, int64_t ldx,
                                const BlockCols& cols, double* stage) {
  if (W == 1) launch_apply_block_nv<S, 1>(L, inv, inv_ptr, X, ldx, cols, stage);
  else if (W == 4) launch_apply_block_nv<S, 4>(L, inv, inv_ptr, X, ldx, cols, stage);
  else if (W == 8) launch_apply_block_nv<S, 8>(L, inv, inv_ptr, X, ldx, cols, stage);
  else return alfi_set_error(L->ctx, ALFI_E_STATE, "block apply with %d waves per patch", W);
  return 0;
}

bool patch_apply_block_waves_ok(int W) { return W == 1 || W == 4 || W == 8; }

// both stages for the 1 .. BLOCK_NV columns of cols on a level whose single apply is patch_apply_kernel with W waves per patch
// (patch_apply_dense_waves, kernels_patch.hip); stage: cols.n x lay.stage_len doubles
int launch_patch_apply_block(alfi_level* L, int W, const BlockCols& cols, const BlockCols& ocols, const double* X, int64_t ldx,
                             double* Y, int64_t ldy, double* stage) {
  alfi_ctx* ctx = L->ctx;
  if (cols.n < 1 || cols.n > BLOCK_NV || ocols.n != cols.n)
    return alfi_set_error(ctx, ALFI_E_ARG, "a block launch takes 1 .. %d columns", BLOCK_NV);
  if (L->npatch > 0) {
    ProfScope prof(ctx, ALFI_EV_PATCH_APPLY);
    if (L->held == HELD_F32) ALFI_CHECK(launch_apply_block_w<float>(L, W, L->inv32, L->inv32_ptr, X, ldx, cols, stage));
    else ALFI_CHECK(launch_apply_block_w<double>(L, W, L->inv, L->inv_ptr, X, ldx, cols, stage));
    ALFI_HIP_CHECK(ctx, hipGetLastError());
  }
  if (!Y) return 0;     // stage 1 alone: the caller sums the staged columns itself (kernels_block_fused.hip)
  return launch_patch_sum_block(L, cols, ocols, X, ldx, Y, ldy, stage);
}

// stage 2 for the columns of cols: what the dense and the condensed (kernels_block_cond.hip) block apply share
int launch_patch_sum_block(alfi_level* L, const BlockCols& cols, const BlockCols& ocols, const double* X, int64_t ldx, double* Y,
                           int64_t ldy, const double* stage) {
  alfi_ctx* ctx = L->ctx;
  if (L->n <= 0) return 0;
  ProfScope prof(ctx, ALFI_EV_PATCH_SCATTER);   // to the end of the function
  const dim3 grid((unsigned)((L->n + 255) / 256)), block(256);
#define ALFI_BSUM(NVV)                                                                                                     \
  hipLaunchKernelGGL((patch_sum_block_kernel<NVV>), grid, block, 0, ctx->stream, L->n, L->dof_ptr, L->dof_pos, stage,       \
                     L->lay.stage_len, L->bc_mask, X, ldx, Y, ldy, cols, ocols, L->pou ? 1 : 0)
  switch (cols.n) {
    case 1: ALFI_BSUM(1); break;
    case 2: ALFI_BSUM(2); break;
    case 3: ALFI_BSUM(3); break;
    default: ALFI_BSUM(4); break;
  }
#undef ALFI_BSUM
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// The widest batch of the product with A under an LDS budget (the ctx's block_lds_bytes): BLOCK_NV where the single product is
// bsr_spmv_flat_kernel (whole-row chunks, or equal chunks + fix-up without de-duplication); where it is bsr_spmv_dedup_kernel,
// as many columns as the staged x entries of the fullest group fit the budget (block_dedup_width, block_cols.h); 0: it loops.
bool bsr_spmv_is_dedup(const DevBSR& A) { return !A.aligned && A.dedup && !A.view && A.kbase == 0; }
int bsr_spmv_block_width(const DevBSR& A, int64_t budget_bytes) {
  if (!A.flat || A.nbrows == 0 || A.nnzb == 0 || (A.bs != 2 && A.bs != 3)) return 0;
  return bsr_spmv_is_dedup(A) ? block_dedup_width(A.max_uniq, A.bs, budget_bytes) : BLOCK_NV;
}
bool bsr_spmv_block_batched(const DevBSR& A, int64_t budget_bytes) { return bsr_spmv_block_width(A, budget_bytes) >= 2; }

template <int BS, int NV>
static int launch_spmv_block_nv(alfi_ctx* ctx, const DevBSR& A, const BlockCols& cols, const BlockCols& ocols, const double* X, int64_t ldx, double* Y,
                                int64_t ldy, const double* B, int64_t ldb, double alpha, int mode, double* carry) {
  if (A.aligned) {
    const int64_t nchunks = A.nchunks;
    hipLaunchKernelGGL((bsr_spmv_flat_block_kernel<BS, true, true, NV>), dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0,
                       ctx->stream, A.kbase, A.nnzb, nchunks, A.chunk_start, A.colidx, A.vals, A.chunk_row, X, ldx, Y, ldy, B, ldb,
                       cols, ocols, alpha, mode, carry, A.carry_row);
    ALFI_HIP_CHECK(ctx, hipGetLastError());
    return 0;
  }
  const int64_t nchunks = (A.nnzb + SPMV_CHUNK - 1) / SPMV_CHUNK;
  if (bsr_spmv_is_dedup(A)) {     // the staged gathers: kernels_block_dedup.hip
    ALFI_CHECK(launch_bsr_spmv_dedup_block(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry));
  } else {
    hipLaunchKernelGGL((bsr_spmv_flat_block_kernel<BS, true, false, NV>), dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0,
                       ctx->stream, A.kbase, A.nnzb, nchunks, (const int64_t*)nullptr, A.colidx, A.vals, A.chunk_row, X, ldx, Y, ldy,
                       B, ldb, cols, ocols, alpha, mode, carry, A.carry_row);
    ALFI_HIP_CHECK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL((bsr_spmv_fixup_block_kernel<BS, NV>), dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, ctx->stream,
                     nchunks, carry, A.carry_row, Y, ldy, ocols, alpha, mode);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
template <int BS>
static int launch_spmv_block_bs(alfi_ctx* ctx, const DevBSR& A, const BlockCols& cols, const BlockCols& ocols, const double* X, int64_t ldx, double* Y,
                                int64_t ldy, const double* B, int64_t ldb, double alpha, int mode, double* carry) {
  switch (cols.n) {
    case 1: return launch_spmv_block_nv<BS, 1>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
    case 2: return launch_spmv_block_nv<BS, 2>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
    case 3: return launch_spmv_block_nv<BS, 3>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
    default: return launch_spmv_block_nv<BS, 4>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
  }
}

// Y[:, c] = A X[:, c] (mode 0) or B[:, c] - alpha A X[:, c] (mode 1) for the columns of cols: 1 .. BLOCK_NV of them on a flat
// operator, 2 .. bsr_spmv_block_width(A, the ctx's block_lds_bytes) on a de-duplicated one; carry: cols.n x ceil(nnzb /
// SPMV_CHUNK) x bs doubles (read by the fix-up of unaligned chunks alone)
int launch_bsr_spmv_block(alfi_ctx* ctx, const DevBSR& A, const BlockCols& cols, const BlockCols& ocols, const double* X,
                          int64_t ldx, double* Y, int64_t ldy, const double* B, int64_t ldb, double alpha, int mode, double* carry) {
  if (cols.n < 1 || cols.n > BLOCK_NV || ocols.n != cols.n)
    return alfi_set_error(ctx, ALFI_E_ARG, "a block launch takes 1 .. %d columns", BLOCK_NV);
  const int width = bsr_spmv_block_width(A, ctx->block_lds_bytes);
  if (width < 2) return alfi_set_error(ctx, ALFI_E_STATE, "block product on an operator whose product does not batch");
  if (cols.n > width)
    return alfi_set_error(ctx, ALFI_E_STATE, "block product: %d columns of %d distinct x entries do not fit the LDS budget", cols.n,
                          A.max_uniq);
  if (mode == 0) B = X, ldb = ldx;      // never read; a valid address for the kernel's pointer arithmetic
  if (A.bs == 2) return launch_spmv_block_bs<2>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
  return launch_spmv_block_bs<3>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
}
