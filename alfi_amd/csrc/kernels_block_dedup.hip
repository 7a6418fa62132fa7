// Block right-hand sides in the de-duplicated level product: bsr_spmv_dedup_kernel of kernels_vec.hip for NV = 2 .. 4 vectors per
// stream of the operator.
//
// The contract is that of kernels_block.hip: column c of the result is the single-vector product on column c BIT FOR BIT.  The
// kernel is its one-vector original with the per-vector state -- staged x entries, partial sums, carries -- held NV times; the
// rows that run on into the next chunk are completed by bsr_spmv_fixup_block_kernel (kernels_block.hip), the fix-up of the flat
// block product.
#include "common.h"
#include "block_cols.h"

typedef double dedup_d2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------------------
// de-duplicated product (bsr_spmv_dedup_kernel, kernels_vec.hip): a workgroup stages the distinct x entries of its group of
// SPMV_WG blocks for the NV columns -- one gather per distinct column and right-hand side -- and streams lidx and the value
// planes once.  Everything per right-hand side is the single kernel's: the FMA order over a block's columns, the segmented scan,
// += carry, the fix-up's chunk-order sum (bsr_spmv_fixup_block_kernel, kernels_block.hip).  The workgroup -> group map over the XCDs is the single
// kernel's too (it moves work, never a result).  carry_out: (NV, nchunks, BS).
// LDS: DYNAMIC, block_dedup_lds(max_uniq, BS, NV) bytes with max_uniq the operator's largest number of distinct columns in a
// group (DevBSR::max_uniq), not SPMV_DEDUP_MAX -- 250 distinct columns take 24 KiB at bs 3 and NV 4, not 96.  The NV copies
// are interleaved entry by entry, xs[(i * NV + c) * BS + q]: a lane forms ONE LDS address from its local index and reads the
// NV * BS doubles of its column at constant offsets (8- or 16-byte reads, 256 B/clk either way); planes per right-hand side would
// need a run-time plane stride in every address and buy nothing, since the lanes' entries are scattered over the banks in both.
// Every wave reaches the staging barrier, also the waves of the last workgroup whose chunk lies past nchunks.
// ---------------------------------------------------------------------------------------------------------------------
template <int BS, int NV>
__global__ __launch_bounds__(256) void bsr_spmv_dedup_block_kernel(int64_t nnzb, int64_t nchunks, const uint16_t* __restrict__ lidx,
                                                                   const int32_t* __restrict__ ucol,
                                                                   const int32_t* __restrict__ uptr,
                                                                   const int32_t* __restrict__ colflag,
                                                                   const double* __restrict__ vals,
                                                                   const int32_t* __restrict__ chunk_row,
                                                                   const double* __restrict__ X, int64_t ldx, double* __restrict__ Y,
                                                                   int64_t ldy, const double* __restrict__ B, int64_t ldb,
                                                                   BlockCols cols, BlockCols ocols, double alpha, int mode,
                                                                   double* __restrict__ carry_out, int32_t* __restrict__ carry_row,
                                                                   int xcd_map, int max_uniq) {
  constexpr int BB = BS * BS, E = NV * BS;      // E: doubles per staged entry
  extern __shared__ __attribute__((aligned(16))) double dedup_blk_xs[];
  double* xs = dedup_blk_xs;                    // max_uniq x NV x BS
  const int lane = threadIdx.x & 63;
  int64_t g = blockIdx.x;
  if (xcd_map == 1) {
    const int64_t nb = gridDim.x, per = nb >> 3, rem = nb & 7, xcd = g & 7, idx = g >> 3;
    g = xcd * per + (xcd < rem ? xcd : rem) + idx;
  } else if (xcd_map > 1) {     // strips, as in bsr_spmv_dedup_kernel
    const int64_t S = xcd_map, nb = gridDim.x, full = nb / (8 * S) * (8 * S);
    if (g < full) {
      const int64_t xcd = g & 7, i = g >> 3, strip = i / S, within = i - strip * S;
      g = (strip * 8 + xcd) * S + within;
    }
  }
  const int64_t chunk = g * 4 + (threadIdx.x >> 6);
  const bool active = chunk < nchunks;
  const int64_t base = chunk * SPMV_CHUNK;
  const int32_t u0 = uptr[g];
  const int nu = min(uptr[g + 1] - u0, max_uniq);      // (max_uniq is the largest such difference: the LDS is sized by it)
  for (int i = threadIdx.x; i < nu; i += 256) {
    const int64_t col = __builtin_nontemporal_load(ucol + u0 + i);
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const double* x = X + (int64_t)cols.c[c] * ldx;
#pragma unroll
      for (int q = 0; q < BS; ++q) xs[i * E + c * BS + q] = x[col * BS + q];
    }
  }
  __syncthreads();
  if (!active) return;
  int R = chunk_row[chunk];
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
    const int64_t k = base + u * 64 + lane;
    const bool valid = k < nnzb;
    const uint16_t li = valid ? __builtin_nontemporal_load(lidx + k) : (uint16_t)0;
    const bool head = (li & 0x8000u) != 0;
    const int lc = li & 0x7fff;
    double p[NV][BS];
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int r = 0; r < BS; ++r) p[c][r] = 0.0;
    if (valid) {
      const double* v = vals + (k >> 6) * (64 * BB);
      double a[BB];
#pragma unroll
      for (int q = 0; q < BB / 2; ++q) {
        const dedup_d2 t = __builtin_nontemporal_load(reinterpret_cast<const dedup_d2*>(v + q * 128) + lane);
        a[2 * q] = t.x;
        a[2 * q + 1] = t.y;
      }
      if (BB & 1) a[BB - 1] = __builtin_nontemporal_load(v + (BB / 2) * 128 + lane);
      const double* xe = xs + lc * E;
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        double xv[BS];
#pragma unroll
        for (int cc = 0; cc < BS; ++cc) xv[cc] = xe[c * BS + cc];
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
          for (int cc = 0; cc < BS; ++cc) p[c][r] = __builtin_fma(a[r * BS + cc], xv[cc], p[c][r]);
      }
    }
    const unsigned long long hm = __ballot(head);
    if (u > 0) {
      if ((hm & 1ull) && lane == 0) store_row(Rlast, carry);
      R = Rlast + (int)(hm & 1ull);
    }
    const int row = R + __popcll(hm & ((2ull << lane) - 2ull));
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
    if (lane < 63 && ((hm >> (lane + 1)) & 1ull)) store_row(row, p);
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int r = 0; r < BS; ++r) carry[c][r] = __shfl(p[c][r], 63);
    Rlast = __shfl(row, 63);
  }
  const int64_t kend = base + SPMV_CHUNK;
  if (lane == 0) {
    const bool closed = kend >= nnzb || colflag[kend] < 0;
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

// ---------------------------------------------------------------------------------------------------------------------
// launch wrapper
// ---------------------------------------------------------------------------------------------------------------------
template <int BS, int NV>
static int launch_dedup_block_nv(alfi_ctx* ctx, const DevBSR& A, const BlockCols& cols, const BlockCols& ocols, const double* X,
                                 int64_t ldx, double* Y, int64_t ldy, const double* B, int64_t ldb, double alpha, int mode,
                                 double* carry) {
  constexpr int xcd = 64;       // strips of 64 groups per XCD: the single launch's map (launch_bsr_spmv_bs, kernels_vec.hip)
  const int64_t nchunks = (A.nnzb + SPMV_CHUNK - 1) / SPMV_CHUNK;
  const size_t lds = (size_t)block_dedup_lds(A.max_uniq, BS, NV);
  // (a budget above the default, alfi_ctx_set_block_lds_bytes, is what brings a launch here above 64 KiB)
  if (lds > 64 * 1024)
    ALFI_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&bsr_spmv_dedup_block_kernel<BS, NV>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((bsr_spmv_dedup_block_kernel<BS, NV>), dim3((unsigned)((nchunks + 3) / 4)), dim3(256), lds, ctx->stream,
                     A.nnzb, nchunks, A.lidx, A.ucol, A.uptr, A.colidx, A.vals, A.chunk_row, X, ldx, Y, ldy, B, ldb, cols, ocols,
                     alpha, mode, carry, A.carry_row, xcd, A.max_uniq);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
template <int BS>
static int launch_dedup_block_bs(alfi_ctx* ctx, const DevBSR& A, const BlockCols& cols, const BlockCols& ocols, const double* X,
                                 int64_t ldx, double* Y, int64_t ldy, const double* B, int64_t ldb, double alpha, int mode,
                                 double* carry) {
  switch (cols.n) {
    case 2: return launch_dedup_block_nv<BS, 2>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
    case 3: return launch_dedup_block_nv<BS, 3>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
    default: return launch_dedup_block_nv<BS, 4>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
  }
}

// The main launch of the block product for the 2 .. BLOCK_NV columns of cols on an operator whose single product de-duplicates
// its gathers (bsr_spmv_is_dedup); launch_bsr_spmv_block (kernels_block.hip), the one caller, runs the fix-up after it and has
// checked that block_dedup_lds(max_uniq, bs, cols.n) is within the ctx's budget, which alfi_ctx_set_block_lds_bytes keeps within
// the device's limit.  carry: cols.n x ceil(nnzb / SPMV_CHUNK) x bs doubles.
int launch_bsr_spmv_dedup_block(alfi_ctx* ctx, const DevBSR& A, const BlockCols& cols, const BlockCols& ocols, const double* X,
                                int64_t ldx, double* Y, int64_t ldy, const double* B, int64_t ldb, double alpha, int mode,
                                double* carry) {
  if (cols.n < 2 || cols.n > BLOCK_NV || ocols.n != cols.n)
    return alfi_set_error(ctx, ALFI_E_ARG, "the de-duplicated block product takes 2 .. %d columns", BLOCK_NV);
  if (!bsr_spmv_is_dedup(A) || (A.bs != 2 && A.bs != 3) || A.max_uniq < 1 || A.max_uniq > SPMV_DEDUP_MAX)
    return alfi_set_error(ctx, ALFI_E_STATE, "de-duplicated block product on an operator without de-duplication tables");
  if (block_dedup_lds(A.max_uniq, A.bs, cols.n) > ctx->block_lds_bytes)
    return alfi_set_error(ctx, ALFI_E_STATE, "block product: %d columns of %d distinct x entries do not fit the LDS budget", cols.n,
                          A.max_uniq);
  if (A.bs == 2) return launch_dedup_block_bs<2>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
  return launch_dedup_block_bs<3>(ctx, A, cols, ocols, X, ldx, Y, ldy, B, ldb, alpha, mode, carry);
}
