// Block transpose of a level operator IN PLACE (alfi_level_transpose): the adjoint of a Newton step solves with
//
//     J^T = [[A^T, B^T], [B, 0]]        for   J = [[A, B^T], [B, 0]],
//
// so only the velocity block of every level changes.  Same sparsity: block k at (i, j) receives A[j, i]^T from its mirror
// block m(k) at (j, i).  The pass is a permutation of the values, so the result is bitwise transpose(A).
//   (1) transpose_mirror_kernel (once per level, cached): a lane per block finds its row by bisecting rowptr and its mirror by
//       bisecting row j's sorted columns for i; a missing mirror (structurally non-symmetric pattern) or unsorted columns
//       raise a device flag, which the host reads BEFORE any value is touched.
//   (2) transpose_swap_kernel: a lane per block k with m(k) >= k owns the pair {k, m(k)}: it loads both bs x bs blocks and
//       stores them swapped and transposed (m == k: the diagonal block transposed in place).  One wave handles 64 consecutive
//       blocks, which in the lane-major layout is one group: its own side of each swap is coalesced (16 B per lane per entry
//       pair), the mirror side is a gather.  Algorithmic bytes 2 * 8 * bs^2 * nnzb (+ 4 * nnzb of the mirror map).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void transpose_mirror_kernel(int64_t nbrows, int64_t nnzb, const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ colidx, int32_t* __restrict__ mirror,
                                                               int* __restrict__ bad) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nnzb) return;
  // row of block k: rowptr[lo] <= k < rowptr[hi] (empty rows of the host layout are skipped by the bisection)
  int64_t lo = 0, hi = nbrows;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= k) lo = mid;
    else hi = mid;
  }
  const int32_t i = (int32_t)lo;
  const int32_t j = colidx[k] & 0x7fffffff;          // (lane-major layout: the sign bit marks a row's first block)
  // columns strictly ascending within the row: the bisection below relies on it
  if (k > rowptr[lo] && (colidx[k - 1] & 0x7fffffff) >= j) atomicOr(bad, 2);
  int32_t m = -1;
  if (j >= 0 && j < nbrows) {
    int32_t a = rowptr[j], b = rowptr[j + 1];
    while (a < b) {
      const int32_t mid = (a + b) >> 1;
      if ((colidx[mid] & 0x7fffffff) < i) a = mid + 1;
      else b = mid;
    }
    if (a < rowptr[j + 1] && (colidx[a] & 0x7fffffff) == i) m = a;
  }
  mirror[k] = m;
  if (m < 0) atomicOr(bad, 1);
}

// one block's bs x bs entries (row-major e = r * bs + c) in and out of the level's value layout
template <int BS, int FLAT>
__device__ __forceinline__ void load_block(const double* __restrict__ vals, int64_t k, double (&v)[BS * BS]) {
  constexpr int BB = BS * BS;
  if (FLAT) {
    const double* g = vals + (k >> 6) * 64 * BB + (k & 63) * 2;
#pragma unroll
    for (int p = 0; p < BB / 2; ++p) {
      const double2 t = *reinterpret_cast<const double2*>(g + p * 128);
      v[2 * p] = t.x;
      v[2 * p + 1] = t.y;
    }
    if (BB & 1) v[BB - 1] = vals[bsr_val_index(1, k, BB - 1, BB)];
  } else {
#pragma unroll
    for (int e = 0; e < BB; ++e) v[e] = vals[k * BB + e];
  }
}
template <int BS, int FLAT>
__device__ __forceinline__ void store_block_transposed(double* __restrict__ vals, int64_t k, const double (&v)[BS * BS]) {
  constexpr int BB = BS * BS;
  double t[BB];
#pragma unroll
  for (int r = 0; r < BS; ++r)
#pragma unroll
    for (int c = 0; c < BS; ++c) t[r * BS + c] = v[c * BS + r];
  if (FLAT) {
    double* g = vals + (k >> 6) * 64 * BB + (k & 63) * 2;
#pragma unroll
    for (int p = 0; p < BB / 2; ++p) *reinterpret_cast<double2*>(g + p * 128) = make_double2(t[2 * p], t[2 * p + 1]);
    if (BB & 1) vals[bsr_val_index(1, k, BB - 1, BB)] = t[BB - 1];
  } else {
#pragma unroll
    for (int e = 0; e < BB; ++e) vals[k * BB + e] = t[e];
  }
}

template <int BS, int FLAT>
__global__ __launch_bounds__(256) void transpose_swap_kernel(int64_t nnzb, const int32_t* __restrict__ mirror,
                                                             double* __restrict__ vals) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nnzb) return;
  const int64_t m = mirror[k];
  if (m < k) return;                       // the pair belongs to lane m
  double a[BS * BS];
  load_block<BS, FLAT>(vals, k, a);
  if (m == k) {
    store_block_transposed<BS, FLAT>(vals, k, a);
    return;
  }
  double b[BS * BS];
  load_block<BS, FLAT>(vals, m, b);
  store_block_transposed<BS, FLAT>(vals, k, b);
  store_block_transposed<BS, FLAT>(vals, m, a);
}

}  // namespace

int launch_transpose_mirror(alfi_ctx* ctx, const DevBSR& A, int32_t* mirror, int* bad) {
  if (A.nnzb == 0) return 0;
  const unsigned grid = (unsigned)((A.nnzb + 255) / 256);
  hipLaunchKernelGGL(transpose_mirror_kernel, dim3(grid), dim3(256), 0, ctx->stream, A.nbrows, A.nnzb, A.rowptr, A.colidx,
                     mirror, bad);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

int launch_transpose_swap(alfi_ctx* ctx, const DevBSR& A, const int32_t* mirror) {
  if (A.nnzb == 0) return 0;
  const unsigned grid = (unsigned)((A.nnzb + 255) / 256);
#define ALFI_TSWAP(BS, FL) hipLaunchKernelGGL((transpose_swap_kernel<BS, FL>), dim3(grid), dim3(256), 0, ctx->stream, A.nnzb, mirror, A.vals)
  if (A.bs == 2) {
    if (A.flat) ALFI_TSWAP(2, 1);
    else ALFI_TSWAP(2, 0);
  } else if (A.bs == 3) {
    if (A.flat) ALFI_TSWAP(3, 1);
    else ALFI_TSWAP(3, 0);
  } else {
    return alfi_set_error(ctx, ALFI_E_ARG, "transpose: block size %d", A.bs);
  }
#undef ALFI_TSWAP
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
