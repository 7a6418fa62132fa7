// Vector kernels of the Chebyshev level smoother (alfi_smooth_chebyshev), the point-Jacobi level preconditioner
// (alfi_level_set_jacobi) and the device CG of alfi_mg_cg.  All of them are memory-bound FP64 streams: wave64, 256 lanes per
// workgroup, 16 bytes per lane and access where the vectors start on a 16-byte boundary, a scalar tail for an odd length.
#include "common.h"

typedef double vec_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ vec_d2 ld2(const double* p, int64_t i2) { return reinterpret_cast<const vec_d2*>(p)[i2]; }
__device__ __forceinline__ void st2(double* p, int64_t i2, vec_d2 v) { reinterpret_cast<vec_d2*>(p)[i2] = v; }

static inline bool aligned16(const void* a, const void* b, const void* c, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}
static inline dim3 stream_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

// ---- fused Chebyshev update: d <- a d + c z, x <- x + d --------------------------------------------------------------------
// 3 reads + 2 writes per entry (40 bytes).  MODE 1: the first step, d <- c z without reading d (it may hold anything, NaNs
// included: 2 reads + 2 writes); MODE 2: the first step from a zero iterate, x <- d without reading x either (1 read + 2 writes).
template <int MODE>
__device__ __forceinline__ void cheb_entry(double& d, double& x, double z, double a, double c) {
  d = MODE == 0 ? __builtin_fma(a, d, c * z) : c * z;
  x = MODE == 2 ? d : x + d;
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void cheb_update_kernel(double* __restrict__ d, double* __restrict__ x,
                                                           const double* __restrict__ z, double a, double c, int64_t n) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t i = t0; i < n2; i += step) {
      vec_d2 di = {0.0, 0.0}, xi = {0.0, 0.0};
      if (MODE == 0) di = ld2(d, i);
      if (MODE != 2) xi = ld2(x, i);
      const vec_d2 zi = ld2(z, i);
      double d0 = di.x, d1 = di.y, x0 = xi.x, x1 = xi.y;
      cheb_entry<MODE>(d0, x0, zi.x, a, c);
      cheb_entry<MODE>(d1, x1, zi.y, a, c);
      st2(d, i, vec_d2{d0, d1});
      st2(x, i, vec_d2{x0, x1});
    }
    if ((n & 1) && t0 == 0) {       // the odd last entry
      double di = MODE == 0 ? d[n - 1] : 0.0, xi = MODE != 2 ? x[n - 1] : 0.0;
      cheb_entry<MODE>(di, xi, z[n - 1], a, c);
      d[n - 1] = di;
      x[n - 1] = xi;
    }
  } else {
    for (int64_t i = t0; i < n; i += step) {
      double di = MODE == 0 ? d[i] : 0.0, xi = MODE != 2 ? x[i] : 0.0;
      cheb_entry<MODE>(di, xi, z[i], a, c);
      d[i] = di;
      x[i] = xi;
    }
  }
}

int launch_cheb_update(alfi_ctx* ctx, double* d, double* x, const double* z, double a, double c, int64_t n, int mode) {
  if (n <= 0) return 0;
  if (mode < 0 || mode > 2) return alfi_set_error(ctx, ALFI_E_ARG, "launch_cheb_update: mode %d", mode);
  const bool vec = aligned16(d, x, z);
  const dim3 grid = stream_grid(vec ? (n + 1) >> 1 : n);
#define ALFI_CHEB_CASE(M)                                                                                           \
  case M:                                                                                                           \
    if (vec) hipLaunchKernelGGL((cheb_update_kernel<M, true>), grid, dim3(256), 0, ctx->stream, d, x, z, a, c, n);  \
    else hipLaunchKernelGGL((cheb_update_kernel<M, false>), grid, dim3(256), 0, ctx->stream, d, x, z, a, c, n);     \
    break;
  switch (mode) {
    ALFI_CHEB_CASE(0)
    ALFI_CHEB_CASE(1)
    ALFI_CHEB_CASE(2)
  }
#undef ALFI_CHEB_CASE
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// ---- point Jacobi ------------------------------------------------------------------------------------------------------------
// diag[i * bs + c] = entry (c, c) of the diagonal block of block row i, in either value layout (bsr_val_index); a block row
// without a diagonal block gets 0, which the apply treats as 1 (PCJacobi does the same with a zero diagonal entry).
__global__ __launch_bounds__(256) void jacobi_diag_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                           const double* __restrict__ vals, int flat, int bs, int64_t nbrows,
                                                           double* __restrict__ diag) {
  const int bb = bs * bs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nbrows; i += (int64_t)gridDim.x * 256) {
    int64_t kd = -1;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      if ((int64_t)(colidx[k] & 0x7fffffff) == i) kd = k;      // (flat layout: the sign bit marks the first block of a row)
    for (int c = 0; c < bs; ++c) diag[i * bs + c] = kd >= 0 ? vals[bsr_val_index(flat, kd, c * bs + c, bb)] : 0.0;
  }
}

int launch_jacobi_diag(alfi_ctx* ctx, const DevBSR& A, double* diag) {
  if (A.nbrows <= 0) return 0;
  hipLaunchKernelGGL(jacobi_diag_kernel, stream_grid(A.nbrows), dim3(256), 0, ctx->stream, A.rowptr, A.colidx, A.vals, A.flat,
                     A.bs, A.nbrows, diag);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// y_i = x_i / A_ii, y_i = x_i on Dirichlet dofs: 2 reads + 1 write of 8 bytes and 1 mask byte per entry (25 bytes)
__device__ __forceinline__ double jacobi_entry(double x, double dg, uint8_t bc) { return (bc || dg == 0.0) ? x : x / dg; }

template <bool VEC>
__global__ __launch_bounds__(256) void jacobi_apply_kernel(double* __restrict__ y, const double* __restrict__ x,
                                                            const double* __restrict__ diag, const uint8_t* __restrict__ bc,
                                                            int64_t n) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t i = t0; i < n2; i += step) {
      const vec_d2 xi = ld2(x, i), di = ld2(diag, i);
      const uint16_t m = reinterpret_cast<const uint16_t*>(bc)[i];     // (the mask comes from hipMalloc: 2-byte aligned)
      vec_d2 yi;
      yi.x = jacobi_entry(xi.x, di.x, (uint8_t)(m & 0xff));
      yi.y = jacobi_entry(xi.y, di.y, (uint8_t)(m >> 8));
      st2(y, i, yi);
    }
    if ((n & 1) && t0 == 0) y[n - 1] = jacobi_entry(x[n - 1], diag[n - 1], bc[n - 1]);
  } else {
    for (int64_t i = t0; i < n; i += step) y[i] = jacobi_entry(x[i], diag[i], bc[i]);
  }
}

int launch_jacobi_apply(alfi_ctx* ctx, double* y, const double* x, const double* diag, const uint8_t* bc, int64_t n) {
  if (n <= 0) return 0;
  const bool vec = aligned16(y, x, diag) && (reinterpret_cast<uintptr_t>(bc) & 1) == 0;
  const dim3 grid = stream_grid(vec ? (n + 1) >> 1 : n);
  if (vec) hipLaunchKernelGGL((jacobi_apply_kernel<true>), grid, dim3(256), 0, ctx->stream, y, x, diag, bc, n);
  else hipLaunchKernelGGL((jacobi_apply_kernel<false>), grid, dim3(256), 0, ctx->stream, y, x, diag, bc, n);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// ---- CG (alfi_mg_cg): the step lengths stay on the device ------------------------------------------------------------------------
// s[0], s[1]: r . z of the current and the next iteration (alternating), s[2]: p . A p, s[3]: |r|^2
// x += alpha p, r -= alpha w with alpha = s[cur] / s[2]
__global__ __launch_bounds__(256) void cg_update_xr_kernel(double* __restrict__ x, double* __restrict__ r,
                                                            const double* __restrict__ p, const double* __restrict__ w,
                                                            const double* __restrict__ s, int cur, int64_t n) {
  const double alpha = s[cur] / s[2];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    x[i] = __builtin_fma(alpha, p[i], x[i]);
    r[i] = __builtin_fma(-alpha, w[i], r[i]);
  }
}
// p = z + beta p with beta = s[cur] / s[cur ^ 1] (this iteration's r . z over the last one's); first: p = z
__global__ __launch_bounds__(256) void cg_update_p_kernel(double* __restrict__ p, const double* __restrict__ z,
                                                           const double* __restrict__ s, int cur, int first, int64_t n) {
  const double beta = first ? 0.0 : s[cur] / s[cur ^ 1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    p[i] = first ? z[i] : __builtin_fma(beta, p[i], z[i]);
}
int launch_cg_update_xr(alfi_ctx* ctx, double* x, double* r, const double* p, const double* w, const double* s, int cur,
                        int64_t n) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cg_update_xr_kernel, stream_grid(n), dim3(256), 0, ctx->stream, x, r, p, w, s, cur, n);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
int launch_cg_update_p(alfi_ctx* ctx, double* p, const double* z, const double* s, int cur, int first, int64_t n) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cg_update_p_kernel, stream_grid(n), dim3(256), 0, ctx->stream, p, z, s, cur, first, n);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}

// *s <- sqrt(*s) (the norm of the new Arnoldi vector from its reduced square)
__global__ void sqrt_inplace_kernel(double* __restrict__ s) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *s = sqrt(*s);
}
int launch_sqrt_inplace(alfi_ctx* ctx, double* s) {
  hipLaunchKernelGGL(sqrt_inplace_kernel, dim3(1), dim3(64), 0, ctx->stream, s);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
