// Block right-hand sides on condensed patch factors: the workgroup-per-patch apply of kernels_bigpatch.hip (cond_front /
// cond_sigma / cond_back, launches of at least COND_PER_PATCH_MIN patches) for NV = 2 .. 4 vectors per stream of X_g, B_g, W_g
// and inv(Sigma).
//
// The contract is that of kernels_block.hip: column c of the result is the single-vector apply on column c BIT FOR BIT.  Every
// kernel here is its one-vector original with the per-vector state held NV times -- the same lane owns the same row pair, the
// same wave the same rows of inv(Sigma), every loop runs to the same bound (the wave maximum of cond_row2_dot included), and per
// right-hand side the products and sums happen in the original's order.  What is loaded once for the NV vectors: the group
// matrices, inv(Sigma), every table of the plan.
//
// LDS operands are interleaved entry by entry (v[i * NV + c]): NV x the one-vector kernel's dynamic LDS, which is what the
// width rule (block_cols.h: block_cond_width) budgets.  Per-column scratch: t and y_S through `ctmp` (slots of sum_n doubles,
// the block twin of CondDev::tmp), the Schur right-hand side and the staged result through `stage` (slots of lay.stage_len).
#include "common.h"
#include "row_piece.h"
#include "block_cols.h"
#include "cond_apply.h"

template <bool NT, int COND_WAVES, int RU, int NV>
__global__ __launch_bounds__(64 * COND_WAVES) void cond_front_block_kernel(int64_t p0, int64_t p1, CondDev cd,
                                                                           const int64_t* __restrict__ patch_ptr,
                                                                           const int64_t* __restrict__ stage_ptr,
                                                                           const double* __restrict__ X, int64_t ldx, BlockCols cols,
                                                                           double* __restrict__ stage, int64_t stage_len,
                                                                           double* __restrict__ ctmp, int64_t ctmp_len, int ordered) {
  extern __shared__ double cond_dsmem[];
  constexpr int NT_ = 64 * COND_WAVES;
  if (p0 + blockIdx.x >= p1) return;
  const int64_t p = ordered ? cd.order[blockIdx.x] : p0 + blockIdx.x;
  const int64_t off = patch_ptr[p];
  const int n = (int)(patch_ptr[p + 1] - off);
  const int nI = cd.p_nI[p];
  const int s = n - nI;
  const int64_t uo0 = cd.uptr[p];
  double* xs = cond_dsmem;          // n x NV
  double* ts = xs + n * NV;         // nI x NV
  double* us = ts + nI * NV;        // u buffer x NV, in the order the right-hand side sums it (u_dst)
  // gather x: 4 index loads, then 4 x NV value loads in flight per thread
  for (int i0 = threadIdx.x; i0 < n; i0 += 4 * NT_) {
    int32_t d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = (i0 + u * NT_ < n) ? cd.dofs[off + i0 + u * NT_] : 0;
    double v[4][NV];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < NV; ++c) v[u][c] = (i0 + u * NT_ < n) ? X[(int64_t)cols.c[c] * ldx + d[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u * NT_ < n) {
#pragma unroll
        for (int c = 0; c < NV; ++c) xs[(i0 + u * NT_) * NV + c] = v[u][c];
      }
  }
  __syncthreads();
  double* tmp = ctmp + off;
  // t = X x, a lane per pair of interior entries
  const int64_t xp0 = cd.xp_ptr[p], bp0 = cd.bp_ptr[p];
  const int nxp = (int)(cd.xp_ptr[p + 1] - xp0), nbp = (int)(cd.bp_ptr[p + 1] - bp0);
  for (int q0 = 0; q0 < nxp; q0 += NT_) {
    const int q = q0 + threadIdx.x;
    const bool act = q < nxp;
    const int32_t g = act ? cd.xp_grp[xp0 + q] : (int32_t)cd.gptr[p];
    const int m = cd.g_m[g], o = cd.g_off[g], i = 2 * (q - cd.g_xp[g]);
    double t[NV][2];
#pragma unroll
    for (int c = 0; c < NV; ++c) t[c][0] = t[c][1] = 0.0;
    cond_row2_dot<NT, RU, NV>(cd.mat + cd.g_mat[g] + i, cond_ldim(m), act ? m : 0, xs + o * NV, t);
    if (act) {
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        ts[(o + i) * NV + c] = t[c][0];
        tmp[c * ctmp_len + o + i] = t[c][0];
        if (i + 1 < m) {
          ts[(o + i + 1) * NV + c] = t[c][1];
          tmp[c * ctmp_len + o + i + 1] = t[c][1];
        }
      }
    }
  }
  __syncthreads();
  // u = B t, a lane per pair of entries of the patch's u buffer
  for (int q0 = 0; q0 < nbp; q0 += NT_) {
    const int q = q0 + threadIdx.x;
    const bool act = q < nbp;
    const int32_t g = act ? cd.bp_grp[bp0 + q] : (int32_t)cd.gptr[p];
    const int m = cd.g_m[g], sc = cd.g_sc[g], j = 2 * (q - cd.g_bp[g]);
    const int64_t ue = uo0 + cd.g_uoff[g] + j;
    const int32_t d0 = act ? cd.u_dst[ue] : 0, d1 = (act && j + 1 < sc) ? cd.u_dst[ue + 1] : 0;
    double u[NV][2];
#pragma unroll
    for (int c = 0; c < NV; ++c) u[c][0] = u[c][1] = 0.0;
    cond_row2_dot<NT, RU, NV>(cd.mat + cd.g_mat[g] + (int64_t)cond_ldim(m) * m + j, cond_ldim(sc), act ? m : 0,
                              ts + cd.g_off[g] * NV, u);
    if (act) {
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        us[d0 * NV + c] = u[c][0];
        if (j + 1 < sc) us[d1 * NV + c] = u[c][1];
      }
    }
  }
  __syncthreads();
  // right-hand side of the Schur system: the contributions to a row are adjacent in us, summed in ascending order
  const int64_t srow0 = cd.sptr[p];
  const int32_t qb = cd.s_uptr[srow0];
  double* rhs = stage + stage_ptr[p] + nI;
  for (int i = threadIdx.x; i < s; i += NT_) {
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = xs[(nI + i) * NV + c];
    const int32_t qe = cd.s_uptr[srow0 + i + 1] - qb;
    for (int32_t q = cd.s_uptr[srow0 + i] - qb; q < qe; ++q) {
#pragma unroll
      for (int c = 0; c < NV; ++c) acc[c] -= us[q * NV + c];
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) rhs[c * stage_len + i] = acc[c];
  }
}

template <bool NT, int NV>
__global__ __launch_bounds__(256) void cond_sigma_block_kernel(int64_t c0, CondDev cd, const int64_t* __restrict__ patch_ptr,
                                                               const int64_t* __restrict__ stage_ptr,
                                                               const double* __restrict__ stage, int64_t stage_len,
                                                               double* __restrict__ ctmp, int64_t ctmp_len) {
  extern __shared__ double cond_dsmem[];
  const int64_t c = c0 + blockIdx.x;
  const int64_t p = cd.ch_patch[c];
  const int r0 = cd.ch_row[c];
  const int64_t off = patch_ptr[p];
  const int n = (int)(patch_ptr[p + 1] - off);
  const int nI = cd.p_nI[p];
  const int s = n - nI;
  const int ld = (s + 1) & ~1;
  const double* rhs = stage + stage_ptr[p] + nI;
  const int r1 = min(ld, r0 + COND_SIGMA_ROWS);
  const int share = (((r1 - r0) + 3) / 4 + 15) & ~15;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int a = r0 + wave * share, b = min(r1, a + share);
  // the first block of the wave's share is requested whole before the right-hand sides are in LDS, as in the one-vector kernel
  int row0 = 0, P = 2, R = 2;
  if (a < b) big_block(ld, a, b, row0, P, R);
  const int lg = __builtin_ctz(R) - 1;
  const bool ahead = a < b && s <= BIG_U * (64 >> lg);      // wave-uniform
  big_d2 sv[BIG_U];
  if (ahead) big_block_prefetch<NT>(cd.sinv + cd.sinv_ptr[p] + (int64_t)row0 * s + (a - row0), P, s, lg, lane, sv);
  for (int i = threadIdx.x; i < s; i += 256) {
#pragma unroll
    for (int v = 0; v < NV; ++v) cond_dsmem[i * NV + v] = rhs[v * stage_len + i];
  }
  __syncthreads();
  double* ys = ctmp + off + nI;
  if (ahead) {
    big_block_finish<NV>(sv, s, lg, cond_dsmem, lane, ys + a, ctmp_len, s - a);
    if (a + R < b) big_rows<NT, NV>(cd.sinv + cd.sinv_ptr[p], s, ld, a + R, b, cond_dsmem, lane, ys, ctmp_len);
  } else if (a < b) {
    big_rows<NT, NV>(cd.sinv + cd.sinv_ptr[p], s, ld, a, b, cond_dsmem, lane, ys, ctmp_len);
  }
}

template <bool NT, int COND_WAVES, int RU, int NV>
__global__ __launch_bounds__(64 * COND_WAVES) void cond_back_block_kernel(int64_t p0, int64_t p1, CondDev cd,
                                                                          const int64_t* __restrict__ patch_ptr,
                                                                          const int64_t* __restrict__ stage_ptr,
                                                                          double* __restrict__ stage, int64_t stage_len,
                                                                          const double* __restrict__ ctmp, int64_t ctmp_len,
                                                                          int ordered) {
  extern __shared__ double cond_dsmem[];
  constexpr int NT_ = 64 * COND_WAVES;
  if (p0 + blockIdx.x >= p1) return;
  const int64_t p = ordered ? cd.order[blockIdx.x] : p0 + blockIdx.x;
  const int64_t off = patch_ptr[p];
  const int n = (int)(patch_ptr[p + 1] - off);
  const int nI = cd.p_nI[p];
  const int s = n - nI;
  const int uo = (int)(cd.uptr[p + 1] - cd.uptr[p]);
  const int64_t g0 = cd.gptr[p];
  double* ys = cond_dsmem;          // s x NV
  double* yg = ys + s * NV;         // uo x NV: y_S[S_g], group after group (the layout of the u buffer)
  const double* tmp = ctmp + off;
  for (int i = threadIdx.x; i < s; i += NT_) {
#pragma unroll
    for (int c = 0; c < NV; ++c) ys[i * NV + c] = tmp[c * ctmp_len + nI + i];
  }
  // the positions S_g of all groups (adjacent in sidx), 4 loads in flight per thread
  const int32_t* si = cd.sidx + (uo > 0 ? cd.g_sidx[g0] : 0);
  int32_t sq[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) sq[u] = (threadIdx.x + u * NT_ < uo) ? si[threadIdx.x + u * NT_] : 0;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (threadIdx.x + u * NT_ < uo) {
#pragma unroll
      for (int c = 0; c < NV; ++c) yg[(threadIdx.x + u * NT_) * NV + c] = ys[sq[u] * NV + c];
    }
  for (int q = threadIdx.x + 4 * NT_; q < uo; q += NT_) {
    const int32_t sp = si[q];
#pragma unroll
    for (int c = 0; c < NV; ++c) yg[q * NV + c] = ys[sp * NV + c];
  }
  __syncthreads();
  double* out = stage + stage_ptr[p];
  // y_g = t_g - W_g y_S[S_g], a lane per pair of interior entries
  const int64_t xp0 = cd.xp_ptr[p];
  const int nxp = (int)(cd.xp_ptr[p + 1] - xp0);
  for (int q0 = 0; q0 < nxp; q0 += NT_) {
    const int q = q0 + threadIdx.x;
    const bool act = q < nxp;
    const int32_t g = act ? cd.xp_grp[xp0 + q] : (int32_t)g0;
    const int m = cd.g_m[g], sc = cd.g_sc[g], o = cd.g_off[g], i = 2 * (q - cd.g_xp[g]);
    const int ldm = cond_ldim(m);
    double tg[NV][2];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      tg[c][0] = act ? tmp[c * ctmp_len + o + i] : 0.0;
      tg[c][1] = (act && i + 1 < m) ? tmp[c * ctmp_len + o + i + 1] : 0.0;
    }
    const int32_t sl0 = act ? cd.slot[off + o + i] : 0, sl1 = (act && i + 1 < m) ? cd.slot[off + o + i + 1] : 0;
    double y[NV][2];
#pragma unroll
    for (int c = 0; c < NV; ++c) y[c][0] = y[c][1] = 0.0;
    cond_row2_dot<NT, RU, NV>(cd.mat + cd.g_mat[g] + (int64_t)ldm * m + (int64_t)cond_ldim(sc) * m + i, ldm, act ? sc : 0,
                              yg + cd.g_uoff[g] * NV, y);
    if (act) {
#pragma unroll
      for (int c = 0; c < NV; ++c) {
        out[c * stage_len + sl0] = tg[c][0] - y[c][0];
        if (i + 1 < m) out[c * stage_len + sl1] = tg[c][1] - y[c][1];
      }
    }
  }
  for (int i = threadIdx.x; i < s; i += NT_) {
    const int32_t sl = cd.slot[off + nI + i];
#pragma unroll
    for (int c = 0; c < NV; ++c) out[c * stage_len + sl] = ys[i * NV + c];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------------------------------------------------
template <int WV, int NV>
static int launch_cond_block_nv(alfi_level* L, const BlockCols& cols, const double* X, int64_t ldx, double* stage, double* ctmp) {
  alfi_ctx* ctx = L->ctx;
  const int64_t npatch = L->npatch, stage_len = L->lay.stage_len, ctmp_len = L->lay.sum_n;
  const int64_t c0 = L->cplan.chptr[0], c1 = L->cplan.chptr[npatch];
  const int ordered = L->cd.order ? 1 : 0;         // a full-range launch: the patches largest first, as the single launcher
  const size_t lds_f = (size_t)NV * L->cplan.lds_front, lds_b = (size_t)NV * L->cplan.lds_back;
  const size_t lds_s = (size_t)NV * (L->cplan.max_s + 2) * sizeof(double);
  const dim3 grid((unsigned)npatch), block(64 * WV);
  // (only a budget above the default, alfi_ctx_set_block_lds_bytes, brings a launch here above 64 KiB)
  if (lds_f > 64 * 1024)
    ALFI_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&cond_front_block_kernel<false, WV, 8, NV>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f));
  hipLaunchKernelGGL((cond_front_block_kernel<false, WV, 8, NV>), grid, block, lds_f, ctx->stream, (int64_t)0, npatch, L->cd,
                     L->patch_ptr, L->stage_ptr, X, ldx, cols, stage, stage_len, ctmp, ctmp_len, ordered);
  if (c1 > c0)
    hipLaunchKernelGGL((cond_sigma_block_kernel<true, NV>), dim3((unsigned)(c1 - c0)), dim3(256), lds_s, ctx->stream, c0, L->cd,
                       L->patch_ptr, L->stage_ptr, stage, stage_len, ctmp, ctmp_len);
  if (lds_b > 64 * 1024)
    ALFI_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&cond_back_block_kernel<false, WV, 8, NV>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
  hipLaunchKernelGGL((cond_back_block_kernel<false, WV, 8, NV>), grid, block, lds_b, ctx->stream, (int64_t)0, npatch, L->cd,
                     L->patch_ptr, L->stage_ptr, stage, stage_len, ctmp, ctmp_len, ordered);
  ALFI_HIP_CHECK(ctx, hipGetLastError());
  return 0;
}
template <int WV>
static int launch_cond_block_w(alfi_level* L, const BlockCols& cols, const double* X, int64_t ldx, double* stage, double* ctmp) {
  switch (cols.n) {
    case 2: return launch_cond_block_nv<WV, 2>(L, cols, X, ldx, stage, ctmp);
    case 3: return launch_cond_block_nv<WV, 3>(L, cols, X, ldx, stage, ctmp);
    default: return launch_cond_block_nv<WV, 4>(L, cols, X, ldx, stage, ctmp);
  }
}

// Both stages of the additive apply for the 2 .. BLOCK_NV columns of cols on a serial level that holds condensed factors and
// has at least COND_PER_PATCH_MIN patches (the whole level: one full-range launch of each kernel).  stage: cols.n x
// lay.stage_len doubles, ctmp: cols.n x lay.sum_n doubles.  The caller has checked that cols.n x max(lds_front, lds_back) is
// within the device's limit (block_cond_width).
int launch_cond_apply_block(alfi_level* L, const BlockCols& cols, const BlockCols& ocols, const double* X, int64_t ldx, double* Y,
                            int64_t ldy, double* stage, double* ctmp) {
  alfi_ctx* ctx = L->ctx;
  if (cols.n < 2 || cols.n > BLOCK_NV || ocols.n != cols.n)
    return alfi_set_error(ctx, ALFI_E_ARG, "a condensed block launch takes 2 .. %d columns", BLOCK_NV);
  if (!L->cond || L->npatch < COND_PER_PATCH_MIN)
    return alfi_set_error(ctx, ALFI_E_STATE, "condensed block apply on a level without the workgroup-per-patch form");
  {
    ProfScope prof(ctx, ALFI_EV_PATCH_APPLY);
    switch (cond_patch_waves(L->cplan.max_pairs)) {
      case 1: ALFI_CHECK((launch_cond_block_w<1>(L, cols, X, ldx, stage, ctmp))); break;
      case 2: ALFI_CHECK((launch_cond_block_w<2>(L, cols, X, ldx, stage, ctmp))); break;
      case 4: ALFI_CHECK((launch_cond_block_w<4>(L, cols, X, ldx, stage, ctmp))); break;
      default: ALFI_CHECK((launch_cond_block_w<8>(L, cols, X, ldx, stage, ctmp))); break;
    }
  }
  if (!Y) return 0;     // stage 1 alone: the caller sums the staged columns itself (kernels_block_fused.hip)
  return launch_patch_sum_block(L, cols, ocols, X, ldx, Y, ldy, stage);
}
