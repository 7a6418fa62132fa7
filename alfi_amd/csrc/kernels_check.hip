// Verification of the stored patch inverses and repair of the ones that fail it.
//
// The reference factors its patches with LAPACK's pivoted LU (patch_sub_pc_type lu + patch_pc_patch_dense_inverse,
// alfi/solver.py:599-602; UMFPACK for Scott-Vogelius, :655-659).  The fast inversion kernels here (kernels_patch.hip,
// kernels_bigpatch.hip) eliminate WITHOUT pivoting, which is backward stable for the SPD-dominated patch operators of the
// shipped problems but not for an arbitrary Newton / SUPG Jacobian at high Reynolds number.  So every factorisation is
// followed by a probe of every patch,
//
//     rho_p = || A_p (X_p e_p) - e_p ||_inf,       e a fixed vector of +-1 (by dof),
//
// (X_p e_p by the level's own apply kernels -- so the probe covers whatever storage the factors have: row pieces, large
// patches, condensed -- then one pass over the patch's operator rows), and every patch with rho_p > tol -- or a non-finite
// inverse -- is re-gathered and re-inverted by Gauss-Jordan WITH partial pivoting (one workgroup per flagged patch, work
// matrix in global scratch), then probed again.  alfi_patches_check reports the worst residual and the counts.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "common.h"

namespace {

__device__ __forceinline__ double probe_entry(int64_t dof) {
  uint32_t h = (uint32_t)dof * 2654435761u;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  return (h & 1u) ? 1.0 : -1.0;
}

__device__ __forceinline__ double wave_sum_chk(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// position of patch dof `gcol` in the ascending list dofs_s[0..n), or -1
__device__ __forceinline__ int find_dof(const int32_t* dofs_s, int n, int gcol) {
  int a = 0, b = n;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (dofs_s[mid] < gcol) a = mid + 1; else b = mid;
  }
  return (a < n && dofs_s[a] == gcol) ? a : -1;
}

__global__ void probe_fill_kernel(double* __restrict__ e, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    e[i] = probe_entry(i);
}

// one workgroup per patch of [p0, p0 + gridDim.x).  The level's own apply kernels (whatever the storage of the factors: row pieces, large
// patches, condensed) have put y_p = X_p e_p into the staging buffer; this kernel forms A_p y_p - e_p from the
// operator rows.  Dynamic LDS: n int32 + n doubles.
template <int BS>
__global__ __launch_bounds__(256) void patch_check_kernel(int64_t p0, const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ colidx,
                                                           const double* __restrict__ vals, int flat,
                                                           const int64_t* __restrict__ patch_ptr,
                                                           const int32_t* __restrict__ patch_dofs,
                                                           const int64_t* __restrict__ stage_ptr,
                                                           const double* __restrict__ stage, double tol,
                                                           unsigned long long* __restrict__ worst_bits,
                                                           int32_t* __restrict__ flagged, int* __restrict__ nflag, int cap,
                                                           const int64_t* __restrict__ fc_ptr, const int32_t* __restrict__ fc_col,
                                                           const int32_t* __restrict__ fc_fac, const double* __restrict__ fc_s,
                                                           const double* __restrict__ fc_beta, double fc_scale) {
  extern __shared__ unsigned char smem[];
  const int64_t p = p0 + blockIdx.x;
  const int64_t off = patch_ptr[p];
  const int n = (int)(patch_ptr[p + 1] - off);
  double* y_s = reinterpret_cast<double*>(smem);
  int32_t* dofs_s = reinterpret_cast<int32_t*>(y_s + n);
  __shared__ double wmax_s[4];
  const double* yp = stage + stage_ptr[p];
  for (int i = threadIdx.x; i < n; i += 256) {
    dofs_s[i] = patch_dofs[off + i];
    y_s[i] = yp[i];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double wmax = 0.0;
  for (int r = wave; r < n; r += 4) {
    const int gr = dofs_s[r];
    const int brow = gr / BS, rr = gr % BS;
    const int32_t lo = rowptr[brow], hi = rowptr[brow + 1];
    const int nent = (hi - lo) * BS;
    double acc = 0.0;
    for (int e = lane; e < nent; e += 64) {
      const int blk = e / BS, cc = e % BS;
      const int a = find_dof(dofs_s, n, (colidx[lo + blk] & 0x7fffffff) * BS + cc);
      if (a >= 0) acc = __builtin_fma(vals[bsr_val_index(flat, lo + blk, rr * BS + cc, BS * BS)], y_s[a], acc);
    }
    acc = wave_sum_chk(acc);
    if (fc_ptr) {              // a Burman level: the patch matrix is A[P, P] minus the facet terms PCPATCH leaves out
      const int64_t rn = off / BS + r / BS;
      for (int64_t q = fc_ptr[rn]; q < fc_ptr[rn + 1]; ++q)
        acc -= fc_scale * fc_beta[fc_fac[q]] * fc_s[q] * y_s[fc_col[q] * BS + r % BS];
    }
    const double res = fabs(acc - probe_entry(gr));
    if (!(res <= wmax)) wmax = (res == res) ? res : INFINITY;      // NaN -> +inf
  }
  if (lane == 0) wmax_s[wave] = wmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = fmax(fmax(wmax_s[0], wmax_s[1]), fmax(wmax_s[2], wmax_s[3]));
    atomicMax(worst_bits, (unsigned long long)__double_as_longlong(m));   // m >= 0: the bit patterns order like the values
    if (!(m <= tol)) {
      const int slot = atomicAdd(nflag, 1);
      if (slot < cap) flagged[slot] = (int32_t)p;
    }
  }
}

// LU with partial pivoting + two triangular sweeps, one workgroup per flagged patch (what LAPACK's getrf + getri amount to):
// gather A_p into the n x n row-major scratch W, factor P A = L U in place, then X = U^-1 (L^-1 P) row by row into the
// second scratch Y (every thread owns columns of X: coalesced, no reduction), store in the row-piece layout.
// (Round 2 re-inverted by Gauss-JORDAN with partial pivoting.  Its right residual || A X - I || grows like cond(A)^2 eps:
// on config 4's patches, cond ~ 1e7, it returned 2e-3 where the UNPIVOTED register kernel it was meant to back up gives
// 5e-8 -- found in round 3 by flagging every patch (ALFI_PATCH_CHECK_TOL=3e-9, scripts/repair_check.py).  Solving
// A x_j = e_j column by column through the LU factors is backward stable per column: cond(A) eps.)
// DENSE: the matrix is not gathered from the level operator but copied from ``dense`` (row-major, leading dimension
// ``dense_ld``) -- the Schur complement of a condensed patch (patch_ptr = CondDev::sptr, inv = CondDev::sinv).
// fc (a Burman level, fc.ptr != NULL): the patch matrix is A[P, P] minus the facet terms PCPATCH leaves out, as in
// patch_facet_correct_kernel and patch_check_kernel -- a thread per patch row subtracts its entries after the gather.
struct RepairFacetRule {
  const int64_t* ptr = nullptr;
  const int32_t* col = nullptr;
  const int32_t* fac = nullptr;
  const double* s = nullptr;
  const double* beta = nullptr;
  double scale = 0.0;
};

template <int BS, bool DENSE>
__global__ __launch_bounds__(256) void patch_repair_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                            const double* __restrict__ vals, int flat,
                                                            const int64_t* __restrict__ patch_ptr,
                                                            const int32_t* __restrict__ patch_dofs,
                                                            const int64_t* __restrict__ inv_ptr, double* __restrict__ inv,
                                                            const int32_t* __restrict__ list, double* __restrict__ scratch,
                                                            int64_t scratch_stride, int* __restrict__ status,
                                                            const double* __restrict__ dense, int dense_ld,
                                                            RepairFacetRule fc) {
  extern __shared__ unsigned char smem[];
  const int64_t p = list[blockIdx.x];
  const int64_t off = patch_ptr[p];
  const int n = (int)(patch_ptr[p + 1] - off);
  const int ld = (n + 1) & ~1;
  double* prow = reinterpret_cast<double*>(smem);        // n: pivot row
  double* mcol = prow + n;                               // n: multipliers of the pivot column
  int32_t* dofs_s = reinterpret_cast<int32_t*>(mcol + n);   // n
  int32_t* perm = dofs_s + n;                            // n: row k was exchanged with row perm[k] at step k
  __shared__ double red_v[256];
  __shared__ int red_i[256];
  __shared__ int bad_s;
  double* W = scratch + (int64_t)blockIdx.x * scratch_stride;     // L \ U
  double* Y = W + (int64_t)n * n;                                   // L^-1 P, then X
  const int tid = threadIdx.x;
  if (tid == 0) bad_s = 0;
  if (DENSE) {
    for (int64_t e = tid; e < (int64_t)n * n; e += 256) W[e] = dense[(e / n) * dense_ld + e % n];
  } else {
    for (int i = tid; i < n; i += 256) dofs_s[i] = patch_dofs[off + i];
    for (int64_t e = tid; e < (int64_t)n * n; e += 256) W[e] = 0.0;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < n && !DENSE; r += 4) {
    const int gr = dofs_s[r];
    const int brow = gr / BS, rr = gr % BS;
    const int32_t lo = rowptr[brow], hi = rowptr[brow + 1];
    const int nent = (hi - lo) * BS;
    for (int e = lane; e < nent; e += 64) {
      const int blk = e / BS, cc = e % BS;
      const int a = find_dof(dofs_s, n, (colidx[lo + blk] & 0x7fffffff) * BS + cc);
      if (a >= 0) W[(int64_t)r * n + a] = vals[bsr_val_index(flat, lo + blk, rr * BS + cc, BS * BS)];
    }
  }
  __syncthreads();
  if (!DENSE && fc.ptr) {
    for (int r = tid; r < n; r += 256) {
      const int64_t rn = off / BS + r / BS;
      for (int64_t q = fc.ptr[rn]; q < fc.ptr[rn + 1]; ++q) {
        const int c = fc.col[q] * BS + r % BS;
        if (c < n) W[(int64_t)r * n + c] -= fc.scale * fc.beta[fc.fac[q]] * fc.s[q];
      }
    }
    __syncthreads();
  }
  // ---- P A = L U
  for (int k = 0; k < n; ++k) {
    // pivot search: largest |W[i][k]|, i >= k (ties: smallest i)
    double bv = -1.0;
    int bi = k;
    for (int i = k + tid; i < n; i += 256) {
      const double v = fabs(W[(int64_t)i * n + k]);
      if (v > bv) { bv = v; bi = i; }
    }
    red_v[tid] = bv;
    red_i[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        const double ov = red_v[tid + s];
        const int oi = red_i[tid + s];
        if (ov > red_v[tid] || (ov == red_v[tid] && oi < red_i[tid])) { red_v[tid] = ov; red_i[tid] = oi; }
      }
      __syncthreads();
    }
    const int pr = red_i[0];
    const double pv = red_v[0];
    if (!(pv > 0.0) || pv == INFINITY) {       // zero / NaN / inf pivot column: singular to working precision
      if (tid == 0) bad_s = 1;
      __syncthreads();
      break;
    }
    if (tid == 0) perm[k] = pr;
    if (pr != k)
      for (int j = tid; j < n; j += 256) {     // whole rows: the multipliers already stored move with their rows
        const double t = W[(int64_t)k * n + j];
        W[(int64_t)k * n + j] = W[(int64_t)pr * n + j];
        W[(int64_t)pr * n + j] = t;
      }
    __syncthreads();
    const double ip = 1.0 / W[(int64_t)k * n + k];
    for (int j = k + 1 + tid; j < n; j += 256) {
      prow[j] = W[(int64_t)k * n + j];
      const double l = W[(int64_t)j * n + k] * ip;
      mcol[j] = l;
      W[(int64_t)j * n + k] = l;
    }
    __syncthreads();
    const int m = n - k - 1;                   // trailing block (k+1 .. n-1)^2
    for (int64_t e = tid; e < (int64_t)m * m; e += 256) {
      const int i = k + 1 + (int)(e / m), j = k + 1 + (int)(e % m);
      W[(int64_t)i * n + j] = __builtin_fma(-mcol[i], prow[j], W[(int64_t)i * n + j]);
    }
    __syncthreads();
  }
  if (bad_s) {
    if (tid == 0) atomicExch(status, 1);
    return;
  }
  // ---- Y = L^-1 P: thread c owns column c; (P e_c) = e_q with q = where the row exchanges move row c ... followed forward
  for (int c = tid; c < n; c += 256) {
    // P applied to the identity: row r of P is e_{src(r)}; build column c of P = position q with src(q) == c
    int q = c;
    // the exchanges were applied to ROWS in order k = 0 .. n-1: the row that started at position c ends at position q
    for (int k = 0; k < n; ++k) {
      const int pr = perm[k];
      if (pr != k) {
        if (q == k) q = pr;
        else if (q == pr) q = k;
      }
    }
    for (int i = 0; i < n; ++i) Y[(int64_t)i * n + c] = (i == q) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int i = 1; i < n; ++i) {                // forward: Y[i][:] -= sum_{j < i} L[i][j] Y[j][:]   (unit diagonal)
    for (int c = tid; c < n; c += 256) {
      double acc = Y[(int64_t)i * n + c];
      for (int j = 0; j < i; ++j) acc = __builtin_fma(-W[(int64_t)i * n + j], Y[(int64_t)j * n + c], acc);
      Y[(int64_t)i * n + c] = acc;
    }
    // (thread c only ever touches column c of Y: no barrier needed between the rows)
  }
  for (int i = n - 1; i >= 0; --i) {           // backward: X[i][:] = (Y[i][:] - sum_{j > i} U[i][j] X[j][:]) / U[i][i]
    const double id = 1.0 / W[(int64_t)i * n + i];
    for (int c = tid; c < n; c += 256) {
      double acc = Y[(int64_t)i * n + c];
      for (int j = i + 1; j < n; ++j) acc = __builtin_fma(-W[(int64_t)i * n + j], Y[(int64_t)j * n + c], acc);
      Y[(int64_t)i * n + c] = acc * id;
    }
  }
  __syncthreads();
  double* S = inv + inv_ptr[p];
  for (int64_t e = tid; e < (int64_t)ld * n; e += 256) {
    const int r = (int)(e / n), c = (int)(e % n);
    S[patch_inv_index(r, c, n, ld)] = r < n ? Y[(int64_t)r * n + c] : 0.0;      // r == n: the zero padding row
  }
}

}  // namespace

// probe the patches [p0, p1): e = +-1 by dof (probe_vec), the stage-1 apply of the condensed factors the level holds or of the
// dense FP64 inverses at inv, residual per patch; results accumulate in L->chk (device)
static int launch_check(alfi_level* L, const double* inv, double tol, int64_t p0, int64_t p1, const double* probe_vec) {
  alfi_ctx* ctx = L->ctx;
  if (p1 <= p0) return 0;
  const bool fc = L->fc_ptr && L->fc_scale != 0.0;
  int rc = L->cond ? launch_patch_apply_range(L, p0, p1, probe_vec) : launch_patch_apply_f64_range(L, inv, p0, p1, probe_vec);
  if (rc == 0) {
    const size_t lds = (size_t)L->lay.max_np * (sizeof(double) + sizeof(int32_t));
    unsigned long long* worst = reinterpret_cast<unsigned long long*>(L->chk);
    int* nflag = reinterpret_cast<int*>(L->chk + 1);
    dim3 grid((unsigned)(p1 - p0)), block(256);
    if (L->bs == 2)
      hipLaunchKernelGGL(patch_check_kernel<2>, grid, block, lds, ctx->stream, p0, L->A.rowptr, L->A.colidx, L->A.vals, L->A.flat,
                         L->patch_ptr, L->patch_dofs, L->stage_ptr, L->stage, tol, worst, L->chk_list, nflag, L->chk_cap,
                         fc ? L->fc_ptr : nullptr, L->fc_col, L->fc_fac, L->fc_s, L->fc_beta, L->fc_scale);
    else
      hipLaunchKernelGGL(patch_check_kernel<3>, grid, block, lds, ctx->stream, p0, L->A.rowptr, L->A.colidx, L->A.vals, L->A.flat,
                         L->patch_ptr, L->patch_dofs, L->stage_ptr, L->stage, tol, worst, L->chk_list, nflag, L->chk_cap,
                         fc ? L->fc_ptr : nullptr, L->fc_col, L->fc_fac, L->fc_s, L->fc_beta, L->fc_scale);
    if (hipGetLastError() != hipSuccess) rc = alfi_set_error(ctx, ALFI_E_HIP, "patch_check_kernel launch failed");
  }
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

static int read_check(alfi_level* L, double* worst, int* nflag) {
  alfi_ctx* ctx = L->ctx;
  double h[2];
  ALFI_HIP_CHECK(ctx, hipMemcpyAsync(h, L->chk, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  *worst = h[0];
  int nf;
  memcpy(&nf, &h[1], sizeof(int));
  *nflag = nf;
  return 0;
}

// Condensed factors (CondDev): a patch that fails the probe -- or met a zero pivot -- gets its group matrices X_g, W_g by LU
// WITH partial pivoting (cond_group_pivot_kernel), its Schur complement formed again from them (fill / Schur kernels of the
// setup, one patch at a time: the rare path) and inverted by the pivoted LU above, all in place: the level keeps its condensed
// storage (round 2 fell back to dense inverses for the whole level, 6.8 x the memory exactly when a patch is ill-conditioned;
// round 3 repaired the Schur complement only, so a bad pivot inside one macro-cell group still did).
static int cond_repair(alfi_level* L, double tol, int nflag, double worst, const double* probe_vec) {
  alfi_ctx* ctx = L->ctx;
  const int smax = L->cplan.max_s;
  if (smax > 4096)
    return alfi_set_error(ctx, ALFI_E_SINGULAR, "%d condensed patch factors fail the residual probe (worst %.3e) and the "
                          "pivoted repair handles Schur complements of at most 4096 dofs", nflag, worst);
  std::vector<int32_t> list((size_t)nflag);
  ALFI_HIP_CHECK(ctx, hipMemcpyAsync(list.data(), L->chk_list, sizeof(int32_t) * (size_t)nflag, hipMemcpyDeviceToHost, ctx->stream));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const int64_t N = ((int64_t)smax + 63) / 64 * 64;
  double *sig = nullptr, *scratch = nullptr;
  int64_t* zero = nullptr;
  ALFI_HIP_CHECK(ctx, hipMalloc((void**)&sig, sizeof(double) * (size_t)(N * N)));
  hipError_t e = hipMalloc((void**)&scratch, sizeof(double) * (size_t)(2 * (int64_t)smax * smax));
  if (e == hipSuccess) e = hipMalloc((void**)&zero, sizeof(int64_t));
  if (e == hipSuccess) e = hipMemsetAsync(zero, 0, sizeof(int64_t), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(L->status, 0, sizeof(int), ctx->stream);
  const size_t lds = (size_t)smax * (2 * sizeof(double) + 2 * sizeof(int32_t));
  if (e == hipSuccess && lds > 64 * 1024)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_repair_kernel<3, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  int rc = e == hipSuccess ? 0 : alfi_set_error(ctx, ALFI_E_HIP, "condensed repair: %s", hipGetErrorString(e));
  for (int i = 0; i < nflag && rc == 0; ++i) {
    const int64_t p = list[(size_t)i];
    const int sp = (int)(L->cplan.sptr[p + 1] - L->cplan.sptr[p]);
    if (sp == 0) continue;
    rc = launch_cond_schur_one(L, p, zero, sig);
    if (rc != 0) break;
    const int Np = (sp + 63) / 64 * 64;              // the padded leading dimension of the setup's Schur scratch (BIG_NB)
    hipLaunchKernelGGL((patch_repair_kernel<3, true>), dim3(1), dim3(256), lds, ctx->stream, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, (const double*)nullptr, 0, L->cd.sptr, (const int32_t*)nullptr, L->cd.sinv_ptr,
                       L->cd.sinv, L->chk_list + i, scratch, (int64_t)0, L->status, (const double*)sig, Np, RepairFacetRule{});
    if (hipGetLastError() != hipSuccess) rc = alfi_set_error(ctx, ALFI_E_HIP, "patch_repair_kernel launch failed");
  }
  int st = 0;
  if (rc == 0 && hipMemcpyAsync(&st, L->status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = ALFI_E_HIP;
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(sig);
  (void)hipFree(scratch);
  (void)hipFree(zero);
  if (rc != 0) return rc;
  if (st != 0) return alfi_set_error(ctx, ALFI_E_SINGULAR, "a condensed patch operator is singular to working precision (pivoted inversion)");
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->chk, 0, 2 * sizeof(double), ctx->stream));
  rc = launch_check(L, nullptr, tol, 0, L->npatch, probe_vec);
  double worst2 = 0.0;
  int nflag2 = 0;
  if (rc == 0) rc = read_check(L, &worst2, &nflag2);
  if (rc != 0) return rc;
  L->chk_repaired = nflag - nflag2;
  L->chk_worst_after = worst2;
  if (nflag2 > 0 && !(worst2 <= alfi_env_patch_check_fail()))
    return alfi_set_error(ctx, ALFI_E_SINGULAR, "%d condensed patch factors still fail the residual probe after pivoted "
                          "re-inversion of their Schur complements (worst %.3e); use dense inverses "
                          "(alfi_patches_set_groups(NULL)) for this operator", nflag2, worst2);
  return 0;
}

// the level's probe vector e (+-1 by dof) on the device; the caller frees it (hipFree)
int patch_probe_vector(alfi_level* L, double** probe_vec) {
  alfi_ctx* ctx = L->ctx;
  double* e = nullptr;
  ALFI_HIP_CHECK(ctx, hipMalloc((void**)&e, sizeof(double) * (size_t)std::max<int64_t>(L->n, 1)));
  hipLaunchKernelGGL(probe_fill_kernel, dim3(1024), dim3(256), 0, ctx->stream, e, L->n);
  if (hipGetLastError() != hipSuccess) {
    (void)hipFree(e);
    return alfi_set_error(ctx, ALFI_E_HIP, "probe_fill_kernel launch failed");
  }
  *probe_vec = e;
  return 0;
}

// what alfi_patches_check reports, from the figures of the ranges (one range: the whole level)
int patch_check_finish(alfi_level* L, const PatchCheckAcc& acc) {
  L->chk_worst = acc.worst;
  L->chk_flagged = acc.flagged;
  L->chk_repaired = acc.repaired;
  L->chk_worst_after = acc.worst_after;
  return 0;
}

// Called by alfi_patches_factor after the fast inversion of the patches [p0, p1): the probe, the repair and the second probe
// (dense FP64 inverses at inv; condensed levels: the factors the level holds, the whole level only).  unpivoted_status: the
// zero-pivot flag of that inversion (a patch that met one holds non-finite entries and is caught by the probe).
// A level factored range by range sees in *acc what one pass over all its patches would have reported: the worst first residual,
// the flagged and repaired counts, and the worst residual of the inverses it ends up with.
int patch_verify_and_repair_range(alfi_level* L, double* inv, int unpivoted_status, int64_t p0, int64_t p1,
                                  const double* probe_vec, PatchCheckAcc* acc) {
  alfi_ctx* ctx = L->ctx;
  const bool enabled = alfi_env_patch_check();
  const double tol = alfi_env_patch_check_tol();
  if (!enabled || p1 <= p0) {
    if (unpivoted_status != 0) return alfi_set_error(ctx, ALFI_E_SINGULAR, "zero pivot while inverting a patch operator");
    return 0;
  }
  if (!L->chk) {
    ALFI_HIP_CHECK(ctx, hipMalloc((void**)&L->chk, 2 * sizeof(double)));
    L->chk_cap = (int)std::min<int64_t>(L->npatch, 1 << 20);
    ALFI_HIP_CHECK(ctx, hipMalloc((void**)&L->chk_list, sizeof(int32_t) * (size_t)L->chk_cap));
  }
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->chk, 0, 2 * sizeof(double), ctx->stream));
  ALFI_CHECK(launch_check(L, inv, tol, p0, p1, probe_vec));
  double worst = 0.0;
  int nflag = 0;
  ALFI_CHECK(read_check(L, &worst, &nflag));
  acc->worst = std::max(acc->worst, worst);
  acc->flagged += nflag;
  if (nflag == 0) {
    acc->worst_after = std::max(acc->worst_after, worst);
    return 0;
  }
  if (nflag > L->chk_cap)
    return alfi_set_error(ctx, ALFI_E_SINGULAR, "%d of %lld patch inverses fail the residual probe (worst %.3e)", nflag,
                          (long long)(p1 - p0), worst);
  constexpr int REPAIR_MAX_NP = PATCH_MAX;     // (a 2000-dof patch takes ~0.5 s of one workgroup: a rare-path safety net)
  if (L->cond) {
    L->chk_repaired = 0;
    const int rc = cond_repair(L, tol, nflag, worst, probe_vec);
    acc->repaired += L->chk_repaired;
    if (rc == 0) acc->worst_after = L->chk_worst_after;
    return rc;
  }
  // a Burman level: the repair subtracts the facet terms PCPATCH leaves out from the gathered matrix (RepairFacetRule)
  RepairFacetRule fc;
  if (L->fc_ptr && L->fc_scale != 0.0) fc = RepairFacetRule{L->fc_ptr, L->fc_col, L->fc_fac, L->fc_s, L->fc_beta, L->fc_scale};
  if (L->lay.max_np > REPAIR_MAX_NP)
    return alfi_set_error(ctx, ALFI_E_SINGULAR, "%d patch inverses fail the residual probe (worst %.3e) and the pivoted "
                          "repair handles patches of at most %d dofs", nflag, worst, (int)REPAIR_MAX_NP);
  // pivoted re-inversion of the flagged patches, in batches bounded by 1 GiB of scratch
  const int64_t stride = 2 * (int64_t)L->lay.max_np * L->lay.max_np;      // L \ U and the inverse being built
  const int64_t per_batch = std::max<int64_t>(1, ((int64_t)1 << 27) / stride);
  double* scratch = nullptr;
  ALFI_HIP_CHECK(ctx, hipMalloc((void**)&scratch, sizeof(double) * (size_t)(std::min<int64_t>(per_batch, nflag) * stride)));
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->status, 0, sizeof(int), ctx->stream));
  const size_t lds = (size_t)L->lay.max_np * (2 * sizeof(double) + 2 * sizeof(int32_t));
  int rc = 0;
  if (lds > 64 * 1024) {     // beyond the default dynamic LDS limit (gfx950: 160 KB per CU)
    hipError_t ea = L->bs == 2 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_repair_kernel<2, false>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                               : hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_repair_kernel<3, false>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) rc = alfi_set_error(ctx, ALFI_E_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(ea));
  }
  for (int64_t b0 = 0; b0 < nflag && rc == 0; b0 += per_batch) {
    const int64_t nb = std::min<int64_t>(per_batch, nflag - b0);
    dim3 grid((unsigned)nb), block(256);
    if (L->bs == 2)
      hipLaunchKernelGGL((patch_repair_kernel<2, false>), grid, block, lds, ctx->stream, L->A.rowptr, L->A.colidx, L->A.vals,
                         L->A.flat, L->patch_ptr, L->patch_dofs, L->inv_ptr, inv, L->chk_list + b0, scratch, stride,
                         L->status, (const double*)nullptr, 0, fc);
    else
      hipLaunchKernelGGL((patch_repair_kernel<3, false>), grid, block, lds, ctx->stream, L->A.rowptr, L->A.colidx, L->A.vals,
                         L->A.flat, L->patch_ptr, L->patch_dofs, L->inv_ptr, inv, L->chk_list + b0, scratch, stride,
                         L->status, (const double*)nullptr, 0, fc);
    if (hipGetLastError() != hipSuccess) rc = alfi_set_error(ctx, ALFI_E_HIP, "patch_repair_kernel launch failed");
  }
  int st = 0;
  if (rc == 0 && hipMemcpyAsync(&st, L->status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = ALFI_E_HIP;
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(scratch);
  if (rc != 0) return rc;
  if (st != 0) return alfi_set_error(ctx, ALFI_E_SINGULAR, "a patch operator is singular to working precision (pivoted inversion)");
  ALFI_CHECK(build_patch_il(L, inv)); // small-patch levels: the repaired inverses into the interleaved copy the apply streams
  // probe again (every patch of the range, the untouched ones included)
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->chk, 0, 2 * sizeof(double), ctx->stream));
  rc = launch_check(L, inv, tol, p0, p1, probe_vec);
  double worst2 = 0.0;
  int nflag2 = 0;
  if (rc == 0) rc = read_check(L, &worst2, &nflag2);
  if (rc != 0) return rc;
  acc->repaired += nflag - nflag2;
  acc->worst_after = std::max(acc->worst_after, worst2);
  // A patch that stays above the tolerance after a pivoted LU inversion is ill-conditioned, not mis-factored: the probe
  // residual of a backward-stable inverse scales like cond(A_p) eps (gamma / nu h^-2 eps: 5e-8 at Re 5000 on the shipped
  // meshes, more on finer levels at Re 10 000).  LAPACK -- the reference's patch solver -- would hand back the same
  // inverse without complaint, so this is reported (alfi_patches_check: worst residual afterwards, flagged != repaired), not
  // an error; only a residual beyond ALFI_PATCH_CHECK_FAIL (default 1000 x the tolerance) or a non-finite one fails the setup.
  if (nflag2 > 0 && !(worst2 <= alfi_env_patch_check_fail()))
    return alfi_set_error(ctx, ALFI_E_SINGULAR, "%d patch inverses still fail the residual probe after pivoted re-inversion "
                          "(worst %.3e): the patch operators are singular to working precision", nflag2, worst2);
  return 0;
}
