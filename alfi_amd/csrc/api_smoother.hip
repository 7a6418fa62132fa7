// C ABI of libalfi_hip.so (include/alfi_hip.h), the level smoothers: FGMRES(k) (KSPFGMRES + PCPATCH, alfi/solver.py:309-317) and
// Chebyshev(k) (KSPCHEBYSHEV, examples/graddiv/graddiv.py:109-110), and the Arnoldi steps its interval is estimated from.
// (One file per concern since round 5: api_ctx / api_level / api_patches / api_smoother / api_cycles / api_saddle; the helpers they
// share are declared in api_internal.h.)
#include <optional>
#include "api_internal.h"

// ---- FGMRES(k) smoother ----------------------------------------------------------------------------------------------------
// the single call's workspace: grow-only in K (a captured cycle holds its addresses; HsLayout is built from the K it holds)
int ensure_fgmres_workspace(alfi_level* L, int k) {
  if (k <= L->ws.K) return 0;
  if (k > RED_MAXV - 1) return alfi_set_error(L->ctx, ALFI_E_ARG, "k = %d exceeds the supported maximum %d", k, RED_MAXV - 1);
  return krylov_ws_ensure(L->ctx, &L->ws, 1, k, L->n);
}

// FGMRES(k) on a small, unpartitioned level with the additive smoother: four launches per iteration (see the kernels in
// kernels_vec.hip).  Same algorithm as the general path below -- right-preconditioned FGMRES, classical Gram-Schmidt,
// explicit norms -- with the normalisation of the new Krylov vector moved behind the patch solves (they are linear).
static int smooth_fgmres_fused(alfi_level* L, int k, const double* db, double* dx, int nonzero_guess, bool flat_spmv) {
  alfi_ctx* ctx = L->ctx;
  const int K = L->ws.K;
  const int64_t n = L->n, ldv = L->ws.ldv;
  HsLayout hl(K);
  double *V = L->ws.V, *Z = L->ws.Z, *w = L->ws.w, *hs = L->ws.hs;
  double* hdots = hs + hl.hd;
  if (nonzero_guess) {
    ALFI_CHECK(alfi_residual(L, db, dx, w));
  } else {
    ALFI_HIP_CHECK(ctx, hipMemsetAsync(dx, 0, sizeof(double) * n, ctx->stream));
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_copy(ctx, w, db, n));
  }
  {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_norm_partials(ctx, w, n));
  }
  const int G = red_blocks_for(n);
  const double* normpart = ctx->red_partial;
  for (int j = 0; j < k; ++j) {
    double* zj = Z + (int64_t)j * ldv;
    ALFI_CHECK(launch_patch_apply_range(L, 0, L->npatch, w));                                   // stage <- patch solves of w
    {
      ProfScope prof(ctx, ALFI_EV_PATCH_SCATTER);
      ALFI_CHECK(launch_patch_sum_scale(L, w, zj, V + (int64_t)j * ldv, normpart, G, hdots, hs, j, K));   // z_j, v_j, H column j-1
    }
    int nb = 0;
    if (!flat_spmv) {
      ProfScope prof(ctx, ALFI_EV_MATMULT);
      ALFI_CHECK(launch_bsr_spmv_dot(ctx, L->A_own, zj, w, V, ldv, j + 1, ctx->red_partial, &nb));  // w = A z_j, V^T w partials
    } else {
      // long or very uneven block rows (the 3-D operators): the nnz-balanced product, then the dots as their own pass; up to
      // 256 partials per vector the projection kernel sums them itself, beyond a one-block reduction does
      const bool in_consumer = G <= 256;
      {
        ProfScope prof(ctx, ALFI_EV_MATMULT);
        ALFI_CHECK(launch_bsr_spmv(ctx, L->A_own, zj, w, nullptr, 1.0, 0));
      }
      ProfScope prof(ctx, ALFI_EV_BLAS1);   // to the end of the branch
      ALFI_CHECK(launch_multi_dot(ctx, V, ldv, j + 1, w, in_consumer ? nullptr : hdots, n));
      nb = in_consumer ? G : 0;
    }
    ProfScope prof(ctx, ALFI_EV_BLAS1);   // to the end of the loop body
    ALFI_CHECK(launch_multi_axpy_norm(ctx, V, ldv, j + 1, hdots, w, n, ctx->red_partial2, nb));     // h, w -= V h, |w|^2 partials
    normpart = ctx->red_partial2;
  }
  ProfScope prof(ctx, ALFI_EV_BLAS1);   // to the end of the function
  ALFI_CHECK(launch_fgmres_finish_fused(ctx, normpart, G, hdots, hs, k, K));                       // H column k-1, y
  ALFI_CHECK(launch_update_solution(ctx, dx, Z, ldv, k, hs + hl.y, n));
  return 0;
}

// Does alfi_smooth_fgmres(L, k, ...) take the four-launch iteration above?  *flat_spmv: with the flat product and the dots as a
// pass of their own.  (The block smoother, api_block.hip, asks too: such a level takes the block form of that iteration,
// kernels_block_fused.hip, or is smoothed column by column.)
bool smoother_takes_fused_iteration(const alfi_level* L, int k, bool* flat_spmv) {
  // unpartitioned levels with short operator rows: the four-launch iteration (on the small levels a smoother iteration is
  // launch latency, on the large 2-D ones the folded vector passes save BLAS-1 traffic, which is comparable to the patch
  // traffic there): patch_sum_scale_kernel writes z_j and v_j in one pass (the normalisation follows the linear patch
  // solves), the product is the lanes-per-row kernel with the dots folded in.
  // Short rows = the 2-D operators (<= 32 blocks).  With the 50 .. 125 blocks per row of the 3-D ones the flat segmented
  // product of the general path below is the faster kernel (config 3 19.0 against 18.9 ms, config 2 5.10 against 5.43, same
  // box; with the bimodal rows of [P1+FB]^3 the lanes-per-row product idles most lanes: config 6 188.8 ms fused, 175.0
  // general) ... except on levels of <= 50 000 dofs, which are bound by the number of dependent launches whatever the rows
  // look like (config 3 18.66 -> 18.12-18.23 ms).  Sending every level here was measured too: nothing (config 3 17.33 /
  // 17.35 ms, config 4 163.1 / 163.3, config 5 27.24 / 27.10).
  constexpr int64_t small_n = 50000;
  const bool fusable = !alfi_test_large_paths() && !L->distributed && L->n_own == L->n && !L->mult && k + 1 <= 16 &&
                       L->A_own.flat && !L->jacobi;   // (the fused iteration launches the patch kernels itself)
  const bool short_rows = L->max_row_blocks <= 32 || L->n <= small_n;
  if (flat_spmv) *flat_spmv = !short_rows;
  return fusable && short_rows;
}

int alfi_smooth_fgmres(alfi_level* L, int k, const double* db, double* dx, int nonzero_guess) {
  alfi_ctx* ctx = L->ctx;
  if (k < 1) return alfi_set_error(ctx, ALFI_E_ARG, "k must be >= 1");
  if (!level_pc_ready(L)) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_smooth_fgmres before alfi_patches_factor");
  ALFI_CHECK(ensure_fgmres_workspace(L, k));
  ctx->cur_tag = L->id;
  bool flat_spmv = false;
  if (smoother_takes_fused_iteration(L, k, &flat_spmv)) return smooth_fgmres_fused(L, k, db, dx, nonzero_guess, flat_spmv);
  return smooth_fgmres_general(L, L->ws, k, block_chunk(1, nullptr, 0), db, 0, dx, 0, nonzero_guess);
}

namespace {
// A BLAS-1 profiling event that can end and begin again.  It exists for the profile's event counts alone: the one-column call
// has always recorded three events per iteration (dots | projection | Hessenberg column, split where a partitioned level
// all-reduces), a chunk of two or more columns one event per slot and iteration -- and both counts stay what they were.
class Blas1Event {
 public:
  explicit Blas1Event(alfi_ctx* ctx) : ctx_(ctx) { open(); }
  void open() { ev_.emplace(ctx_, ALFI_EV_BLAS1); }
  void close() { ev_.reset(); }

 private:
  alfi_ctx* ctx_;
  std::optional<ProfScope> ev_;
};
}   // namespace

// The general path: right-preconditioned FGMRES(k), classical Gram-Schmidt, explicit norms, for the 1 .. BLOCK_NV columns
// `cols` of B and X with slot s of ws for column cols.c[s].  Per iteration ONE (block) apply and ONE (block) product for all
// slots; the BLAS-1 and Hessenberg launches slot by slot: a slot's chain hands its reduction partials from one launch to the
// next through the ctx's two partial buffers and is finished before the next slot's begins.  A partitioned level comes with
// one column only (check_block_call): its dots and norms are reduced into the ctx's buffer and all-reduced there.
int smooth_fgmres_general(alfi_level* L, const KrylovWs& ws, int k, const BlockCols& cols, const double* B, int64_t ldb, double* X,
                          int64_t ldx, int nonzero_guess) {
  alfi_ctx* ctx = L->ctx;
  const int K = ws.K, nc = cols.n;
  const bool one = nc == 1;
  const int64_t n = L->n_own;    // vector kernels and reductions run on the owned prefix
  const int64_t ldv = ws.ldv;    // stride of the Krylov bases (local length incl. ghost slots, rounded up to even)
  const bool par = L->distributed;
  HsLayout hl(K);
  const BlockCols slots = block_chunk(nc, nullptr, 0);
  auto hdots_of = [&](int s) { return par ? ctx->dred : ws.h(s) + hl.hd; };
  double* nrm2 = par ? ctx->dred + RED_MAXV : nullptr;
  // One column: the BLAS-1 event ends here and the next one begins, and in between a partitioned level all-reduces `count`
  // doubles at `offset` of the ctx's buffer.  Two or more columns: one event per slot and step, nothing to do.
  auto event_ends = [&](Blas1Event& ev, bool reduce, int64_t offset, int64_t count) -> int {
    if (!one) return 0;
    ev.close();
    if (reduce) ALFI_CHECK(comm_allreduce(L, offset, count));
    ev.open();
    return 0;
  };
  // r0 = b - A x (MatMult), beta = |r0|, v0 = r0 / beta
  if (nonzero_guess) {
    ALFI_CHECK(block_spmv(L, cols, slots, X, ldx, ws.w, ldv, B, ldb, 1));
  } else {
    for (int s = 0; s < nc; ++s) {
      ALFI_HIP_CHECK(ctx, hipMemsetAsync(X + cols.c[s] * ldx, 0, sizeof(double) * L->n, ctx->stream));
      ProfScope prof(ctx, ALFI_EV_BLAS1);
      ALFI_CHECK(launch_copy(ctx, ws.wv(s), B + cols.c[s] * ldb, n));
    }
  }
  // reductions: red_blocks_for(n) partials per vector.  Up to 256 of them (levels of <= 1 M dofs, where a smoother
  // iteration is a chain of launches of a few microseconds each) the kernel that needs a reduced value sums the partials
  // itself -- every block in the same fixed order -- instead of waiting for a one-block reduction launch.
  const int G = red_blocks_for(n);
  // (G = n / 4096 partials per vector; a limit of 512 would include config 3's finest level, 319 partials: measured 18.31
  // against 18.13 ms per cycle, the re-summation in every consumer block costs more than the launch)
  const bool fused = !par && G <= 256 && k + 1 <= 16;
  const double* part1 = par ? nrm2 : ctx->red_partial;      // where the consumer of a norm finds it: all-reduced, or nblk partials
  const double* part2 = par ? nrm2 : ctx->red_partial2;
  const int nblk = par ? 1 : G;
  for (int s = 0; s < nc; ++s) {
    Blas1Event ev(ctx);
    ALFI_CHECK(launch_norm_partials(ctx, ws.wv(s), n));
    if (par) ALFI_CHECK(launch_reduce_partials(ctx, ctx->red_partial, G, 1, nrm2));
    ALFI_CHECK(event_ends(ev, par, RED_MAXV, 1));
    ALFI_CHECK(launch_norm_init_finish(ctx, part1, nblk, ws.h(s), K));
    ALFI_CHECK(launch_scale_by_inv(ctx, ws.v(s, 0), ws.wv(s), ws.h(s) + hl.beta, n));
  }
  for (int j = 0; j < k; ++j) {
    if (one) {      // straight to the level: a sum exchange after the patch solves spares the product its forward exchange
      bool zghosts = false;
      ALFI_CHECK(level_patch_apply(L, ws.v(0, j), ws.z(0, j), &zghosts));                            // z_j = M^-1 v_j
      ALFI_CHECK(level_spmv(L, ws.z(0, j), ws.w, nullptr, 0, zghosts));                              // w = A z_j
    } else {
      ALFI_CHECK(block_patch_apply(L, slots, slots, ws.v(0, j), ws.vs(), ws.z(0, j), ws.zs()));
      ALFI_CHECK(block_spmv(L, slots, slots, ws.z(0, j), ws.zs(), ws.w, ldv, nullptr, 0, 0));
    }
    // partitioned: |w|^2 rides along in the same all-reduce; |w - V h|^2 = |w|^2 - |h|^2 then needs no second one
    const bool pyth = par && !ctx->exact_norm;
    for (int s = 0; s < nc; ++s) {
      double *V = ws.v(s, 0), *w = ws.wv(s), *hs = ws.h(s), *hdots = hdots_of(s);
      const double* ww = pyth ? hdots + (j + 1) : nullptr;
      Blas1Event ev(ctx);   // to the end of the loop body
      // h = V^T w (classical GS); fused: the partials stay in red_partial and the projection kernel sums them
      ALFI_CHECK(launch_multi_dot(ctx, V, ldv, j + 1, w, fused ? nullptr : hdots, n));
      if (pyth) {
        ALFI_CHECK(launch_norm_partials(ctx, w, n));
        ALFI_CHECK(launch_reduce_partials(ctx, ctx->red_partial, G, 1, hdots + (j + 1)));
      }
      ALFI_CHECK(event_ends(ev, par, 0, pyth ? j + 2 : j + 1));
      // w -= V h, |w|^2 partials (into the second partial buffer: the dot partials are still being read)
      ALFI_CHECK(launch_multi_axpy_norm(ctx, V, ldv, j + 1, hdots, w, n, ctx->red_partial2, fused ? G : 0));
      if (par && !pyth) ALFI_CHECK(launch_reduce_partials(ctx, ctx->red_partial2, G, 1, nrm2));
      ALFI_CHECK(event_ends(ev, par && !pyth, RED_MAXV, 1));
      if (j + 1 < k)   // Hessenberg column + v_{j+1} = w / |w| in one launch
        ALFI_CHECK(launch_hessenberg_scale(ctx, part2, nblk, hdots, hs, j, K, ws.v(s, j + 1), w, n, ww));
      else
        ALFI_CHECK(launch_hessenberg_update(ctx, part2, nblk, hdots, hs, j, K, ww));
    }
  }
  for (int s = 0; s < nc; ++s) {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_fgmres_finish(ctx, ws.h(s), k, K));
    ALFI_CHECK(launch_update_solution(ctx, X + cols.c[s] * ldx, ws.z(s, 0), ldv, k, ws.h(s) + hl.y, n));
  }
  return 0;
}

// ---- Chebyshev(k) smoother ---------------------------------------------------------------------------------------------------
// (allocates: alfi_mg_set_smoother and the readiness check of a cycle call it, so that no cycle -- captured or not -- has to)
int ensure_cheb_workspace(alfi_level* L) {
  alfi_ctx* ctx = L->ctx;
  if (L->cheb_d) return 0;
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_CHECK(dev_alloc(ctx, &L->cheb_r, L->n));
  ALFI_CHECK(dev_alloc(ctx, &L->cheb_z, L->n));
  ALFI_CHECK(dev_alloc(ctx, &L->cheb_d, L->n));
  return 0;
}

// Saad, Iterative Methods for Sparse Linear Systems, Alg. 12.1 on the preconditioned operator M A with the spectrum assumed in
// [emin, emax]: theta = (emax + emin) / 2, delta = (emax - emin) / 2, sigma_1 = theta / delta, rho_0 = 1 / sigma_1,
//   d_0 = z_0 / theta,   d_i = rho_i rho_{i-1} d_{i-1} + (2 rho_i / delta) z_i,   rho_i = 1 / (2 sigma_1 - rho_{i-1}),
// z_i = M (b - A x_i), x_{i+1} = x_i + d_i: the error after k steps is T_k((theta - M A) / delta) / T_k(theta / delta) e_0.
// One residual, one preconditioner application and one fused update per step; the coefficients are host scalars passed as
// kernel arguments, so there is no reduction and no read-back.
int alfi_smooth_chebyshev(alfi_level* L, int k, double emin, double emax, const double* db, double* dx, int nonzero_guess) {
  if (!L) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL level");
  alfi_ctx* ctx = L->ctx;
  if (level_is_partitioned(L))
    return alfi_set_error(ctx, ALFI_E_ARG, "alfi_smooth_chebyshev on a partitioned level (serial levels only)");
  if (k < 1) return alfi_set_error(ctx, ALFI_E_ARG, "k must be >= 1");
  if (!(emin > 0.0) || !(emax > emin) || !std::isfinite(emax))
    return alfi_set_error(ctx, ALFI_E_ARG, "Chebyshev interval [%g, %g]: need 0 < emin < emax", emin, emax);
  if (!db || !dx || db == dx) return alfi_set_error(ctx, ALFI_E_ARG, "alfi_smooth_chebyshev: b and x must be distinct vectors");
  if (!level_pc_ready(L)) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_smooth_chebyshev before alfi_patches_factor");
  ALFI_CHECK(ensure_cheb_workspace(L));
  ctx->cur_tag = L->id;
  const int64_t n = L->n;
  const double theta = 0.5 * (emax + emin), delta = 0.5 * (emax - emin), sigma1 = theta / delta;
  double rho = 1.0 / sigma1;
  for (int i = 0; i < k; ++i) {
    const bool x_is_zero = i == 0 && !nonzero_guess;
    const double* r = db;                                      // zero iterate: r = b, no product
    if (!x_is_zero) {
      ALFI_CHECK(alfi_residual(L, db, dx, L->cheb_r));         // r = b - A x
      r = L->cheb_r;
    }
    ALFI_CHECK(level_patch_apply(L, r, L->cheb_z));            // z = M r
    double a = 0.0, c = 1.0 / theta;
    if (i > 0) {
      const double rho_new = 1.0 / (2.0 * sigma1 - rho);
      a = rho_new * rho;
      c = 2.0 * rho_new / delta;
      rho = rho_new;
    }
    ProfScope prof(ctx, ALFI_EV_BLAS1);   // to the end of the loop body
    ALFI_CHECK(launch_cheb_update(ctx, L->cheb_d, dx, L->cheb_z, a, c, n, i > 0 ? 0 : (x_is_zero ? 2 : 1)));
  }
  return 0;
}

// m Arnoldi steps on M A from v0 (set-up of the Chebyshev interval, KSPChebyshevEstEigSet): classical Gram-Schmidt with the
// smoother's multi-dot / multi-axpy kernels, the Hessenberg matrix assembled on the device, one synchronisation at the end.
int alfi_level_arnoldi(alfi_level* L, int m, const double* dv0, double* H_host, int* m_done) {
  if (!L) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL level");
  alfi_ctx* ctx = L->ctx;
  if (level_is_partitioned(L))
    return alfi_set_error(ctx, ALFI_E_ARG, "alfi_level_arnoldi on a partitioned level (serial levels only)");
  if (m < 1 || m > 30) return alfi_set_error(ctx, ALFI_E_ARG, "Arnoldi steps %d not in 1..30", m);
  if (!dv0 || !H_host || !m_done) return alfi_set_error(ctx, ALFI_E_ARG, "NULL argument");
  if (!level_pc_ready(L)) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_level_arnoldi before alfi_patches_factor");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->cur_tag = L->id;
  const int64_t n = L->n, ld = krylov_ldv(n);             // 16-byte aligned basis vectors
  const int G = red_blocks_for(n);
  const int ldh = m + 2;                                  // device Hessenberg: column j at Hd + j * ldh, slot m + 1 = |v0|
  double *V = nullptr, *z = nullptr, *w = nullptr, *Hd = nullptr;
  int rc = dev_alloc(ctx, &V, (int64_t)(m + 1) * ld);
  if (rc == 0) rc = dev_alloc(ctx, &z, ld);
  if (rc == 0) rc = dev_alloc(ctx, &w, ld);
  if (rc == 0) rc = dev_alloc(ctx, &Hd, (int64_t)m * ldh);
  if (rc == 0 && hipMemsetAsync(Hd, 0, sizeof(double) * m * ldh, ctx->stream) != hipSuccess) rc = ALFI_E_HIP;
  auto run = [&]() -> int {
    double* beta = Hd + (m + 1);
    {
      ProfScope prof(ctx, ALFI_EV_BLAS1);
      ALFI_CHECK(launch_norm_partials(ctx, dv0, n));
      ALFI_CHECK(launch_reduce_partials(ctx, ctx->red_partial, G, 1, beta));
      ALFI_CHECK(launch_sqrt_inplace(ctx, beta));
      ALFI_CHECK(launch_scale_by_inv(ctx, V, dv0, beta, n));                      // v_0 = v0 / |v0|
    }
    for (int j = 0; j < m; ++j) {
      double* h = Hd + (int64_t)j * ldh;
      ALFI_CHECK(level_spmv(L, V + (int64_t)j * ld, z, nullptr, 0));               // z = A v_j
      ALFI_CHECK(level_patch_apply(L, z, w));                                     // w = M z
      ProfScope prof(ctx, ALFI_EV_BLAS1);   // to the end of the loop body
      ALFI_CHECK(launch_multi_dot(ctx, V, ld, j + 1, w, h, n));                   // h = V^T w
      ALFI_CHECK(launch_multi_axpy_norm(ctx, V, ld, j + 1, h, w, n, ctx->red_partial2, 0));   // w -= V h, |w|^2 partials
      ALFI_CHECK(launch_reduce_partials(ctx, ctx->red_partial2, G, 1, h + j + 1));
      ALFI_CHECK(launch_sqrt_inplace(ctx, h + j + 1));                            // h_{j+1,j} = |w|
      ALFI_CHECK(launch_scale_by_inv(ctx, V + (int64_t)(j + 1) * ld, w, h + j + 1, n));   // (a zero norm gives a zero vector)
    }
    return 0;
  };
  if (rc == 0) rc = run();
  std::vector<double> Hh((size_t)m * ldh, 0.0);
  if (rc == 0 && hipMemcpyAsync(Hh.data(), Hd, sizeof(double) * m * ldh, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    rc = alfi_set_error(ctx, ALFI_E_HIP, "alfi_level_arnoldi: read-back failed");
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == 0) rc = alfi_set_error(ctx, ALFI_E_HIP, "alfi_level_arnoldi: sync failed");
  dev_free(V);
  dev_free(z);
  dev_free(w);
  dev_free(Hd);
  if (rc != 0) return rc;
  // breakdown: the first column whose subdiagonal entry is zero (to rounding, against the column) or not finite ends the basis
  int done = m;
  for (int j = 0; j < m && done == m; ++j) {
    double cn = 0.0;
    for (int i = 0; i <= j; ++i) cn = std::max(cn, std::fabs(Hh[(size_t)j * ldh + i]));
    const double sub = Hh[(size_t)j * ldh + j + 1];
    if (!std::isfinite(sub) || !std::isfinite(cn)) done = j;
    else if (sub <= 1e-14 * cn) done = j + 1;
  }
  for (int i = 0; i <= m; ++i)
    for (int j = 0; j < m; ++j) H_host[(size_t)i * m + j] = (j < done && i <= j + 1) ? Hh[(size_t)j * ldh + i] : 0.0;
  *m_done = done;
  return 0;
}
