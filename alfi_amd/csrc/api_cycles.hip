// C ABI of libalfi_hip.so (include/alfi_hip.h), coarse solve, Schoeberl transfers, PCMG V / W / full cycles, their hipGraph replay,
// and CG preconditioned by one cycle.
// (One file per concern since round 5: api_ctx / api_level / api_patches / api_smoother / api_cycles / api_saddle; the helpers they
// share are declared in api_internal.h.)
#include "api_internal.h"
#include "block_cols.h"

// ---- coarse solve ------------------------------------------------------------------------------------------------------------
int alfi_coarse_set_inverse(alfi_level* L, const double* inv, int inv_is_device) {
  alfi_ctx* ctx = L->ctx;
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (L->cinv_owned) dev_free(L->cinv);
  L->cinv = nullptr;
  L->cinv_owned = false;
  mf_free(L->mf);
  L->mf = nullptr;
  if (inv_is_device) {
    L->cinv = const_cast<double*>(inv);
  } else {
    ALFI_CHECK(dev_upload(ctx, &L->cinv, inv, L->n * L->n));
    L->cinv_owned = true;
  }
  return 0;
}

// +-1 pattern for the residual probe of the coarse inverse
int alfi_coarse_factor(alfi_level* L) {
  alfi_ctx* ctx = L->ctx;
  if (L->has_halo && L->n_own != L->n)
    return alfi_set_error(ctx, ALFI_E_STATE, "alfi_coarse_factor needs a level owned by one rank");
  if (L->n > ((int64_t)1 << 17)) return alfi_set_error(ctx, ALFI_E_ARG, "coarse level of %lld dofs: the dense inverse would "
                                                      "take %.0f GB", (long long)L->n, 8e-9 * (double)L->n * (double)L->n);
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (L->cinv_owned) dev_free(L->cinv);
  L->cinv = nullptr;
  L->cinv_owned = false;
  mf_free(L->mf);
  L->mf = nullptr;
  double* inv = nullptr;
  ALFI_CHECK(dev_alloc(ctx, &inv, L->n * L->n));
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->status, 0, sizeof(int), ctx->stream));
  int rc = launch_coarse_factor(L, inv);
  int st = 0;
  if (rc == 0 && hipMemcpy(&st, L->status, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = ALFI_E_HIP;
  if (rc == 0 && st != 0) rc = alfi_set_error(ctx, ALFI_E_SINGULAR, "zero pivot block while inverting the coarse operator");
  // residual probe: || A (X e) - e ||_inf for a +-1 vector e
  if (rc == 0) {
    double *de = nullptr, *dy = nullptr, *dr = nullptr;
    double worst = 0.0;
    rc = dev_alloc(ctx, &de, L->n);
    if (rc == 0) rc = dev_alloc(ctx, &dy, L->n);
    if (rc == 0) rc = dev_alloc(ctx, &dr, L->n);
    if (rc == 0) rc = launch_probe_fill(ctx, de, L->n);
    if (rc == 0) rc = launch_dense_gemv(ctx, inv, de, dy, L->n);
    if (rc == 0) rc = launch_bsr_spmv(ctx, L->A, dy, dr, nullptr, 1.0, 0);
    if (rc == 0) rc = launch_probe_residual(ctx, dr, L->n, &worst);
    else (void)hipStreamSynchronize(ctx->stream);
    dev_free(de);
    dev_free(dy);
    dev_free(dr);
    if (rc == 0) {
      L->cinv_residual = worst;
      // (cond(A_0) ~ 1e8 at config 4: cond * eps * |X| |A| |e| leaves ~1e-7 even for a perfectly rounded inverse; the
      // residual of a backward-stable factorisation scales with the condition number, so a large one is REPORTED through
      // alfi_coarse_residual and only one beyond alfi_env_coarse_check_fail() -- default 1e-2, or a non-finite one -- fails the setup)
      if (!(worst <= alfi_env_coarse_check_fail()))
        rc = alfi_set_error(ctx, ALFI_E_SINGULAR, "coarse inverse fails the residual probe: || A X e - e || = %.3e", worst);
    }
  }
  if (rc != 0) {
    dev_free(inv);
    return rc;
  }
  L->cinv = inv;
  L->cinv_owned = true;
  return 0;
}

// || A x - e ||_inf for x = solve(e), e a +-1 vector: the residual probe shared by the dense and the sparse coarse solver
static int coarse_probe(alfi_level* L, double* worst_out) {
  alfi_ctx* ctx = L->ctx;
  double *de = nullptr, *dy = nullptr, *dr = nullptr;
  int rc = dev_alloc(ctx, &de, L->n);
  if (rc == 0) rc = dev_alloc(ctx, &dy, L->n);
  if (rc == 0) rc = dev_alloc(ctx, &dr, L->n);
  if (rc == 0) rc = launch_probe_fill(ctx, de, L->n);
  if (rc == 0) rc = L->mf ? mf_solve(L, de, dy) : launch_dense_gemv(ctx, L->cinv, de, dy, L->n);
  if (rc == 0) rc = launch_bsr_spmv(ctx, L->A, dy, dr, nullptr, 1.0, 0);
  if (rc == 0) rc = launch_probe_residual(ctx, dr, L->n, worst_out);
  else (void)hipStreamSynchronize(ctx->stream);
  dev_free(de);
  dev_free(dy);
  dev_free(dr);
  return rc;
}

// Sparse direct factorisation of the level operator (multifrontal, mf_coarse.h) for coarse grids beyond the dense inverse.
// coords: nbrows x dim node coordinates (host) for the geometric nested dissection, or NULL (BFS level sets of the graph).
int alfi_coarse_factor_sparse(alfi_level* L, const double* coords, int dim, int leaf_nodes) {
  alfi_ctx* ctx = L->ctx;
  if (L->has_halo && L->n_own != L->n)
    return alfi_set_error(ctx, ALFI_E_STATE, "alfi_coarse_factor_sparse needs a level owned by one rank");
  if (coords && (dim < 1 || dim > 3)) return alfi_set_error(ctx, ALFI_E_ARG, "node coordinates of dimension %d", dim);
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (L->cinv_owned) dev_free(L->cinv);
  L->cinv = nullptr;
  L->cinv_owned = false;
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->status, 0, sizeof(int), ctx->stream));
  ALFI_CHECK(mf_factor(L, coords, dim, leaf_nodes));
  int st = 0;
  ALFI_HIP_CHECK(ctx, hipMemcpy(&st, L->status, sizeof(int), hipMemcpyDeviceToHost));
  int rc = 0;
  if (st != 0) rc = alfi_set_error(ctx, ALFI_E_SINGULAR, "zero pivot block in a front of the coarse factorisation");
  double worst = 0.0;
  if (rc == 0) rc = coarse_probe(L, &worst);
  if (rc == 0) {
    L->cinv_residual = worst;
    if (!(worst <= alfi_env_coarse_check_fail()))
      rc = alfi_set_error(ctx, ALFI_E_SINGULAR, "sparse coarse factorisation fails the residual probe: || A x - e || = %.3e", worst);
  }
  if (rc != 0) {
    mf_free(L->mf);
    L->mf = nullptr;
  }
  return rc;
}

int alfi_coarse_factor_bytes(alfi_level* L, int64_t* bytes) {
  if (L->mf) *bytes = mf_bytes(L->mf);
  else if (L->cinv) *bytes = L->n * L->n * 8;
  else return alfi_set_error(L->ctx, ALFI_E_STATE, "no coarse factorisation");
  return 0;
}

int alfi_coarse_residual(alfi_level* L, double* worst) {
  if (!L->cinv && !L->mf) return alfi_set_error(L->ctx, ALFI_E_STATE, "no coarse inverse");
  *worst = L->cinv_residual;
  return 0;
}

int alfi_coarse_solve(alfi_level* L, const double* db, double* dx) {
  if (!L->cinv && !L->mf) return alfi_set_error(L->ctx, ALFI_E_STATE, "alfi_coarse_solve before alfi_coarse_set_inverse");
  L->ctx->cur_tag = L->id;
  ProfScope prof(L->ctx, ALFI_EV_COARSE);   // to the end of the function
  if (L->mf) ALFI_CHECK(mf_solve(L, db, dx));
  else ALFI_CHECK(launch_dense_gemv(L->ctx, L->cinv, db, dx, L->n));
  return 0;
}

// ---- transfer ------------------------------------------------------------------------------------------------------------------
int alfi_transfer_create(alfi_ctx* ctx, alfi_level* coarse, alfi_level* fine, const alfi_bsr_host* P,
                         const alfi_bsr_host* PT, const alfi_bsr_host* PT_plain, const alfi_bsr_host* D_I,
                         const alfi_bsr_host* D_IT, int64_t nblk, int m, const int32_t* blk_dofs, const double* K_II,
                         const double* D_II, alfi_transfer** out) {
  if (!ctx || !coarse || !fine || !P || !PT || !D_I || !D_IT || !blk_dofs || !K_II || !D_II || !out)
    return alfi_set_error(ctx, ALFI_E_ARG, "NULL argument");
  const int bs = fine->bs;
  if (coarse->bs != bs) return alfi_set_error(ctx, ALFI_E_ARG, "block size mismatch");
  if (m < 1 || m > PATCH_MAX)
    return alfi_set_error(ctx, ALFI_E_ARG, "interior block size %d not in 1..%d", m, PATCH_MAX);
  // partitioned fine level: P and D_I^T hold the owned fine rows, P^T the owned fine columns (its rows are partial sums
  // over the local coarse numbering, reverse-added to their owners); serial: n_own == n
  if (P->nbrows * bs != fine->n_own || P->nbcols * bs != coarse->n || PT->nbrows * bs != coarse->n ||
      (PT->nbcols * bs != fine->n_own && PT->nbcols * bs != fine->n))
    return alfi_set_error(ctx, ALFI_E_ARG, "prolongation shape does not match the levels");
  if ((nblk * m) % bs != 0 || D_I->nbrows * bs != nblk * m || D_I->nbcols * bs != fine->n ||
      D_IT->nbrows * bs != fine->n_own || D_IT->nbcols * bs != nblk * m)
    return alfi_set_error(ctx, ALFI_E_ARG, "grad-div interior rows shape mismatch");
  if (fine->distributed && !coarse->has_halo)
    return alfi_set_error(ctx, ALFI_E_STATE, "coarse level of a partitioned transfer needs alfi_level_set_partition");
  for (int64_t i = 0; i < nblk * m; ++i)
    if (blk_dofs[i] < 0 || blk_dofs[i] >= fine->n) return alfi_set_error(ctx, ALFI_E_ARG, "blk_dofs out of range");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  alfi_transfer* T = new alfi_transfer();
  T->ctx = ctx;
  T->coarse = coarse;
  T->fine = fine;
  T->bs = bs;
  T->nblk = nblk;
  T->m = m;
  T->ld = (m + 1) & ~1;
  int rc = upload_bsr(ctx, &T->P, P, bs);
  if (rc == 0) rc = upload_bsr(ctx, &T->PT, PT, bs);
  if (rc == 0) {
    if (PT_plain) {
      rc = upload_bsr(ctx, &T->PTp, PT_plain, bs);
    } else {
      T->PTp = T->PT;
      T->ptp_alias = true;
    }
  }
  if (rc == 0) rc = upload_bsr(ctx, &T->DI, D_I, bs);
  if (rc == 0) rc = upload_bsr(ctx, &T->DIT, D_IT, bs);
  if (rc == 0) rc = dev_upload(ctx, &T->blk_dofs, blk_dofs, nblk * m);
  if (rc == 0) rc = dev_upload(ctx, &T->KII, K_II, nblk * m * m);
  if (rc == 0) rc = dev_upload(ctx, &T->DII, D_II, nblk * m * m);
  if (m > 32) {
    // macro-cell blocks (Scott-Vogelius transfer, transfer.py:49-88): inverses in the row-piece layout, solved with the
    // patch smoother's kernels; compact vectors keep stride m, the kernels write row pairs with stride ld (for odd m the
    // result passes through pm_tmp)
    T->patch_mode = true;
    T->bstride = ((int64_t)m * T->ld + 15) & ~(int64_t)15;
    std::vector<int64_t> ptr(nblk + 1), iptr(nblk + 1), sptr(nblk + 1);
    std::vector<int32_t> iota((size_t)nblk * m);
    for (int64_t b = 0; b <= nblk; ++b) {
      ptr[b] = b * m;
      iptr[b] = b * T->bstride;
      sptr[b] = b * T->ld;
    }
    for (int64_t i = 0; i < nblk * m; ++i) iota[i] = (int32_t)i;
    if (rc == 0) rc = dev_upload(ctx, &T->pm_ptr, ptr.data(), nblk + 1);
    if (rc == 0) rc = dev_upload(ctx, &T->pm_inv_ptr, iptr.data(), nblk + 1);
    if (rc == 0) rc = dev_upload(ctx, &T->pm_stage_ptr, sptr.data(), nblk + 1);
    if (rc == 0) rc = dev_upload(ctx, &T->pm_iota, iota.data(), nblk * m);
    if (rc == 0) rc = dev_alloc(ctx, &T->binv, nblk * T->bstride);
    if (rc == 0 && T->ld != m) rc = dev_alloc(ctx, &T->pm_tmp, nblk * T->ld);
    if (rc == 0) rc = dev_alloc(ctx, &T->pm_res, nblk * m);       // one step of iterative refinement per interior solve
    if (rc == 0) rc = dev_alloc(ctx, &T->pm_cor, nblk * m);
    if (rc == 0) rc = dev_alloc(ctx, &T->AIIt, nblk * m * T->ld);
  } else if (rc == 0) {
    rc = dev_alloc(ctx, &T->binv, nblk * m * T->ld);
  }
  if (rc == 0) rc = dev_alloc(ctx, &T->tI, nblk * m);
  if (rc == 0) rc = dev_alloc(ctx, &T->bI, nblk * m);
  if (rc == 0) rc = dev_alloc(ctx, &T->tmp_f, fine->n);
  if (rc == 0) rc = dev_alloc(ctx, &T->status, 1);
  if (rc != 0) {
    alfi_transfer_destroy(T);
    return rc;
  }
  *out = T;
  return 0;
}

int alfi_transfer_destroy(alfi_transfer* T) {
  if (!T) return 0;
  (void)hipStreamSynchronize(T->ctx->stream);
  free_bsr(&T->P);
  free_bsr(&T->PT);
  if (!T->ptp_alias) free_bsr(&T->PTp);
  free_bsr(&T->DI);
  free_bsr(&T->DIT);
  dev_free(T->blk_dofs);
  dev_free(T->KII);
  dev_free(T->DII);
  dev_free(T->binv);
  dev_free(T->pm_ptr);
  dev_free(T->pm_inv_ptr);
  dev_free(T->pm_stage_ptr);
  dev_free(T->pm_iota);
  dev_free(T->pm_tmp);
  dev_free(T->pm_res);
  dev_free(T->pm_cor);
  dev_free(T->AIIt);
  dev_free(T->tI);
  dev_free(T->bI);
  dev_free(T->tmp_f);
  dev_free(T->inj);
  if (T->injm) {
    free_csr(T->injm);
    delete T->injm;
  }
  dev_free(T->status);
  delete T;
  return 0;
}

int alfi_transfer_set_injection(alfi_transfer* T, const int32_t* fine_node) {
  alfi_ctx* ctx = T->ctx;
  if (!fine_node) return alfi_set_error(ctx, ALFI_E_ARG, "NULL injection map");
  if (T->fine->has_halo || T->coarse->has_halo)
    return alfi_set_error(ctx, ALFI_E_ARG, "alfi_inject is not available on partitioned levels");
  const int64_t nc = T->coarse->n / T->bs, nf = T->fine->n / T->bs;
  for (int64_t i = 0; i < nc; ++i)
    if (fine_node[i] < 0 || fine_node[i] >= nf) return alfi_set_error(ctx, ALFI_E_ARG, "injection map entry out of range");
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  dev_free(T->inj);
  T->inj = nullptr;
  return dev_upload(ctx, &T->inj, fine_node, nc);
}

int alfi_transfer_set_injection_matrix(alfi_transfer* T, const alfi_csr_host* J) {
  alfi_ctx* ctx = T->ctx;
  if (!J) return alfi_set_error(ctx, ALFI_E_ARG, "NULL injection matrix");
  if (T->fine->has_halo || T->coarse->has_halo)
    return alfi_set_error(ctx, ALFI_E_ARG, "alfi_inject is not available on partitioned levels");
  const int64_t nc = T->coarse->n / T->bs, nf = T->fine->n / T->bs;
  if (J->nrows != nc || J->ncols != nf)
    return alfi_set_error(ctx, ALFI_E_ARG, "injection matrix must be %lld x %lld (coarse nodes x fine nodes)", (long long)nc, (long long)nf);
  for (int64_t i = 0; i < nc; ++i)
    if (J->rowptr[i + 1] < J->rowptr[i]) return alfi_set_error(ctx, ALFI_E_ARG, "row pointer not monotone");
  for (int64_t k = 0; k < J->rowptr[nc]; ++k)
    if (J->colidx[k] < 0 || J->colidx[k] >= nf) return alfi_set_error(ctx, ALFI_E_ARG, "injection matrix column out of range");
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (T->injm) {
    free_csr(T->injm);
    delete T->injm;
    T->injm = nullptr;
  }
  DevCSR* M = new DevCSR();
  const int rc = upload_csr(ctx, M, J);
  if (rc != 0) {
    free_csr(M);
    delete M;
    return rc;
  }
  T->injm = M;
  return 0;
}

int alfi_inject(alfi_transfer* T, const double* dxf, double* dxc) {
  if (T->injm) return launch_inject_csr(T->ctx, *T->injm, T->bs, dxf, dxc);
  if (!T->inj) return alfi_set_error(T->ctx, ALFI_E_STATE, "alfi_inject before alfi_transfer_set_injection");
  return launch_halo_pack(T->ctx, dxc, dxf, T->inj, T->coarse->n / T->bs, T->bs);   // coarse[i] = fine[inj[i]]
}

int alfi_transfer_update(alfi_transfer* T, double nu, double gamma) {
  alfi_ctx* ctx = T->ctx;
  T->nu = nu;
  T->gamma = gamma;
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(T->status, 0, sizeof(int), ctx->stream));
  ALFI_CHECK(launch_block_build_invert(T));
  int st = 0;
  ALFI_HIP_CHECK(ctx, hipMemcpyAsync(&st, T->status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (st != 0) return alfi_set_error(ctx, ALFI_E_SINGULAR, "zero pivot while inverting a coarse-cell interior block");
  T->ready = true;
  return 0;
}

int alfi_transfer_get_block_inverse(alfi_transfer* T, int64_t blk, double* out) {
  alfi_ctx* ctx = T->ctx;
  if (!T->ready) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_transfer_get_block_inverse before alfi_transfer_update");
  if (blk < 0 || blk >= T->nblk) return alfi_set_error(ctx, ALFI_E_ARG, "block index out of range");
  const int m = T->m, ld = T->ld;
  const int64_t stride = T->patch_mode ? T->bstride : (int64_t)m * ld;
  std::vector<double> tmp((size_t)m * ld);
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ALFI_HIP_CHECK(ctx, hipMemcpy(tmp.data(), T->binv + blk * stride, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j)
      out[(int64_t)i * m + j] = T->patch_mode ? tmp[patch_inv_index(i, j, m, ld)] : tmp[(int64_t)j * ld + i];
  return 0;
}

int alfi_prolong(alfi_transfer* T, const double* dxc, double* dxf) {
  alfi_ctx* ctx = T->ctx;
  if (!T->ready) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_prolong before alfi_transfer_update");
  ctx->cur_tag = T->fine->id;
  // partitioned fine level: coarse ghosts in, rhs on the owned fine rows, fine ghosts in; the interior solves of every
  // coarse cell touching an owned node run locally (redundantly at partition boundaries), writes to ghost slots are scratch
  const bool par = T->fine->distributed;
  if (par) ALFI_CHECK(halo_fwd(T->coarse, const_cast<double*>(dxc)));
  {
    ProfScope prof(ctx, ALFI_EV_PROLONG);
    ALFI_CHECK(launch_bsr_spmv(ctx, T->P, dxc, dxf, nullptr, 0.0, 0));               // rhs = P coarse        :247
  }
  if (par) ALFI_CHECK(halo_fwd(T->fine, dxf));
  ProfScope prof(ctx, ALFI_EV_PROLONG);   // to the end of the function
  ALFI_CHECK(launch_bsr_spmv(ctx, T->DI, dxf, T->bI, nullptr, 0.0, 0));              // b_I = (D rhs)_I       :249
  ALFI_CHECK(launch_block_gemv(T, T->bI, T->tI, false));                              // t = inv(A_II) b_I     :254-257
  ALFI_CHECK(launch_scatter_sub(ctx, dxf, T->blk_dofs, T->tI, T->gamma, T->nblk * T->m));  // fine = rhs - gamma t  :259
  ALFI_CHECK(launch_zero_dofs(ctx, dxf, T->fine->bc_dofs, T->fine->nbc));
  return 0;
}

int alfi_restrict(alfi_transfer* T, const double* drf, double* drc, int robust) {
  alfi_ctx* ctx = T->ctx;
  if (robust && !T->ready) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_restrict before alfi_transfer_update");
  ctx->cur_tag = T->fine->id;
  const bool par = T->fine->distributed;
  if (par && robust) ALFI_CHECK(halo_fwd(T->fine, const_cast<double*>(drf)));
  if (robust) {
    ProfScope prof(ctx, ALFI_EV_RESTRICT);
    ALFI_CHECK(launch_block_gemv(T, drf, T->tI, true));                               // t = inv(A_II) r_I     :265-270
    ALFI_CHECK(launch_bsr_spmv(ctx, T->DIT, T->tI, T->tmp_f, drf, T->gamma, 1));      // s = r - gamma D t     :272-274
    ALFI_CHECK(launch_bsr_spmv(ctx, T->PT, T->tmp_f, drc, nullptr, 0.0, 0));          // coarse = P^T s        :275
  } else {
    ProfScope prof(ctx, ALFI_EV_RESTRICT);
    ALFI_CHECK(launch_bsr_spmv(ctx, T->PTp, drf, drc, nullptr, 0.0, 0));              // firedrake.restrict
  }
  if (par) ALFI_CHECK(halo_rev(T->coarse, drc));   // partial sums over the owned fine nodes -> the coarse owners
  ProfScope prof(ctx, ALFI_EV_RESTRICT);   // to the end of the function
  ALFI_CHECK(launch_zero_dofs(ctx, drc, T->coarse->bc_dofs, T->coarse->nbc));
  return 0;
}

// ---- multigrid --------------------------------------------------------------------------------------------------------------------
int alfi_mg_create(alfi_ctx* ctx, int nlevels, alfi_level** levels, alfi_transfer** transfers, int k,
                   int robust_restriction, alfi_mg** out) {
  if (!ctx || nlevels < 1 || !levels || (nlevels > 1 && !transfers) || !out)
    return alfi_set_error(ctx, ALFI_E_ARG, "bad arguments");
  for (int l = 1; l < nlevels; ++l) {
    if (transfers[l - 1]->coarse != levels[l - 1] || transfers[l - 1]->fine != levels[l])
      return alfi_set_error(ctx, ALFI_E_ARG, "transfer %d does not link levels %d and %d", l - 1, l - 1, l);
  }
  // (patch factors and the coarse inverse are asked for when a cycle runs -- mg_ready -- not here: a hierarchy whose operators
  // are formed on the device is linked before its first refresh)
  alfi_mg* mg = new alfi_mg();
  mg->ctx = ctx;
  mg->levels.assign(levels, levels + nlevels);
  if (nlevels > 1) mg->transfers.assign(transfers, transfers + nlevels - 1);
  mg->k = k;
  mg->robust = robust_restriction;
  for (int l = 0; l < nlevels; ++l) {
    alfi_level* L = levels[l];
    int rc = 0;
    if (!L->mg_b) rc = dev_alloc(ctx, &L->mg_b, L->n);
    if (rc == 0 && !L->mg_x) rc = dev_alloc(ctx, &L->mg_x, L->n);
    if (rc == 0 && !L->mg_r) rc = dev_alloc(ctx, &L->mg_r, L->n);
    if (rc == 0 && l > 0 && L->n_own > 0) rc = ensure_fgmres_workspace(L, k);
    if (rc != 0) {
      delete mg;
      return rc;
    }
  }
  *out = mg;
  return 0;
}

int alfi_mg_destroy(alfi_mg* mg) {
  if (!mg) return 0;
  (void)hipStreamSynchronize(mg->ctx->stream);
  for (CycleGraph& g : mg->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  dev_free(mg->cg_r);
  dev_free(mg->cg_z);
  dev_free(mg->cg_p);
  dev_free(mg->cg_w);
  dev_free(mg->cg_s);
  delete mg;
  return 0;
}

// serial hierarchies only: what the Chebyshev smoother, the W-cycle and CG ask of every level
static int mg_require_serial(alfi_mg* mg, const char* what) {
  for (alfi_level* L : mg->levels)
    if (level_is_partitioned(L)) return alfi_set_error(mg->ctx, ALFI_E_ARG, "%s on a partitioned hierarchy (serial levels only)", what);
  return 0;
}

int alfi_mg_set_smoother(alfi_mg* mg, int type, const double* emin, const double* emax) {
  if (!mg) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL multigrid");
  alfi_ctx* ctx = mg->ctx;
  if (type != ALFI_SMOOTHER_FGMRES && type != ALFI_SMOOTHER_CHEBYSHEV)
    return alfi_set_error(ctx, ALFI_E_ARG, "smoother type %d (0 FGMRES, 1 Chebyshev)", type);
  if (type == ALFI_SMOOTHER_FGMRES) {
    mg->smoother = type;
    return 0;
  }
  ALFI_CHECK(mg_require_serial(mg, "alfi_mg_set_smoother(Chebyshev)"));
  const int nl = (int)mg->levels.size();
  if (nl > 1 && (!emin || !emax)) return alfi_set_error(ctx, ALFI_E_ARG, "Chebyshev smoother without intervals");
  for (int l = 1; l < nl; ++l)
    if (!(emin[l - 1] > 0.0) || !(emax[l - 1] > emin[l - 1]) || !std::isfinite(emax[l - 1]))
      return alfi_set_error(ctx, ALFI_E_ARG, "Chebyshev interval [%g, %g] of level %d: need 0 < emin < emax", emin[l - 1],
                            emax[l - 1], l);
  // the smoother's work vectors now, not in the first cycle: with graphs on that cycle may already be a capture
  for (int l = 1; l < nl; ++l) ALFI_CHECK(ensure_cheb_workspace(mg->levels[l]));
  mg->emin.assign((size_t)nl, 0.0);
  mg->emax.assign((size_t)nl, 0.0);
  for (int l = 1; l < nl; ++l) {
    mg->emin[l] = emin[l - 1];
    mg->emax[l] = emax[l - 1];
  }
  mg->smoother = type;
  return 0;
}

int alfi_mg_set_cycles(alfi_mg* mg, int cycles) {
  if (!mg) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL multigrid");
  if (cycles != 1 && cycles != 2) return alfi_set_error(mg->ctx, ALFI_E_ARG, "cycles %d (1 V, 2 W)", cycles);
  if (cycles > 1) ALFI_CHECK(mg_require_serial(mg, "alfi_mg_set_cycles(W)"));
  mg->cycles = cycles;
  return 0;
}

// ---- the cycles, for the 1 .. BLOCK_NV columns `cols` of B and X -------------------------------------------------------------------
// The single calls (alfi_mg_vcycle / _fcycle) are the one-column case.  The smoother and the residual are the block forms of
// api_block.hip, which are the single-vector code on one column; transfers, the coarse solve and the correction loop over the
// columns with the single-vector code.  Below the level a cycle starts on, column i of the chunk lives in column i of the levels'
// work vectors (b, x, r of leading dimension ld): own_work -- the level's mg_b / mg_x / mg_r, one column, whose addresses a
// captured single cycle holds -- or block_work, the slots of blk_mg_b / _x / _r (mg_block_vectors).
struct MgWork {
  double *b, *x, *r;
  int64_t ld;
};
typedef MgWork (*MgWorkOf)(const alfi_level*);
static MgWork own_work(const alfi_level* L) { return {L->mg_b, L->mg_x, L->mg_r, 0}; }
static MgWork block_work(const alfi_level* L) { return {L->blk_mg_b.p, L->blk_mg_x.p, L->blk_mg_r.p, L->blk_mg_b.per}; }

// the level smoother of the hierarchy (alfi_mg_set_smoother)
static int mg_smooth(alfi_mg* mg, int l, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx,
                     int nonzero_guess) {
  alfi_level* L = mg->levels[l];
  if (mg->smoother == ALFI_SMOOTHER_CHEBYSHEV) {
    for (int i = 0; i < cols.n; ++i)
      ALFI_CHECK(alfi_smooth_chebyshev(L, mg->k, mg->emin[l], mg->emax[l], B + cols.c[i] * ldb, X + cols.c[i] * ldx, nonzero_guess));
    return 0;
  }
  return block_smooth_fgmres(L, mg->k, cols, B, ldb, X, ldx, nonzero_guess);
}

// PCMGMCycle_Private [3P]: x_l <- M(b_l, x_l), the V-cycle for cycles = 1 and the W-cycle for cycles = 2: level 1 visits the
// coarse solve once, every level >= 2 recurses `cycles` times on the same restricted right-hand side, the later visits
// continuing from the coarse iterate of the one before.  x_zero: the incoming x is known to be zero (every level below the one the
// cycle starts on): the pre-smoother then runs with a zero initial guess -- r0 = b, no residual SpMV -- as PCMG does by
// switching KSPSetInitialGuessNonzero off for the down-smoother of those levels; the result is the same bit for bit.
static int vcycle(alfi_mg* mg, MgWorkOf work, int l, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx,
                  bool x_zero) {
  alfi_ctx* ctx = mg->ctx;
  alfi_level* L = mg->levels[l];
  const int nc = cols.n;
  if (l == 0) {
    // partitioned hierarchies: a rank's lowest level is either the coarse grid it owns or ghost copies of a level another
    // rank owns and solves (then there is nothing to do here); every level above is owned in part by every rank
    for (int i = 0; i < nc && L->n_own > 0; ++i) ALFI_CHECK(alfi_coarse_solve(L, B + cols.c[i] * ldb, X + cols.c[i] * ldx));
    return 0;
  }
  alfi_transfer* T = mg->transfers[l - 1];
  const BlockCols slots = block_chunk(nc, nullptr, 0);
  const MgWork wl = work(L), wc = work(mg->levels[l - 1]);
  ALFI_CHECK(mg_smooth(mg, l, cols, B, ldb, X, ldx, x_zero ? 0 : 1));                                // pre-smooth
  ALFI_CHECK(block_spmv(L, cols, slots, X, ldx, wl.r, wl.ld, B, ldb, 1));                           // r = b - A x
  for (int i = 0; i < nc; ++i) ALFI_CHECK(alfi_restrict(T, wl.r + i * wl.ld, wc.b + i * wc.ld, mg->robust));   // b_{l-1} = R r
  // x_{l-1} = 0: the coarse solve overwrites it, a smoother with a zero initial guess zeroes it itself
  const int cycles = l == 1 ? 1 : mg->cycles;
  for (int c = 0; c < cycles; ++c) ALFI_CHECK(vcycle(mg, work, l - 1, slots, wc.b, wc.ld, wc.x, wc.ld, c == 0));
  for (int i = 0; i < nc; ++i) ALFI_CHECK(alfi_prolong(T, wc.x + i * wc.ld, wl.r + i * wl.ld));
  ctx->cur_tag = L->id;
  for (int i = 0; i < nc; ++i) {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_axpy(ctx, X + cols.c[i] * ldx, wl.r + i * wl.ld, 1.0, L->n_own));              // x += P x_{l-1}
  }
  return mg_smooth(mg, l, cols, B, ldb, X, ldx, 1);                                                 // post-smooth
}

// PCMGFCycle_Private [3P]
static int fcycle(alfi_mg* mg, MgWorkOf work, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx) {
  const int Lmax = (int)mg->levels.size() - 1, nc = cols.n;
  if (Lmax == 0) return vcycle(mg, work, 0, cols, B, ldb, X, ldx, false);
  const BlockCols slots = block_chunk(nc, nullptr, 0);
  for (int i = 0; i < nc; ++i) {         // restrict the right-hand sides through all levels
    const double* bf = B + cols.c[i] * ldb;
    for (int l = Lmax; l >= 1; --l) {
      const MgWork wc = work(mg->levels[l - 1]);
      ALFI_CHECK(alfi_restrict(mg->transfers[l - 1], bf, wc.b + i * wc.ld, mg->robust));
      bf = wc.b + i * wc.ld;
    }
  }
  for (int l = 0; l < Lmax; ++l) {
    // inside vcycle(l) the coarser levels' b and x are overwritten; level l's own b survives: vcycle(l) only writes b of
    // levels < l.  The restricted right-hand sides of levels < l are gone then, and no longer needed (increasing order).
    const MgWork wl = work(mg->levels[l]), wn = work(mg->levels[l + 1]);
    ALFI_CHECK(vcycle(mg, work, l, slots, wl.b, wl.ld, wl.x, wl.ld, l == 0));    // l >= 1: x_l is the prolonged coarser solution
    for (int i = 0; i < nc; ++i)
      ALFI_CHECK(alfi_prolong(mg->transfers[l], wl.x + i * wl.ld, l + 1 == Lmax ? X + cols.c[i] * ldx : wn.x + i * wn.ld));
  }
  return vcycle(mg, work, Lmax, cols, B, ldb, X, ldx, false);
}

// ---- whole cycles as hipGraphs (alfi_ctx_set_graph) -----------------------------------------------------------------------
// A cycle on the small levels of a hierarchy is a few hundred short kernels whose launch cost exceeds their run time
// (ldc2d at 1.2 M dofs: 6 ms per V-cycle against 1.8 ms of HBM time; multiplicative sweeps launch one kernel per
// wavefront of patches).  With graphs on, the second call of a cycle with the same (b, x) pair captures its launch
// sequence from the library's stream and every later call replays it; the first call runs eagerly (it may still allocate
// the smoother's workspace).  Anything a captured argument depends on is part of the entry's signature, so new operator
// values in place are picked up for free and new (nu, gamma), patches or a new coarse inverse re-capture.  Profiling
// events and the exchange callbacks of partitioned levels cannot be captured: those runs stay eager.
static void cycle_signature(alfi_mg* mg, std::vector<uint64_t>* sig) {
  auto push = [&](const void* q) { sig->push_back((uint64_t)(uintptr_t)q); };
  auto pushd = [&](double v) {
    uint64_t u;
    memcpy(&u, &v, sizeof(u));
    sig->push_back(u);
  };
  sig->clear();
  sig->push_back((uint64_t)mg->k);
  sig->push_back((uint64_t)mg->robust);
  sig->push_back((uint64_t)mg->smoother);
  sig->push_back((uint64_t)mg->cycles);
  if (mg->smoother == ALFI_SMOOTHER_CHEBYSHEV)       // the interval becomes kernel arguments
    for (size_t l = 1; l < mg->levels.size(); ++l) {
      pushd(mg->emin[l]);
      pushd(mg->emax[l]);
    }
  for (alfi_level* L : mg->levels) {
    sig->push_back((uint64_t)(L->jacobi ? 1 : 0));
    push(L->jac_diag);
    push(L->cheb_d);
    push(L->A.vals);
    push(L->inv);
    push(L->inv32);
    sig->push_back((uint64_t)(L->held == HELD_F32 ? 1 : 0));
    push(L->cd.mat);
    push(L->cd.sinv);
    push(L->patch_ptr);
    push(L->patch_dofs);
    push(L->cinv);
    push(L->mf);
    push(L->ws.V);
    push(L->mult_seq);
    push(L->mcw_gchunk);
    push(L->mcw_schunk);
    push(L->mcw_node);
    push(L->mcw_r);
    sig->push_back((uint64_t)L->npatch);
    sig->push_back((uint64_t)L->ws.K);
    sig->push_back((uint64_t)(L->mult ? 1 + (L->mult_symmetrise ? 1 : 0) + 4 * L->sweep.wave_ptr.size() : 0));
  }
  for (alfi_transfer* T : mg->transfers) {
    push(T->binv);
    pushd(T->nu);
    pushd(T->gamma);
  }
}

// every level has what a cycle multiplies with: factored patches, a coarse inverse
static int mg_ready(alfi_mg* mg) {
  alfi_ctx* ctx = mg->ctx;
  for (size_t l = 1; l < mg->levels.size(); ++l) {
    alfi_level* L = mg->levels[l];
    if (L->n_own > 0 && !level_pc_ready(L))
      return alfi_set_error(ctx, ALFI_E_STATE, "level %d: patches not factored", (int)l);
    if (mg->smoother == ALFI_SMOOTHER_CHEBYSHEV) ALFI_CHECK(ensure_cheb_workspace(L));   // (a no-op after alfi_mg_set_smoother)
    // a point-Jacobi level: the diagonal of the current operator values, extracted here and not inside the cycle, so that a
    // captured cycle never holds the extraction and never multiplies with a stale diagonal
    if (L->jacobi && L->jac_version != L->op_version) {
      ALFI_CHECK(launch_jacobi_diag(ctx, L->A, L->jac_diag));
      L->jac_version = L->op_version;
    }
  }
  // a rank that only holds ghost copies of its lowest level (the owner solves it) needs no coarse inverse
  alfi_level* C = mg->levels[0];
  if (C->n_own > 0 && !C->cinv && !C->mf) return alfi_set_error(ctx, ALFI_E_STATE, "coarse level has no inverse");
  return 0;
}

static int run_cycle(alfi_mg* mg, int kind, const double* db, double* dx) {
  alfi_ctx* ctx = mg->ctx;
  ALFI_CHECK(mg_ready(mg));
  const BlockCols one = block_chunk(1, nullptr, 0);      // the vector pair as a one-column operand
  auto eager = [&]() {
    return kind ? fcycle(mg, own_work, one, db, 0, dx, 0) : vcycle(mg, own_work, (int)mg->levels.size() - 1, one, db, 0, dx, 0, false);
  };
  bool ok = ctx->use_graph && ctx->prof == 0;
  for (alfi_level* L : mg->levels) ok = ok && !L->has_halo;
  if (!ok) return eager();
  std::vector<uint64_t> sig;
  cycle_signature(mg, &sig);
  CycleGraph* G = nullptr;
  for (CycleGraph& g : mg->graphs)
    if (g.kind == kind && g.b == db && g.x == dx) G = &g;
  if (!G) {                       // first call with this pair: eager, remember it
    if (mg->graphs.size() >= 16) {
      for (CycleGraph& g : mg->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
      mg->graphs.clear();
    }
    CycleGraph g;
    g.kind = kind;
    g.b = db;
    g.x = dx;
    mg->graphs.push_back(g);
    return eager();
  }
  if (G->failed) return eager();
  if (G->exec && G->sig != sig) {
    (void)hipGraphExecDestroy(G->exec);
    G->exec = nullptr;
  }
  if (!G->exec) {
    // the workspace may have changed between the eager call and now: compare after a possible eager warm-up
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError();
      G->failed = true;
      return eager();
    }
    const int rc = eager();
    const hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
    if (rc != 0 || e != hipSuccess || !graph) {
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      G->failed = true;
      return rc != 0 ? rc : eager();
    }
    const hipError_t ei = hipGraphInstantiate(&G->exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
      (void)hipGetLastError();
      G->exec = nullptr;
      G->failed = true;
      return eager();
    }
    cycle_signature(mg, &G->sig);
  }
  ALFI_HIP_CHECK(ctx, hipGraphLaunch(G->exec, ctx->stream));
  return 0;
}

int alfi_mg_vcycle(alfi_mg* mg, const double* db, double* dx) { return run_cycle(mg, 0, db, dx); }

int alfi_mg_fcycle(alfi_mg* mg, const double* db, double* dx) { return run_cycle(mg, 1, db, dx); }

// ---- block cycles (alfi_mg_vcycle_block / _fcycle_block) ---------------------------------------------------------------------------
// The cycles above on the block work vectors, chunk after chunk, eagerly (never a captured graph).
static int mg_block_vectors(alfi_mg* mg, int ncol) {
  for (alfi_level* L : mg->levels)
    for (SlotBuf* v : {&L->blk_mg_b, &L->blk_mg_x, &L->blk_mg_r}) ALFI_CHECK(slot_buf_ensure(mg->ctx, v, ncol, krylov_ldv(L->n)));
  return 0;
}

// one full cycle on the 1 .. BLOCK_NV columns `cols` of B and X, arguments unchecked (alfi_saddle_precond_block)
int mg_fcycle_block_chunk(alfi_mg* mg, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx) {
  ALFI_CHECK(mg_ready(mg));
  ALFI_CHECK(mg_block_vectors(mg, cols.n));
  return fcycle(mg, block_work, cols, B, ldb, X, ldx);
}

static int run_cycle_block(alfi_mg* mg, int kind, const char* what, int ncol, const int* cols, int nx, const double* B, int64_t ldb,
                           double* X, int64_t ldx) {
  if (!mg) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL multigrid");
  ALFI_CHECK(mg_require_serial(mg, what));
  const BlockOperand ops[2] = {{B, ldb, false}, {X, ldx, true}};
  ALFI_CHECK(check_block_call(mg->levels.back(), what, ncol, cols, nx, ops, 2));
  ALFI_CHECK(mg_ready(mg));
  ALFI_CHECK(mg_block_vectors(mg, ncol));
  for (int q = 0; q < block_chunks(ncol); ++q) {
    const BlockCols c = block_chunk(ncol, cols, q);
    ALFI_CHECK(kind ? fcycle(mg, block_work, c, B, ldb, X, ldx)
                    : vcycle(mg, block_work, (int)mg->levels.size() - 1, c, B, ldb, X, ldx, false));
  }
  return 0;
}

int alfi_mg_vcycle_block(alfi_mg* mg, int ncol, const int* cols, int nx, const double* B, int64_t ldb, double* X, int64_t ldx) {
  return run_cycle_block(mg, 0, "alfi_mg_vcycle_block", ncol, cols, nx, B, ldb, X, ldx);
}
int alfi_mg_fcycle_block(alfi_mg* mg, int ncol, const int* cols, int nx, const double* B, int64_t ldb, double* X, int64_t ldx) {
  return run_cycle_block(mg, 1, "alfi_mg_fcycle_block", ncol, cols, nx, B, ldb, X, ldx);
}

// KSPCG [3P] with a zero initial guess and the unpreconditioned residual norm, preconditioned by one cycle of mg
// (examples/graddiv/graddiv.py:85-95).  The step lengths are formed on the device from reduced scalars (kernels_cheb.hip);
// the one read-back per iteration is |r|^2 for the convergence test, taken before the cycle so that no cycle is wasted.
int alfi_mg_cg(alfi_mg* mg, const double* db, double* dx, double rtol, double atol, int max_it, int full, int* its,
               double* rnorm) {
  if (!mg) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL multigrid");
  alfi_ctx* ctx = mg->ctx;
  ALFI_CHECK(mg_require_serial(mg, "alfi_mg_cg"));
  if (!db || !dx || db == dx || !its || !rnorm || max_it < 0 || !(rtol >= 0.0) || !(atol >= 0.0))
    return alfi_set_error(ctx, ALFI_E_ARG, "alfi_mg_cg: bad arguments");
  alfi_level* L = mg->levels.back();
  const int64_t n = L->n;
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!mg->cg_s) {
    ALFI_CHECK(dev_alloc(ctx, &mg->cg_r, n));
    ALFI_CHECK(dev_alloc(ctx, &mg->cg_z, n));
    ALFI_CHECK(dev_alloc(ctx, &mg->cg_p, n));
    ALFI_CHECK(dev_alloc(ctx, &mg->cg_w, n));
    ALFI_CHECK(dev_alloc(ctx, &mg->cg_s, 4));
  }
  double *r = mg->cg_r, *z = mg->cg_z, *p = mg->cg_p, *w = mg->cg_w, *s = mg->cg_s;
  auto precond = [&]() -> int {     // z = PCMG(r)
    if (full) return run_cycle(mg, 1, r, z);
    ALFI_HIP_CHECK(ctx, hipMemsetAsync(z, 0, sizeof(double) * n, ctx->stream));
    return run_cycle(mg, 0, r, z);
  };
  auto dot = [&](const double* a, const double* b, double* out) -> int {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    return launch_multi_dot(ctx, a, 0, 1, b, out, n);
  };
  auto read_rr = [&](double* rr) -> int {
    ALFI_HIP_CHECK(ctx, hipMemcpyAsync(rr, s + 3, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return check_dev_err(ctx);
  };
  ctx->cur_tag = L->id;
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(dx, 0, sizeof(double) * n, ctx->stream));
  {
    ProfScope prof(ctx, ALFI_EV_BLAS1);
    ALFI_CHECK(launch_copy(ctx, r, db, n));                    // x = 0: r = b
  }
  ALFI_CHECK(dot(r, r, s + 3));
  double rr = 0.0;
  ALFI_CHECK(read_rr(&rr));
  const double tol = std::max(rtol * std::sqrt(rr), atol);
  int it = 0;
  while (std::sqrt(rr) > tol && it < max_it && std::isfinite(rr)) {
    const int cur = it & 1;
    ALFI_CHECK(precond());
    ctx->cur_tag = L->id;
    ALFI_CHECK(dot(r, z, s + cur));                            // r . z of this iteration
    {
      ProfScope prof(ctx, ALFI_EV_BLAS1);
      ALFI_CHECK(launch_cg_update_p(ctx, p, z, s, cur, it == 0 ? 1 : 0, n));   // p = z + (r.z / r.z of the last iteration) p
    }
    ALFI_CHECK(level_spmv(L, p, w, nullptr, 0));               // w = A p
    ALFI_CHECK(dot(p, w, s + 2));
    {
      ProfScope prof(ctx, ALFI_EV_BLAS1);
      ALFI_CHECK(launch_cg_update_xr(ctx, dx, r, p, w, s, cur, n));                // x += alpha p, r -= alpha w
    }
    ALFI_CHECK(dot(r, r, s + 3));
    ++it;
    ALFI_CHECK(read_rr(&rr));
  }
  *its = it;
  *rnorm = std::sqrt(rr);
  return 0;
}

int alfi_ctx_comm_stats(alfi_ctx* ctx, int64_t* halo_exchanges, int64_t* allreduces, int64_t* doubles_sent, int reset) {
  if (halo_exchanges) *halo_exchanges = ctx->comm_nhalo;
  if (allreduces) *allreduces = ctx->comm_nred;
  if (doubles_sent) *doubles_sent = ctx->comm_sent;
  if (reset) ctx->comm_nhalo = ctx->comm_nred = ctx->comm_sent = 0;
  return 0;
}

int alfi_ctx_set_graph(alfi_ctx* ctx, int on) {
  ctx->use_graph = on != 0;
  return 0;
}
