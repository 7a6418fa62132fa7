// C ABI of libalfi_hip.so (include/alfi_hip.h), the outer saddle-point solve and the vector operations of the Newton loop around the path.
// (One file per concern since round 5: api_ctx / api_level / api_patches / api_smoother / api_cycles / api_saddle; the helpers they
// share are declared in api_internal.h.)
#include "api_internal.h"
#include "block_cols.h"

// ---- outer saddle-point solve (alfi/solver.py:386-422) ----------------------------------------------------------------------------
int upload_csr(alfi_ctx* ctx, DevCSR* d, const alfi_csr_host* h) {
  d->nrows = h->nrows;
  d->ncols = h->ncols;
  d->nnz = h->rowptr[h->nrows];
  ALFI_CHECK(dev_upload(ctx, &d->rowptr, h->rowptr, h->nrows + 1));
  ALFI_CHECK(dev_upload(ctx, &d->colidx, h->colidx, d->nnz));
  ALFI_CHECK(dev_upload(ctx, &d->vals, h->vals, d->nnz));
  return 0;
}
void free_csr(DevCSR* d) {
  dev_free(d->rowptr);
  dev_free(d->colidx);
  dev_free(d->vals);
  *d = DevCSR();
}

// ---- building blocks of the outer solve on partitioned levels (alfi_amd/dist.py: DistSaddle drives them from the host) -------
int alfi_level_halo_forward(alfi_level* L, double* dv) {
  if (!L->distributed) return 0;
  L->ctx->cur_tag = L->id;
  return halo_fwd(L, dv);
}

int alfi_level_halo_reverse_add(alfi_level* L, double* dv) {
  if (!L->distributed) return 0;
  L->ctx->cur_tag = L->id;
  return halo_rev(L, dv);
}

// ---- small vector operations for the Newton loop around the path: state, update and residual stay in HBM (the reference's
// NonlinearVariationalSolver keeps z as a Function, alfi/solver.py:245-273); only scalars come back ------------------------------
int alfi_transfer_stats(int64_t* h2d_bytes, int64_t* d2h_bytes, int reset) {
  if (h2d_bytes) *h2d_bytes = g_alfi_h2d_bytes.load();
  if (d2h_bytes) *d2h_bytes = g_alfi_d2h_bytes.load();
  if (reset) {
    g_alfi_h2d_bytes = 0;
    g_alfi_d2h_bytes = 0;
  }
  return 0;
}

int alfi_vec_axpy(alfi_ctx* ctx, double* dy, const double* dx, double a, int64_t n) {
  if (n < 0 || (n > 0 && (!dy || !dx))) return alfi_set_error(ctx, ALFI_E_ARG, "bad vector arguments");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return n == 0 ? 0 : launch_axpy(ctx, dy, dx, a, n);
}

int alfi_vec_copy(alfi_ctx* ctx, double* dy, const double* dx, int64_t n) {
  if (n < 0 || (n > 0 && (!dy || !dx))) return alfi_set_error(ctx, ALFI_E_ARG, "bad vector arguments");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return n == 0 ? 0 : launch_copy(ctx, dy, dx, n);
}

// dst[i] = src[idx[i]] (bs consecutive doubles per index): a level's state from a vector that holds the values it needs
int alfi_vec_gather(alfi_ctx* ctx, double* dst, const double* src, const int32_t* d_idx, int64_t nidx, int bs) {
  if (nidx < 0 || bs < 1 || (nidx > 0 && (!dst || !src || !d_idx))) return alfi_set_error(ctx, ALFI_E_ARG, "bad gather arguments");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return nidx == 0 ? 0 : launch_halo_pack(ctx, dst, src, d_idx, nidx, bs);
}

// dst[i*bs + c] = sum over k in [rowptr[i], rowptr[i+1]) of weights[k] * src[colidx[k]*bs + c]: a level's state on a non-nested
// hierarchy, where a node of the level is a point evaluation of the finest field (bs 1, 2 or 3: the velocity blocks)
int alfi_vec_gather_csr(alfi_ctx* ctx, double* dst, const double* src, const int32_t* d_rowptr, const int32_t* d_colidx,
                        const double* d_weights, int64_t nrows, int bs) {
  if (nrows < 0 || bs < 1 || bs > 3 || (nrows > 0 && (!dst || !src || !d_rowptr || !d_colidx || !d_weights)))
    return alfi_set_error(ctx, ALFI_E_ARG, "bad weighted gather arguments");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return nrows == 0 ? 0 : launch_gather_csr(ctx, dst, src, d_rowptr, d_colidx, d_weights, nrows, bs);
}

// dv[Dirichlet dofs of the level] = 0 (bc.zero(F), alfi/solver.py:282-286)
int alfi_level_zero_bc(alfi_level* L, double* dv) {
  alfi_ctx* ctx = L->ctx;
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return L->nbc == 0 ? 0 : launch_zero_dofs(ctx, dv, L->bc_dofs, L->nbc);
}

// x . y of two vectors of the outer solve, (velocity | pressure) -- on a partitioned finest level the owned entries, summed over
// the ranks: every rank gets the same value.  Fixed summation order (two-stage reduction).
int alfi_saddle_dot(alfi_saddle* S, const double* dx, const double* dy, double* out_host) {
  alfi_ctx* ctx = S->ctx;
  if (!dx || !dy || !out_host) return alfi_set_error(ctx, ALFI_E_ARG, "NULL argument");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t n = S->nu_dofs + S->np_dofs;
  if (!S->dotbuf) ALFI_CHECK(dev_alloc(ctx, &S->dotbuf, 2));
  double* out = S->par ? ctx->dred : S->dotbuf;
  ALFI_CHECK(launch_multi_dot(ctx, dx, n, 1, dy, out, n));
  if (S->par) {
    ctx->cur_tag = S->fine->id;
    ALFI_CHECK(comm_allreduce(S->fine, 0, 1));
  }
  ALFI_HIP_CHECK(ctx, hipMemcpyAsync(out_host, out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return check_dev_err(ctx);
}

// the merged exchange of the smoother (alfi_level_set_sum_exchange): every holder of a shared node ends with the sum of all
// holders' values
int alfi_level_halo_sum(alfi_level* L, double* dv) {
  if (!L->distributed) return 0;
  if (!L->sum_ready) return alfi_set_error(L->ctx, ALFI_E_STATE, "alfi_level_halo_sum before alfi_level_set_sum_exchange");
  L->ctx->cur_tag = L->id;
  return halo_sum(L, dv);
}

struct alfi_csr {
  alfi_ctx* ctx = nullptr;
  DevCSR M;
};

int alfi_csr_create(alfi_ctx* ctx, const alfi_csr_host* h, alfi_csr** out) {
  if (!ctx || !h || !out) return alfi_set_error(ctx, ALFI_E_ARG, "NULL argument");
  for (int64_t i = 0; i < h->nrows; ++i)
    if (h->rowptr[i + 1] < h->rowptr[i]) return alfi_set_error(ctx, ALFI_E_ARG, "row pointer not monotone");
  const int64_t nnz = h->rowptr[h->nrows];
  for (int64_t k = 0; k < nnz; ++k)
    if (h->colidx[k] < 0 || h->colidx[k] >= h->ncols) return alfi_set_error(ctx, ALFI_E_ARG, "column index out of range");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  alfi_csr* C = new alfi_csr();
  C->ctx = ctx;
  int rc = upload_csr(ctx, &C->M, h);
  if (rc != 0) {
    free_csr(&C->M);
    delete C;
    return rc;
  }
  *out = C;
  return 0;
}

int alfi_csr_destroy(alfi_csr* C) {
  if (!C) return 0;
  (void)hipStreamSynchronize(C->ctx->stream);
  free_csr(&C->M);
  delete C;
  return 0;
}

// mode 0: y = M x;  1: y = b - alpha M x;  2: y += M x;  3: y = alpha M x
int alfi_csr_mult(alfi_csr* C, const double* dx, double* dy, const double* db, double alpha, int mode) {
  if (mode < 0 || mode > 3 || (mode == 1 && !db)) return alfi_set_error(C->ctx, ALFI_E_ARG, "bad mode / missing b");
  return launch_csr_spmv(C->ctx, C->M, dx, dy, db, alpha, mode);
}

// On a PARTITIONED finest level (alfi_level_set_partition, distributed) the call is collective and the matrices are the rank's
// pieces: B = the rank's pressure rows over all LOCAL velocity dofs (owned + ghost: n_loc columns), BT = its transpose (n_loc
// rows; the ghost rows hold contributions for their owners, reverse-added).  Vectors then hold (owned velocity dofs | owned
// pressure dofs) and every reduction is one all-reduce -- the same Krylov loop as on one GPU, no host arithmetic.
int alfi_saddle_create(alfi_mg* mg, const alfi_csr_host* B, const alfi_csr_host* BT, const double* mass_diag,
                       double nu, double gamma, int remove_constant_nullspace, alfi_saddle** out) {
  if (!mg || !B || !BT || !mass_diag || !out) return alfi_set_error(mg ? mg->ctx : nullptr, ALFI_E_ARG, "NULL argument");
  alfi_ctx* ctx = mg->ctx;
  alfi_level* F = mg->levels.back();
  const bool par = F->distributed;
  if (F->has_halo && !par)
    return alfi_set_error(ctx, ALFI_E_ARG, "the finest level has a halo but is not distributed: no outer solve on it");
  if (B->ncols != F->n || BT->nrows != F->n || BT->ncols != B->nrows)
    return alfi_set_error(ctx, ALFI_E_ARG, "divergence matrix shape does not match the finest level");
  for (int64_t i = 0; i < B->nrows; ++i)
    if (!(mass_diag[i] > 0.0)) return alfi_set_error(ctx, ALFI_E_ARG, "pressure mass matrix entry %lld is not positive", (long long)i);
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  alfi_saddle* S = new alfi_saddle();
  S->ctx = ctx;
  S->mg = mg;
  S->fine = F;
  S->par = par;
  S->n_loc = F->n;
  S->nu_dofs = par ? F->n_own : F->n;
  S->np_dofs = B->nrows;
  S->np_global = (double)B->nrows;
  S->nu = nu;
  S->gamma = gamma;
  S->remove_nullspace = remove_constant_nullspace != 0;
  std::vector<double> minv(std::max<int64_t>(B->nrows, 1), 1.0);
  for (int64_t i = 0; i < B->nrows; ++i) minv[i] = 1.0 / mass_diag[i];
  int rc = upload_csr(ctx, &S->B, B);
  if (rc == 0) rc = upload_csr(ctx, &S->BT, BT);
  if (rc == 0) rc = dev_upload(ctx, &S->minv, minv.data(), (int64_t)minv.size());
  if (rc == 0) rc = dev_alloc(ctx, &S->tmp_u, S->n_loc);
  if (rc == 0) rc = dev_alloc(ctx, &S->tmp_p, std::max<int64_t>(S->np_dofs, 1));
  if (rc == 0 && par) {
    rc = dev_alloc(ctx, &S->wa, S->n_loc);
    if (rc == 0) rc = dev_alloc(ctx, &S->wb, S->n_loc);
    if (rc == 0) rc = dev_alloc(ctx, &S->wc, S->n_loc);
    if (rc == 0 && hipMemsetAsync(S->wa, 0, sizeof(double) * S->n_loc, ctx->stream) != hipSuccess) rc = ALFI_E_HIP;
    // pressure dofs of all ranks: one all-reduce at setup
    if (rc == 0) {
      const double mine = (double)B->nrows;
      if (hipMemcpyAsync(ctx->dred + RED_MAXV, &mine, sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
          hipStreamSynchronize(ctx->stream) != hipSuccess)
        rc = alfi_set_error(ctx, ALFI_E_HIP, "alfi_saddle_create: copy to the reduction buffer failed");
    }
    if (rc == 0) {
      ctx->cur_tag = F->id;
      rc = comm_allreduce(F, RED_MAXV, 1);
    }
    if (rc == 0) {
      double tot = 0.0;
      if (hipMemcpyAsync(&tot, ctx->dred + RED_MAXV, sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
          hipStreamSynchronize(ctx->stream) != hipSuccess)
        rc = alfi_set_error(ctx, ALFI_E_HIP, "alfi_saddle_create: copy from the reduction buffer failed");
      S->np_global = tot;
    }
  }
  if (rc != 0) {
    alfi_saddle_destroy(S);
    return rc;
  }
  *out = S;
  return 0;
}

int alfi_saddle_destroy(alfi_saddle* S) {
  if (!S) return 0;
  (void)hipStreamSynchronize(S->ctx->stream);
  free_csr(&S->B);
  free_csr(&S->BT);
  if (S->has_Minv) free_csr(&S->Minv);
  dev_free(S->minv);
  release_workspaces(S);      // Krylov workspaces, block buffers
  dev_free(S->tmp_u);
  dev_free(S->tmp_p);
  dev_free(S->wa);
  dev_free(S->wb);
  dev_free(S->wc);
  dev_free(S->dotbuf);
  mf_free(S->vmf);
  delete S;
  return 0;
}

int alfi_saddle_update(alfi_saddle* S, double nu, double gamma) {
  S->nu = nu;
  S->gamma = gamma;
  return 0;
}

// y = [A B^T; B 0] x
int alfi_saddle_mult(alfi_saddle* S, const double* dx, double* dy) {
  alfi_ctx* ctx = S->ctx;
  const int64_t nu = S->nu_dofs;
  if (S->par) {
    alfi_level* F = S->fine;
    ctx->cur_tag = F->id;
    ALFI_CHECK(launch_copy(ctx, S->wa, dx, nu));
    ALFI_CHECK(level_spmv(F, S->wa, S->wb, nullptr, 0));                          // ghosts of wa filled; owned rows of A
    ALFI_CHECK(launch_csr_spmv(ctx, S->B, S->wa, dy + nu, nullptr, 0.0, 0));      // y_p = B u (needs the ghosts)
    ALFI_CHECK(launch_csr_spmv(ctx, S->BT, dx + nu, S->wc, nullptr, 0.0, 0));     // partial B^T p on all local dofs
    ALFI_CHECK(halo_rev(F, S->wc));                                               // ... summed onto their owners
    return launch_add(ctx, dy, S->wb, S->wc, nu);
  }
  ALFI_CHECK(alfi_spmv(S->fine, dx, dy));                                       // y_u = A x_u
  ALFI_CHECK(launch_csr_spmv(ctx, S->BT, dx + nu, dy, nullptr, 0.0, 2));        // y_u += B^T x_p
  ALFI_CHECK(launch_csr_spmv(ctx, S->B, dx, dy + nu, nullptr, 0.0, 0));         // y_p = B x_u
  return 0;
}

// PCFIELDSPLIT, Schur, full factorisation [3P] with the sub-solvers of solver.py:359-391
int alfi_saddle_set_mass_inverse(alfi_saddle* S, const alfi_csr_host* Minv) {
  alfi_ctx* ctx = S->ctx;
  if (!Minv || Minv->nrows != S->np_dofs || Minv->ncols != S->np_dofs)
    return alfi_set_error(ctx, ALFI_E_ARG, "mass inverse must be %lld x %lld", (long long)S->np_dofs, (long long)S->np_dofs);
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (S->has_Minv) free_csr(&S->Minv);
  S->has_Minv = false;
  ALFI_CHECK(upload_csr(ctx, &S->Minv, Minv));
  S->has_Minv = true;
  return 0;
}

// y_p = -(nu + gamma) M^-1 q
static int saddle_schur(alfi_saddle* S, const double* q, double* yp) {
  if (S->has_Minv) return launch_csr_spmv(S->ctx, S->Minv, q, yp, nullptr, -(S->nu + S->gamma), 3);
  return launch_scale_rows(S->ctx, yp, q, S->minv, -(S->nu + S->gamma), S->np_dofs);
}

// ---- fieldsplit_0 as an exact solve (solver_type allu, alfi/solver.py:346-352): multifrontal factors of the finest operator ----
int alfi_saddle_set_velocity_solver(alfi_saddle* S, int kind) {
  if (!S) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL saddle");
  alfi_ctx* ctx = S->ctx;
  if (kind != ALFI_VELOCITY_MG && kind != ALFI_VELOCITY_DIRECT)
    return alfi_set_error(ctx, ALFI_E_ARG, "velocity solver kind %d (ALFI_VELOCITY_MG or ALFI_VELOCITY_DIRECT)", kind);
  alfi_level* F = S->fine;
  if (kind == ALFI_VELOCITY_DIRECT && (S->par || F->has_halo || F->n_own != F->n))
    return alfi_set_error(ctx, ALFI_E_STATE, "the direct velocity solve needs a finest level owned by one rank");
  if (kind == ALFI_VELOCITY_MG && S->vmf) {      // the factors are released with the mode
    ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    mf_free(S->vmf);
    S->vmf = nullptr;
    S->vmf_residual = -1.0;
  }
  S->vkind = kind;
  return 0;
}

// numeric factorisation of the finest operator's current values (the plan of the first call is kept while the sparsity and
// the ordering request stay the same), then the residual probe || A x - e ||_inf, x = solve(e), of alfi_coarse_factor_sparse
int alfi_saddle_factor_velocity(alfi_saddle* S, const double* node_coords, int dim, int leaf_nodes, int64_t max_bytes) {
  if (!S) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL saddle");
  alfi_ctx* ctx = S->ctx;
  alfi_level* F = S->fine;
  if (S->vkind != ALFI_VELOCITY_DIRECT)
    return alfi_set_error(ctx, ALFI_E_STATE, "alfi_saddle_factor_velocity before alfi_saddle_set_velocity_solver(DIRECT)");
  if (node_coords && (dim < 1 || dim > 3)) return alfi_set_error(ctx, ALFI_E_ARG, "node coordinates of dimension %d", dim);
  if (max_bytes < 0) return alfi_set_error(ctx, ALFI_E_ARG, "negative memory cap");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  S->vmf_residual = -1.0;
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(F->status, 0, sizeof(int), ctx->stream));
  ALFI_CHECK(mf_factor_slot(F, &S->vmf, node_coords, dim, leaf_nodes, max_bytes));
  int st = 0;
  int rc = hipMemcpy(&st, F->status, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess ? 0 : ALFI_E_HIP;
  if (rc == 0 && st != 0) rc = alfi_set_error(ctx, ALFI_E_SINGULAR, "zero pivot block in a front of the direct velocity factorisation");
  double worst = 0.0;
  if (rc == 0) {
    double *de = nullptr, *dy = nullptr, *dr = nullptr;
    rc = dev_alloc(ctx, &de, F->n);
    if (rc == 0) rc = dev_alloc(ctx, &dy, F->n);
    if (rc == 0) rc = dev_alloc(ctx, &dr, F->n);
    if (rc == 0) rc = launch_probe_fill(ctx, de, F->n);
    if (rc == 0) rc = mf_solve_slot(F, S->vmf, de, dy);
    if (rc == 0) rc = launch_bsr_spmv(ctx, F->A, dy, dr, nullptr, 1.0, 0);
    if (rc == 0) rc = launch_probe_residual(ctx, dr, F->n, &worst);
    else (void)hipStreamSynchronize(ctx->stream);
    dev_free(de);
    dev_free(dy);
    dev_free(dr);
  }
  if (rc == 0 && !(worst <= alfi_env_coarse_check_fail()))
    rc = alfi_set_error(ctx, ALFI_E_SINGULAR, "direct velocity factorisation fails the residual probe: || A x - e || = %.3e", worst);
  if (rc != 0) {
    mf_free(S->vmf);
    S->vmf = nullptr;
    return rc;
  }
  S->vmf_residual = worst;
  S->vmf_version = F->op_version;
  return 0;
}

// factors present and computed from the finest operator's current values
static int velocity_ready(alfi_saddle* S) {
  if (!S->vmf) return alfi_set_error(S->ctx, ALFI_E_STATE, "direct velocity solve before alfi_saddle_factor_velocity");
  if (S->vmf_version != S->fine->op_version)
    return alfi_set_error(S->ctx, ALFI_E_STATE, "direct velocity solve with factors of an earlier operator (the finest operator "
                                                "changed since alfi_saddle_factor_velocity)");
  return 0;
}

int alfi_saddle_velocity_solve(alfi_saddle* S, const double* db, double* dx) {
  if (!S || !db || !dx || db == dx) return alfi_set_error(S ? S->ctx : nullptr, ALFI_E_ARG, "bad arguments");
  if (S->vkind != ALFI_VELOCITY_DIRECT) return alfi_set_error(S->ctx, ALFI_E_STATE, "the velocity solver is not DIRECT");
  ALFI_CHECK(velocity_ready(S));
  return mf_solve_slot(S->fine, S->vmf, db, dx);
}

int alfi_saddle_velocity_info(alfi_saddle* S, int64_t* bytes, double* probe_residual) {
  if (!S) return alfi_set_error(nullptr, ALFI_E_ARG, "NULL saddle");
  if (!S->vmf) return alfi_set_error(S->ctx, ALFI_E_STATE, "no direct velocity factorisation");
  if (bytes) *bytes = mf_bytes(S->vmf);
  if (probe_residual) *probe_residual = S->vmf_residual;
  return 0;
}

int alfi_saddle_precond(alfi_saddle* S, const double* dx, double* dy) {
  alfi_ctx* ctx = S->ctx;
  const int64_t nu = S->nu_dofs, np = S->np_dofs;
  if (S->vkind == ALFI_VELOCITY_DIRECT) {                                        // (never partitioned: refused when set)
    alfi_level* F = S->fine;
    ALFI_CHECK(velocity_ready(S));
    ALFI_CHECK(mf_solve_slot(F, S->vmf, dx, dy));                               // y_u = A^-1 b_u
    ALFI_CHECK(launch_csr_spmv(ctx, S->B, dy, S->tmp_p, dx + nu, 1.0, 1));      // q = b_p - B y_u
    ALFI_CHECK(saddle_schur(S, S->tmp_p, dy + nu));                             // y_p = -(nu+gamma) M^-1 q
    ALFI_CHECK(launch_csr_spmv(ctx, S->BT, dy + nu, S->tmp_u, dx, 1.0, 1));     // t = b_u - B^T y_p
    ALFI_CHECK(mf_solve_slot(F, S->vmf, S->tmp_u, dy));                         // y_u = A^-1 t
    if (S->remove_nullspace) ALFI_CHECK(launch_remove_mean(ctx, dy + nu, np));
    return 0;
  }
  if (S->par) {
    alfi_level* F = S->fine;
    ALFI_CHECK(launch_copy(ctx, S->wa, dx, nu));
    ALFI_CHECK(alfi_mg_fcycle(S->mg, S->wa, S->wb));                              // y_u = MG(b_u)
    ctx->cur_tag = F->id;
    ALFI_CHECK(halo_fwd(F, S->wb));
    ALFI_CHECK(launch_csr_spmv(ctx, S->B, S->wb, S->tmp_p, dx + nu, 1.0, 1));     // q = b_p - B y_u
    ALFI_CHECK(saddle_schur(S, S->tmp_p, dy + nu));
    ALFI_CHECK(launch_csr_spmv(ctx, S->BT, dy + nu, S->wc, nullptr, 0.0, 0));     // B^T y_p: partial sums on all local dofs
    ALFI_CHECK(halo_rev(F, S->wc));
    ALFI_CHECK(launch_xmy(ctx, S->wc, dx, nu));                                   // t = b_u - B^T y_p
    ALFI_CHECK(alfi_mg_fcycle(S->mg, S->wc, S->wb));                              // y_u = MG(t)
    ALFI_CHECK(launch_copy(ctx, dy, S->wb, nu));
    if (S->remove_nullspace) {                                                    // y_p -= (sum over all ranks) / (all pressure dofs)
      ctx->cur_tag = F->id;
      ALFI_CHECK(launch_sum_to(ctx, dy + nu, np, ctx->dred + RED_MAXV));
      ALFI_CHECK(comm_allreduce(F, RED_MAXV, 1));
      ALFI_CHECK(launch_sub_scaled(ctx, dy + nu, np, ctx->dred + RED_MAXV, 1.0 / S->np_global));
    }
    return 0;
  }
  ALFI_CHECK(alfi_mg_fcycle(S->mg, dx, dy));                                    // y_u = MG(b_u)
  ALFI_CHECK(launch_csr_spmv(ctx, S->B, dy, S->tmp_p, dx + nu, 1.0, 1));        // q = b_p - B y_u
  ALFI_CHECK(saddle_schur(S, S->tmp_p, dy + nu));                               // y_p = -(nu+gamma) M^-1 q
  ALFI_CHECK(launch_csr_spmv(ctx, S->BT, dy + nu, S->tmp_u, dx, 1.0, 1));       // t = b_u - B^T y_p
  ALFI_CHECK(alfi_mg_fcycle(S->mg, S->tmp_u, dy));                              // y_u = MG(t)
  if (S->remove_nullspace) ALFI_CHECK(launch_remove_mean(ctx, dy + nu, np));
  return 0;
}

// ---- block right-hand sides -----------------------------------------------------------------------------------------------------
// alfi_saddle_mult / _precond / _solve for the columns of column-major operands (block_cols.h), columns of n_u + n_p entries.
// Column c of every result is the single call on column c bit for bit: the velocity-block product and the full cycles are the
// block forms of api_block.hip / api_cycles.hip (one launch for up to four columns where the finest level batches), everything
// else -- the divergence and gradient products, the Schur solve, the mean removal, the BLAS-1 and Hessenberg launches of the
// outer FGMRES, the exact velocity solve -- is the single call's launch, column after column.  Serial saddles only.
static int saddle_block_check(alfi_saddle* S, const char* what, int ncol, const int* cols, int nx, const BlockOperand* ops, int nops) {
  if (!S) return alfi_set_error(nullptr, ALFI_E_ARG, "%s: NULL saddle", what);
  if (S->par || level_is_partitioned(S->fine))
    return alfi_set_error(S->ctx, ALFI_E_ARG, "%s on a partitioned finest level (serial levels only)", what);
  return check_block_operands(S->ctx, what, S->nu_dofs + S->np_dofs, ncol, cols, nx, ops, nops);
}

static int saddle_mult_chunk(alfi_saddle* S, const BlockCols& c, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  alfi_ctx* ctx = S->ctx;
  const int64_t nu = S->nu_dofs;
  if (c.n == 1) return alfi_saddle_mult(S, X + c.c[0] * ldx, Y + c.c[0] * ldy);            // (on a partitioned level too)
  ALFI_CHECK(block_spmv(S->fine, c, c, X, ldx, Y, ldy, nullptr, 0, 0));                    // y_u = A x_u
  for (int i = 0; i < c.n; ++i) {
    const double* x = X + c.c[i] * ldx;
    double* y = Y + c.c[i] * ldy;
    ALFI_CHECK(launch_csr_spmv(ctx, S->BT, x + nu, y, nullptr, 0.0, 2));                   // y_u += B^T x_p
    ALFI_CHECK(launch_csr_spmv(ctx, S->B, x, y + nu, nullptr, 0.0, 0));                    // y_p = B x_u
  }
  return 0;
}

// nx: the columns the operands have (the velocity work columns are indexed like them)
static int saddle_precond_chunk(alfi_saddle* S, const BlockCols& c, int nx, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  alfi_ctx* ctx = S->ctx;
  const int64_t nu = S->nu_dofs, np = S->np_dofs, ldu = krylov_ldv(nu);
  if (S->vkind == ALFI_VELOCITY_DIRECT || c.n == 1) {
    for (int i = 0; i < c.n; ++i) ALFI_CHECK(alfi_saddle_precond(S, X + c.c[i] * ldx, Y + c.c[i] * ldy));
    return 0;
  }
  if (S->blk_tmp_u.slots < nx) ALFI_CHECK(slot_buf_resize(ctx, &S->blk_tmp_u, nx, ldu));      // (by operand columns, not by chunk)
  ALFI_CHECK(mg_fcycle_block_chunk(S->mg, c, X, ldx, Y, ldy));                              // y_u = MG(b_u)
  for (int i = 0; i < c.n; ++i) {
    const double* x = X + c.c[i] * ldx;
    double* y = Y + c.c[i] * ldy;
    ALFI_CHECK(launch_csr_spmv(ctx, S->B, y, S->tmp_p, x + nu, 1.0, 1));                   // q = b_p - B y_u
    ALFI_CHECK(saddle_schur(S, S->tmp_p, y + nu));                                         // y_p = -(nu+gamma) M^-1 q
    ALFI_CHECK(launch_csr_spmv(ctx, S->BT, y + nu, S->blk_tmp_u.slot(c.c[i]), x, 1.0, 1));   // t = b_u - B^T y_p
  }
  ALFI_CHECK(mg_fcycle_block_chunk(S->mg, c, S->blk_tmp_u.p, ldu, Y, ldy));                   // y_u = MG(t)
  if (S->remove_nullspace)
    for (int i = 0; i < c.n; ++i) ALFI_CHECK(launch_remove_mean(ctx, Y + c.c[i] * ldy + nu, np));
  return 0;
}

int alfi_saddle_mult_block(alfi_saddle* S, int ncol, const int* cols, int nx, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  const BlockOperand ops[2] = {{X, ldx, false}, {Y, ldy, true}};
  ALFI_CHECK(saddle_block_check(S, "alfi_saddle_mult_block", ncol, cols, nx, ops, 2));
  for (int q = 0; q < block_chunks(ncol); ++q) ALFI_CHECK(saddle_mult_chunk(S, block_chunk(ncol, cols, q), X, ldx, Y, ldy));
  return 0;
}

int alfi_saddle_precond_block(alfi_saddle* S, int ncol, const int* cols, int nx, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  const BlockOperand ops[2] = {{X, ldx, false}, {Y, ldy, true}};
  ALFI_CHECK(saddle_block_check(S, "alfi_saddle_precond_block", ncol, cols, nx, ops, 2));
  for (int q = 0; q < block_chunks(ncol); ++q) ALFI_CHECK(saddle_precond_chunk(S, block_chunk(ncol, cols, q), nx, X, ldx, Y, ldy));
  return 0;
}

// Restarted FGMRES (zero initial guess) on the 1 .. BLOCK_NV columns c of B and X in lockstep; slot s of ws belongs to column
// c.c[s].  alfi_saddle_solve is the one-column case on the saddle's own workspace.  The columns start together, so every active
// column is at the same inner iteration j and the same count `its`; a column leaves the active list when its own test
// max(rtol |b_c|, atol) is met -- inside a cycle (finish and update at its own j) or at a restart's true residual.  its_out[s],
// rn_out[s]: iterations and final true residual norm per slot.  A partitioned saddle comes with one column only
// (saddle_block_check): dots and norms are reduced into the ctx's reduction buffer and all-reduced there, as in the level
// smoother; the values every rank reads back are identical, so all ranks take the same branches.
static int saddle_solve_chunk(alfi_saddle* S, const KrylovWs& ws, const BlockCols& c, const double* B, int64_t ldb, double* X,
                              int64_t ldx, double rtol, double atol, int max_it, int* its_out, double* rn_out) {
  alfi_ctx* ctx = S->ctx;
  alfi_level* F = S->fine;
  const bool par = S->par;
  const int64_t n = S->nu_dofs + S->np_dofs, ldv = ws.ldv;
  const int K = ws.K, nc = c.n;
  HsLayout hl(K);
  const int G = red_blocks_for(n);
  double* nrm2 = par ? ctx->dred + RED_MAXV : nullptr;
  const double* normpart = par ? nrm2 : ctx->red_partial2;      // |w - V h|^2: all-reduced, or nblk partials
  const int nblk = par ? 1 : G;
  auto hdots_of = [&](int s) { return par ? ctx->dred : ws.h(s) + hl.hd; };
  auto bcol = [&](int s) { return B + c.c[s] * ldb; };
  auto xcol = [&](int s) { return X + c.c[s] * ldx; };
  auto allreduce = [&](int64_t offset, int64_t count) -> int {
    ctx->cur_tag = F->id;
    return comm_allreduce(F, offset, count);
  };
  auto list = [&](const bool* on) {           // the slots that are on, as a column list of the workspace operands
    BlockCols b = block_chunk(nc, nullptr, 0);
    int m = 0;
    for (int s = 0; s < nc; ++s)
      if (on[s]) b.c[m++] = s;
    b.n = m;
    for (int i = m; i < BLOCK_NV; ++i) b.c[i] = m ? b.c[0] : 0;
    return b;
  };
  // out[s] = hs_s[off] for the slots that are on: the copies queued together, one synchronisation
  auto read = [&](const bool* on, int off, double* out) -> int {
    for (int s = 0; s < nc; ++s)
      if (on[s]) ALFI_HIP_CHECK(ctx, hipMemcpyAsync(out + s, ws.h(s) + off, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
  };
  // beta = |w| into hs (and the rotated right-hand side)
  auto norm_init = [&](int s) -> int {
    ALFI_CHECK(launch_norm_partials(ctx, ws.wv(s), n));
    if (par) {
      ALFI_CHECK(launch_reduce_partials(ctx, ctx->red_partial, G, 1, nrm2));
      ALFI_CHECK(allreduce(RED_MAXV, 1));
      return launch_norm_init_finish(ctx, nrm2, 1, ws.h(s), K);
    }
    return launch_norm_init_finish(ctx, ctx->red_partial, G, ws.h(s), K);
  };
  bool active[BLOCK_NV] = {false, false, false, false}, all[BLOCK_NV] = {false, false, false, false};
  double bnorm[BLOCK_NV] = {0, 0, 0, 0}, tol[BLOCK_NV] = {0, 0, 0, 0}, val[BLOCK_NV] = {0, 0, 0, 0};
  int its[BLOCK_NV] = {0, 0, 0, 0};
  for (int s = 0; s < nc; ++s) {
    all[s] = true;
    ALFI_HIP_CHECK(ctx, hipMemsetAsync(ws.h(s), 0, sizeof(double) * hl.total, ctx->stream));
    ALFI_HIP_CHECK(ctx, hipMemsetAsync(xcol(s), 0, sizeof(double) * n, ctx->stream));
    ALFI_CHECK(launch_copy(ctx, ws.wv(s), bcol(s), n));                           // r = b (zero initial guess)
    ALFI_CHECK(norm_init(s));
  }
  ALFI_CHECK(read(all, hl.beta, bnorm));
  int nactive = 0;
  for (int s = 0; s < nc; ++s) {
    tol[s] = std::max(rtol * bnorm[s], atol);
    active[s] = !(bnorm[s] <= tol[s]);
    nactive += active[s] ? 1 : 0;
  }
  // w_s = b_s - K x_s and beta_s = |w_s| for the slots in `on`, column by column (x is a column of the caller's operand, w one
  // of the workspace: two column lists, which the block product does not take)
  auto residual_of = [&](const bool* on) -> int {
    for (int s = 0; s < nc; ++s) {
      if (!on[s]) continue;
      ALFI_CHECK(alfi_saddle_mult(S, xcol(s), ws.wv(s)));
      ALFI_CHECK(launch_xmy(ctx, ws.wv(s), bcol(s), n));
      ALFI_CHECK(norm_init(s));
    }
    return 0;
  };
  int it = 0;                                   // iterations of every still active column
  while (nactive > 0 && it < max_it) {
    for (int s = 0; s < nc; ++s)
      if (active[s]) ALFI_CHECK(launch_scale_by_inv(ctx, ws.v(s, 0), ws.wv(s), ws.h(s) + hl.beta, n));      // v_0 = r / |r|
    int j = 0;
    bool cycle[BLOCK_NV];                        // the columns that run this restart cycle to its end
    for (int s = 0; s < nc; ++s) cycle[s] = active[s];
    int ncycle = nactive;
    for (; j < K && it < max_it && ncycle > 0; ++j) {
      const BlockCols a = list(cycle);
      ALFI_CHECK(saddle_precond_chunk(S, a, nc, ws.v(0, j), ws.vs(), ws.z(0, j), ws.zs()));          // z_j = P^-1 v_j
      ALFI_CHECK(saddle_mult_chunk(S, a, ws.z(0, j), ws.zs(), ws.w, ldv));                           // w = K z_j
      for (int s = 0; s < nc; ++s) {
        if (!cycle[s]) continue;
        double *hs = ws.h(s), *hdots = hdots_of(s);
        ALFI_CHECK(launch_multi_dot(ctx, ws.v(s, 0), ldv, j + 1, ws.wv(s), hdots, n));
        if (par) ALFI_CHECK(allreduce(0, j + 1));
        ALFI_CHECK(launch_multi_axpy_norm(ctx, ws.v(s, 0), ldv, j + 1, hdots, ws.wv(s), n, ctx->red_partial2, 0));
        if (par) {                                                              // |w - V h| by its own all-reduce (VecNorm)
          ALFI_CHECK(launch_reduce_partials(ctx, ctx->red_partial2, G, 1, nrm2));
          ALFI_CHECK(allreduce(RED_MAXV, 1));
        }
        ALFI_CHECK(launch_hessenberg_update(ctx, normpart, nblk, hdots, hs, j, K, nullptr));
      }
      ++it;
      ALFI_CHECK(read(cycle, hl.grs + j + 1, val));                            // |rotated rhs| = residual norm estimates
      for (int s = 0; s < nc; ++s) {
        if (!cycle[s]) continue;
        its[s] = it;
        if (std::fabs(val[s]) <= tol[s]) {                                     // converged: finished at its own j, out of the list
          ALFI_CHECK(launch_fgmres_finish(ctx, ws.h(s), j + 1, K));
          ALFI_CHECK(launch_update_solution(ctx, xcol(s), ws.z(s, 0), ldv, j + 1, ws.h(s) + hl.y, n));
          cycle[s] = active[s] = false;
          --ncycle;
          --nactive;
        } else if (j + 1 < K) {
          ALFI_CHECK(launch_scale_by_inv(ctx, ws.v(s, j + 1), ws.wv(s), ws.h(s) + hl.tt, n));
        }
      }
    }
    for (int s = 0; s < nc; ++s) {
      if (!cycle[s]) continue;
      ALFI_CHECK(launch_fgmres_finish(ctx, ws.h(s), j, K));
      ALFI_CHECK(launch_update_solution(ctx, xcol(s), ws.z(s, 0), ldv, j, ws.h(s) + hl.y, n));
    }
    if (nactive == 0 || it >= max_it) break;
    ALFI_CHECK(residual_of(active));                                           // restart: true residuals
    ALFI_CHECK(read(active, hl.beta, val));
    for (int s = 0; s < nc; ++s)
      if (active[s] && val[s] <= tol[s]) {
        active[s] = false;
        --nactive;
      }
  }
  ALFI_CHECK(residual_of(all));                                                // final true residual norms
  ALFI_CHECK(read(all, hl.beta, val));
  for (int s = 0; s < nc; ++s) {
    its_out[s] = its[s];
    rn_out[s] = val[s];
  }
  return 0;
}

static int check_restart(alfi_ctx* ctx, int restart) {
  if (restart < 1 || restart > RED_MAXV - 2) return alfi_set_error(ctx, ALFI_E_ARG, "restart must be in 1..%d", RED_MAXV - 2);
  return 0;
}

int alfi_saddle_solve(alfi_saddle* S, const double* db, double* dx, double rtol, double atol, int max_it, int restart,
                      int* iterations, double* residual_norm) {
  alfi_ctx* ctx = S->ctx;
  ALFI_CHECK(check_restart(ctx, restart));
  ALFI_CHECK(krylov_ws_ensure(ctx, &S->ws, 1, restart, S->nu_dofs + S->np_dofs));
  int its = 0;
  double rn = 0.0;
  ALFI_CHECK(saddle_solve_chunk(S, S->ws, block_chunk(1, nullptr, 0), db, 0, dx, 0, rtol, atol, max_it, &its, &rn));
  if (iterations) *iterations = its;
  if (residual_norm) *residual_norm = rn;
  // a persistent multiplicative sweep inside a cycle may have run into its wait bound: the iterates above were then computed
  // from an incomplete smoother result -- report it instead of returning counts and norms of garbage
  return check_dev_err(ctx);
}

int alfi_saddle_solve_block(alfi_saddle* S, int ncol, const int* cols, int nx, const double* B, int64_t ldb, double* X, int64_t ldx,
                            double rtol, double atol, int max_it, int restart, int* iterations, double* residual_norms) {
  const BlockOperand ops[2] = {{B, ldb, false}, {X, ldx, true}};
  ALFI_CHECK(saddle_block_check(S, "alfi_saddle_solve_block", ncol, cols, nx, ops, 2));
  alfi_ctx* ctx = S->ctx;
  if (!iterations || !residual_norms) return alfi_set_error(ctx, ALFI_E_ARG, "alfi_saddle_solve_block: NULL result arrays");
  ALFI_CHECK(check_restart(ctx, restart));
  ALFI_CHECK(krylov_ws_ensure(ctx, &S->blk_ws, block_slots_needed(S->blk_ws.slots, ncol), restart, S->nu_dofs + S->np_dofs));
  for (int q = 0; q < block_chunks(ncol); ++q)
    ALFI_CHECK(saddle_solve_chunk(S, S->blk_ws, block_chunk(ncol, cols, q), B, ldb, X, ldx, rtol, atol, max_it,
                                  iterations + q * BLOCK_NV, residual_norms + q * BLOCK_NV));
  return check_dev_err(ctx);
}
