// C ABI of libalfi_hip.so (include/alfi_hip.h), PCPATCH: patch sets, condensed factors, multiplicative schedules, factorisation, apply.
// (One file per concern since round 5: api_ctx / api_level / api_patches / api_smoother / api_cycles / api_saddle; the helpers they
// share are declared in api_internal.h.)
#include <optional>
#include "api_internal.h"
#include "find_groups.h"

static_assert(PLAN_E_ARG == ALFI_E_ARG, "the planners (patch_plan.h) return the C ABI's code");

// ---- the storage of a level's patch factors (state: common.h, questions: api_internal.h) ---------------------------------------
// Every function here expects the stream synchronised by its caller.

// the single-precision copy of the inverses and its offsets; the last FP32 level of the ctx takes the FP64 work buffer with it
static void free_f32(alfi_level* L) {
  if (L->inv32 && --L->ctx->f32_levels == 0) {
    dev_free(L->ctx->f32_work);
    L->ctx->f32_work = nullptr;
    L->ctx->f32_work_doubles = 0;
  }
  dev_free(L->inv32);
  dev_free(L->inv32_ptr);
  L->inv32 = nullptr;
  L->inv32_ptr = nullptr;
  L->inv32_floats = 0;
  std::vector<int64_t>().swap(L->f32_ptr);
  if (L->held == HELD_F32) set_held(L, HELD_NONE);
}

// `inv` as the 16-double placeholder: all a level has of dense FP64 inverses before its first dense factorisation, with condensed
// factors and with FP32 storage (never NULL once the patches are set: a kernel argument and part of the cycle graphs' signature)
static int inv_to_placeholder(alfi_level* L) {
  dev_free(L->inv);
  L->inv = nullptr;
  if (L->held == HELD_F64) set_held(L, HELD_NONE);
  return dev_alloc(L->ctx, &L->inv, 16);
}

void free_patch_factors(alfi_level* L) {
  dev_free(L->inv);
  L->inv = nullptr;
  dev_free(L->inv_il);
  L->inv_il = nullptr;
  L->il_doubles = 0;
  L->il_valid = false;
  free_f32(L);
  free_cond(L);
  set_held(L, HELD_NONE);
  L->store_req = STORE_REQ_F64;                   // a new patch set starts in FP64 and undecided about condensation
  L->cond_by = COND_UNDECIDED;
  L->factored = false;
}

// ---- patches -------------------------------------------------------------------------------------------------------------
int alfi_patches_set(alfi_level* L, int64_t npatch, const int64_t* pptr, const int32_t* pdofs) {
  alfi_ctx* ctx = L->ctx;
  if (npatch < 0 || (npatch > 0 && (!pptr || !pdofs))) return alfi_set_error(ctx, ALFI_E_ARG, "NULL patch arrays");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  dev_free(L->fc_ptr); dev_free(L->fc_col); dev_free(L->fc_fac); dev_free(L->fc_s);
  L->fc_ptr = nullptr; L->fc_col = nullptr; L->fc_fac = nullptr; L->fc_s = nullptr;
  dev_free(L->patch_ptr);
  dev_free(L->patch_dofs);
  dev_free(L->inv_ptr);
  dev_free(L->stage_ptr);
  free_patch_factors(L);
  dev_free(L->canon_rank);
  L->canon_rank = nullptr;
  dev_free(L->stage);
  block_release_patch_buffers(L);
  dev_free(L->dof_ptr);
  dev_free(L->dof_pos);
  L->patch_ptr = nullptr; L->patch_dofs = nullptr; L->inv_ptr = nullptr; L->stage_ptr = nullptr;
  L->stage = nullptr; L->dof_ptr = nullptr; L->dof_pos = nullptr;
  L->npatch = npatch;
  PatchLayout lay;
  std::string err;
  if (const int rc = plan_patch_layout(L->n, npatch, pptr, pdofs, PATCH_MAX, &lay, &err))
    return alfi_set_error(ctx, rc, "%s", err.c_str());
  ALFI_CHECK(dev_upload(ctx, &L->patch_ptr, pptr, npatch + 1));
  ALFI_CHECK(dev_upload(ctx, &L->patch_dofs, pdofs, lay.sum_n));
  ALFI_CHECK(dev_upload(ctx, &L->inv_ptr, lay.inv_ptr.data(), npatch + 1));
  ALFI_CHECK(dev_upload(ctx, &L->stage_ptr, lay.stage_ptr.data(), npatch + 1));
  ALFI_CHECK(dev_upload(ctx, &L->dof_ptr, lay.dof_ptr.data(), L->n + 1));
  ALFI_CHECK(dev_upload(ctx, &L->dof_pos, lay.dof_pos.data(), lay.sum_n));
  // the dense inverses (8 sum n_p^2 bytes) are allocated by the first alfi_patches_factor that needs them: a level that
  // gets condensed factors (alfi_patches_set_groups) never holds them -- 265 GB for the 3.4 M-dof Scott-Vogelius level
  ALFI_CHECK(inv_to_placeholder(L));
  ALFI_CHECK(dev_alloc(ctx, &L->stage, lay.stage_len));
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->stage, 0, (size_t)std::max<int64_t>(lay.stage_len, 1) * sizeof(double), ctx->stream));
  // later calls read patch_ptr, patch_dofs and inv_ptr on the host (copied here, while the device clears the staging buffer);
  // the other tables live on the device now
  lay.patch_ptr.assign(pptr, pptr + npatch + 1);
  lay.patch_dofs.assign(pdofs, pdofs + lay.sum_n);
  lay.release_tables();
  L->lay = std::move(lay);
  dev_free(L->mult_seq);
  L->mult_seq = nullptr;
  L->mult = false;
  free_mult_schedule(L);
  L->sweep = SweepPlan();
  // a new patch set invalidates the interior-patch count of alfi_level_set_overlap: back to the plain exchange until the
  // caller declares the new one
  L->overlap = false;
  L->npatch_int = 0;
  return 0;
}

// The two requests for FP32 storage.  What has no single-precision form is refused here, before any device work: the request
// is explicit, so nothing falls back to FP64 behind the caller's back.  The star request (alfi_patches_set_storage) also refuses
// what it has no kernel for (patches above 160 dofs) and no place for the facet rule for (a facet correction); the macro request
// (alfi_patches_set_macro_storage), the one macro stars and Burman levels can make, accepts both.
static int set_storage_request(alfi_level* L, int dtype, bool macro) {
  alfi_ctx* ctx = L->ctx;
  const char* fn = macro ? "alfi_patches_set_macro_storage" : "alfi_patches_set_storage";
  const char* what = macro ? "FP32 macro-star storage" : "FP32 patch storage";
  if (!L->patch_ptr) return alfi_set_error(ctx, ALFI_E_STATE, "%s before alfi_patches_set", fn);
  if (dtype != ALFI_STORAGE_F64 && dtype != ALFI_STORAGE_F32)
    return alfi_set_error(ctx, ALFI_E_ARG, "%s: dtype %d (0: FP64, 1: FP32)", fn, dtype);
  if (dtype == ALFI_STORAGE_F32) {
    if (L->npatch == 0) return alfi_set_error(ctx, ALFI_E_ARG, "%s: the level has no patches", what);
    if (L->lay.max_np <= 32)
      return alfi_set_error(ctx, ALFI_E_ARG, "%s: every patch has <= 32 dofs and the level applies the interleaved small-patch "
                                             "copy, which has no FP32 form", what);
    if (!macro && L->lay.max_np > SMALL_PATCH_MAX)
      return alfi_set_error(ctx, ALFI_E_ARG, "%s: a patch has %d dofs; the FP32 apply handles at most %d (macro stars keep FP64)",
                            what, L->lay.max_np, SMALL_PATCH_MAX);
    if (cond_by_caller(L))
      return alfi_set_error(ctx, ALFI_E_ARG, "%s: the level has caller-supplied groups; condensed factors cancel in single "
                                             "precision and stay FP64 (alfi_patches_set_groups(NULL) first)", what);
    if (L->mult) return alfi_set_error(ctx, ALFI_E_ARG, "%s: multiplicative sweeps read FP64 inverses", what);
    if (!macro && L->fc_ptr)
      return alfi_set_error(ctx, ALFI_E_ARG, "%s: the level has a facet correction (Burman); its patch matrices are factored "
                                             "and repaired in FP64 only", what);
  }
  // (the level keeps what it holds, and works with it, until the next alfi_patches_factor)
  L->store_req = dtype != ALFI_STORAGE_F32 ? STORE_REQ_F64 : macro ? STORE_REQ_F32_MACRO : STORE_REQ_F32_STAR;
  return 0;
}

int alfi_patches_set_storage(alfi_level* L, int dtype) { return set_storage_request(L, dtype, false); }
int alfi_patches_set_macro_storage(alfi_level* L, int dtype) { return set_storage_request(L, dtype, true); }

int alfi_ctx_set_f32_work_bytes(alfi_ctx* ctx, int64_t bytes) {
  if (bytes <= 0) return alfi_set_error(ctx, ALFI_E_ARG, "alfi_ctx_set_f32_work_bytes: %lld bytes", (long long)bytes);
  ctx->f32_work_cap = bytes;
  return 0;
}

int alfi_ctx_f32_work_bytes(alfi_ctx* ctx, int64_t* bytes) {
  if (bytes) *bytes = 8 * ctx->f32_work_doubles;
  return 0;
}

int alfi_patches_set_canonical_order(alfi_level* L, const int32_t* rank) {
  alfi_ctx* ctx = L->ctx;
  if (!L->patch_ptr) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_patches_set_canonical_order before alfi_patches_set");
  if (rank) {                                      // per patch a permutation of 0 .. n_p - 1
    std::vector<char> seen;
    for (int64_t p = 0; p < L->npatch; ++p) {
      const int64_t a = L->lay.patch_ptr[p], n = L->lay.patch_ptr[p + 1] - a;
      seen.assign((size_t)n, 0);
      for (int64_t q = 0; q < n; ++q) {
        if (rank[a + q] < 0 || rank[a + q] >= n || seen[(size_t)rank[a + q]])
          return alfi_set_error(ctx, ALFI_E_ARG, "patch %lld: the canonical order is not a permutation of its entries", (long long)p);
        seen[(size_t)rank[a + q]] = 1;
      }
    }
  }
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  dev_free(L->canon_rank);
  L->canon_rank = nullptr;
  if (rank) ALFI_CHECK(dev_upload(ctx, &L->canon_rank, rank, L->lay.sum_n));
  if (is_or_will_be_f32(L)) L->factored = false;   // the stored inverses belong to the old order
  return 0;
}

int alfi_patches_storage(alfi_level* L, int* dtype) {
  if (dtype) *dtype = L->held == HELD_F32 ? ALFI_STORAGE_F32 : ALFI_STORAGE_F64;
  return 0;
}

// the block sparsity of the level on the host (row starts are marked in the sign bit of the flat layout: masked by the readers)
static int download_sparsity(alfi_level* L, std::vector<int32_t>* rowptr, std::vector<int32_t>* colidx) {
  alfi_ctx* ctx = L->ctx;
  const int64_t nb = L->A.nbrows, nnzb = L->A.nnzb;
  rowptr->resize(nb + 1);
  colidx->resize(nnzb > 0 ? nnzb : 1);
  ALFI_HIP_CHECK(ctx, hipMemcpy(rowptr->data(), L->A.rowptr, sizeof(int32_t) * (nb + 1), hipMemcpyDeviceToHost));
  if (nnzb > 0) ALFI_HIP_CHECK(ctx, hipMemcpy(colidx->data(), L->A.colidx, sizeof(int32_t) * nnzb, hipMemcpyDeviceToHost));
  return 0;
}

// alfi_patches_set_groups for the caller's labels and for the library's own (alfi_patches_factor, which has the sparsity on
// the host already: sparsity = {rowptr, colidx}, else NULL)
static int set_groups_impl(alfi_level* L, const int32_t* group, const std::vector<int32_t>* const* sparsity = nullptr) {
  alfi_ctx* ctx = L->ctx;
  if (!L->patch_ptr) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_patches_set_groups before alfi_patches_set");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  free_cond(L);
  L->factored = false;
  if (!group) return 0;                                  // back to dense inverses (allocated by alfi_patches_factor)
  if (L->mult) return alfi_set_error(ctx, ALFI_E_STATE, "condensed patch factors do not support multiplicative sweeps");
  std::vector<int32_t> own_rowptr, own_colidx;
  if (!sparsity) ALFI_CHECK(download_sparsity(L, &own_rowptr, &own_colidx));
  const std::vector<int32_t>& rowptr = sparsity ? *sparsity[0] : own_rowptr;
  const std::vector<int32_t>& colidx = sparsity ? *sparsity[1] : own_colidx;
  CondPlan pl;
  std::string err;
  if (const int rc = plan_condensed(L->bs, L->A.nbrows, L->npatch, L->lay.patch_ptr.data(), L->lay.patch_dofs.data(), group,
                                    rowptr.data(), colidx.data(), COND_SIGMA_ROWS, &pl, &err))
    return alfi_set_error(ctx, rc, "%s", err.c_str());
  CondDev cd;
  // every table of the plan under its name in CondDev, in this order
#define ALFI_COND_UP(f) ALFI_CHECK(cond_upload(L, &cd.f, pl.f))
  ALFI_COND_UP(dofs); ALFI_COND_UP(slot); ALFI_COND_UP(gptr); ALFI_COND_UP(g_off); ALFI_COND_UP(g_m); ALFI_COND_UP(g_sc);
  ALFI_COND_UP(g_uoff); ALFI_COND_UP(g_mat); ALFI_COND_UP(g_sidx); ALFI_COND_UP(sidx); ALFI_COND_UP(p_nI); ALFI_COND_UP(sptr);
  ALFI_COND_UP(sinv_ptr); ALFI_COND_UP(s_uptr); ALFI_COND_UP(s_uidx); ALFI_COND_UP(order);
  // the three-launch apply: sigma chunks, the row-sorted u buffer, row pairs, group chunks
  ALFI_COND_UP(ch_patch); ALFI_COND_UP(ch_row); ALFI_COND_UP(uptr); ALFI_COND_UP(u_dst); ALFI_COND_UP(xp_ptr); ALFI_COND_UP(xp_grp);
  ALFI_COND_UP(g_xp); ALFI_COND_UP(bp_ptr); ALFI_COND_UP(bp_grp); ALFI_COND_UP(g_bp); ALFI_COND_UP(gc);
#undef ALFI_COND_UP
  ALFI_CHECK(dev_alloc(ctx, &cd.ubuf, pl.uptr.back()));
  L->cond_allocs.push_back(cd.ubuf);
  ALFI_CHECK(dev_alloc(ctx, &cd.tmp, L->lay.sum_n));
  L->cond_allocs.push_back(cd.tmp);
  ALFI_CHECK(dev_alloc(ctx, &cd.mat, pl.mat_doubles));
  L->cond_allocs.push_back(cd.mat);
  ALFI_CHECK(dev_alloc(ctx, &cd.sinv, pl.sinv_doubles));
  L->cond_allocs.push_back(cd.sinv);
  // the dense inverses are not needed any more
  if (L->held == HELD_F64) ALFI_CHECK(inv_to_placeholder(L));
  L->cd = cd;
  set_held(L, HELD_COND);
  L->il_valid = false;
  pl.release_tables();                                   // the host keeps sptr, gptr, chptr, gcptr and the limits
  L->cplan = std::move(pl);
  return 0;
}

int alfi_patches_set_groups(alfi_level* L, const int32_t* group) {
  if (group && is_or_will_be_f32(L))
    return alfi_set_error(L->ctx, ALFI_E_STATE, "alfi_patches_set_groups on a level with FP32 patch storage: condensed factors "
                                                "stay FP64 (alfi_patches_set_storage(lvl, 0) first)");
  const int rc = set_groups_impl(L, group);
  // the caller has decided for this patch set, NULL (dense inverses) included: no search for groups at the factorisation
  L->cond_by = rc != 0 ? COND_UNDECIDED : group ? COND_BY_CALLER : COND_DENSE;
  return rc;
}

static int find_groups(alfi_level* L, int32_t* group_out, int64_t* npatch_grouped, std::vector<int32_t>* rowptr_out = nullptr,
                       std::vector<int32_t>* colidx_out = nullptr) {
  alfi_ctx* ctx = L->ctx;
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<int32_t> own_rowptr, own_colidx;
  std::vector<int32_t>& rowptr = rowptr_out ? *rowptr_out : own_rowptr;
  std::vector<int32_t>& colidx = colidx_out ? *colidx_out : own_colidx;
  ALFI_CHECK(download_sparsity(L, &rowptr, &colidx));
  const int64_t ng = alfi_find_groups_host(L->bs, L->A.nbrows, L->npatch, L->lay.patch_ptr.data(), L->lay.patch_dofs.data(),
                                           rowptr.data(), colidx.data(), group_out);
  if (npatch_grouped) *npatch_grouped = ng;
  return 0;
}

int alfi_patches_find_groups(alfi_level* L, int32_t* group_out) {
  alfi_ctx* ctx = L->ctx;
  if (!L->patch_ptr) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_patches_find_groups before alfi_patches_set");
  if (!group_out) return alfi_set_error(ctx, ALFI_E_ARG, "group_out is NULL");
  return find_groups(L, group_out, nullptr);
}

int alfi_ctx_set_condense_min_bytes(alfi_ctx* ctx, int64_t min_bytes) {
  ctx->condense_min_bytes = min_bytes;
  return 0;
}

int alfi_patches_condensed(alfi_level* L, int* mode) {
  if (mode) *mode = !L->cond ? 0 : (cond_by_own_choice(L) ? 2 : 1);
  return 0;
}

int alfi_patches_factor_bytes(alfi_level* L, int64_t* bytes) {
  if (L->held == HELD_F32) {
    *bytes = 4 * L->inv32_floats;
  } else if (wants_f32(L)) {                          // not factored yet: what the factorisation will store
    std::vector<int64_t> ptr;
    *bytes = 4 * plan_f32_offsets(L->npatch, L->lay.patch_ptr.data(), &ptr);
  } else {
    *bytes = L->cond ? 8 * (L->cplan.mat_doubles + L->cplan.sinv_doubles) : 8 * L->lay.inv_doubles;
  }
  return 0;
}

// A level that condensed itself (or has not decided yet) and now gets something the condensed factors do not support --
// multiplicative sweeps, PCPATCH's facet rule, FP32 storage -- goes back to dense inverses for good.  The condensed storage is
// released here (the two are never held together); returns whether the level was factored: the caller factors it again.
// (Groups of the caller's are the caller's to withdraw: such a level stays as it is.)
bool auto_cond_to_dense(alfi_level* L) {
  bool refactor = false;
  if (cond_by_own_choice(L)) {
    refactor = L->factored;
    free_cond(L);
    L->factored = false;
  }
  if (L->cond_by != COND_BY_CALLER) L->cond_by = COND_DENSE;
  return refactor;
}

void free_mult_schedule(alfi_level* L) {
  dev_free(L->mult_items); dev_free(L->mult_pred0); dev_free(L->mult_pred); dev_free(L->mult_succ_ptr);
  dev_free(L->mult_succ); dev_free(L->mult_ctl); dev_free(L->mult_rowtab);
  dev_free(L->mcw_gchunk); dev_free(L->mcw_schunk); dev_free(L->mcw_node); dev_free(L->mcw_r);
  L->mcw_gchunk = L->mcw_schunk = L->mcw_node = nullptr;
  L->mcw_r = nullptr;
  std::vector<int64_t>().swap(L->mcw_wk_ptr);
  std::vector<int64_t>().swap(L->mcw_wc_ptr);
  std::vector<int64_t>().swap(L->mcw_wn_ptr);
  L->mult_rowtab = nullptr;
  L->mult_items = L->mult_pred0 = L->mult_pred = L->mult_succ_ptr = L->mult_succ = L->mult_ctl = nullptr;
  L->sweep.nitems = 0;
}

// alfi_patches_set_multiplicative, and -- keep_cond -- alfi_patches_set_multiplicative_condensed on a level with the caller's
// groups: the same arguments, refusals and schedule; the level keeps its condensed factors and gets the work lists of the
// wavefronts (plan_sweep_condensed) in addition
static int set_multiplicative_impl(alfi_level* L, int64_t nit, const int64_t* iterset, int symmetrise, bool keep_cond) {
  alfi_ctx* ctx = L->ctx;
  if (!L->patch_ptr) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_patches_set_multiplicative before alfi_patches_set");
  ALFI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  dev_free(L->mult_seq);
  L->mult_seq = nullptr;
  L->mult = false;
  free_mult_schedule(L);
  L->sweep = SweepPlan();
  // a new schedule starts with a clean device-side error word: after a timeout every later sweep on this ctx would stop at its
  // first wait (the word is tested inside the spin loop); (re)setting the sweeps is how a context recovers
  if (ctx->dev_err) ALFI_HIP_CHECK(ctx, hipMemset(ctx->dev_err, 0, 16));
  if (nit == 0) return 0;
  if (nit < 0 || !iterset) return alfi_set_error(ctx, ALFI_E_ARG, "bad iteration set");
  if (is_or_will_be_f32(L))
    return alfi_set_error(ctx, ALFI_E_STATE, "multiplicative sweeps on a level with FP32 patch storage: the sweeps read FP64 "
                                             "inverses (alfi_patches_set_storage(lvl, 0) first)");
  if (cond_by_caller(L) && !keep_cond)
    return alfi_set_error(ctx, ALFI_E_STATE, "multiplicative sweeps need dense patch inverses (alfi_patches_set_groups(NULL))");
  // (groups the library found itself are its own business: the sweeps read dense inverses, so such a level goes back to them
  // below, once the arguments have been checked, and is factored again at the end)
  if (L->pou) return alfi_set_error(ctx, ALFI_E_STATE, "partition of unity applies to the additive smoother");
  // partitioned levels: every rank sweeps over its own patches with the residual of its local vector (ghost slots hold
  // the rank's own contributions only) and the ghost contributions are added onto their owners at the end -- what
  // PCPATCH does under MPI: local Gauss-Seidel, additive between ranks [3P]
  if (nit > INT32_MAX) return alfi_set_error(ctx, ALFI_E_ARG, "iteration set too long");
  // patches must be unions of whole nodes (the sweep works on block rows); up to 64 nodes and 160 dofs a wave sweeps a
  // patch, beyond (macro stars) a workgroup does
  const int64_t* pp = L->lay.patch_ptr.data();
  const int32_t* pd = L->lay.patch_dofs.data();
  std::string err;
  SweepPlan sw;
  const int check_rc = check_sweep(L->bs, L->npatch, pp, pd, SMALL_PATCH_MAX, nit, iterset, &sw.big, &err);
  L->sweep.big = sw.big;
  if (check_rc != 0) return alfi_set_error(ctx, check_rc, "%s", err.c_str());
  // every argument is checked: now a level that condensed itself goes back to dense inverses (auto_cond_to_dense)
  const bool refactor = auto_cond_to_dense(L);
  // sparsity of the operator on the host (row starts are marked in the sign bit of the flat layout)
  std::vector<int32_t> rowptr, colidx;
  ALFI_CHECK(download_sparsity(L, &rowptr, &colidx));
  // (the plan fails only at the int32 limits of the persistent schedule: the per-wavefront schedule is complete and set then)
  const int plan_rc = plan_sweep(L->bs, L->A.nbrows, L->npatch, pp, pd, rowptr.data(), colidx.data(), nit, iterset, symmetrise != 0,
                                 sw.big, &sw, &err);
  ALFI_CHECK(dev_upload(ctx, &L->mult_seq, sw.seq.data(), nit));
  if (keep_cond) {
    // the lists the condensed launches take per wavefront, and the residual vector; set before the level counts as sweeping
    SweepCondPlan sc;
    const int64_t nwave = (int64_t)sw.wave_ptr.size() - 1;
    if (const int rc = plan_sweep_condensed(L->bs, L->npatch, pp, pd, nwave, sw.wave_ptr.data(), sw.seq.data(), L->cplan.gcptr.data(),
                                            L->cplan.chptr.data(), &sc, &err))
      return alfi_set_error(ctx, rc, "%s", err.c_str());
    ALFI_CHECK(dev_upload(ctx, &L->mcw_gchunk, sc.gchunk.data(), (int64_t)sc.gchunk.size()));
    ALFI_CHECK(dev_upload(ctx, &L->mcw_schunk, sc.schunk.data(), (int64_t)sc.schunk.size()));
    ALFI_CHECK(dev_upload(ctx, &L->mcw_node, sc.node.data(), (int64_t)sc.node.size()));
    ALFI_CHECK(dev_alloc(ctx, &L->mcw_r, L->n));
    ALFI_HIP_CHECK(ctx, hipMemset(L->mcw_r, 0, sizeof(double) * (size_t)std::max<int64_t>(L->n, 1)));
    L->mcw_wk_ptr = std::move(sc.wk_ptr);
    L->mcw_wc_ptr = std::move(sc.wc_ptr);
    L->mcw_wn_ptr = std::move(sc.wn_ptr);
  }
  L->sweep.wave_ptr = std::move(sw.wave_ptr);
  L->mult = true;
  L->mult_symmetrise = symmetrise != 0;
  if (!sw.big) ALFI_CHECK(dev_upload(ctx, &L->mult_rowtab, sw.rowtab.data(), (int64_t)sw.rowtab.size()));
  if (plan_rc != 0) return alfi_set_error(ctx, plan_rc, "%s", err.c_str());
  const int64_t N = sw.nitems;
  ALFI_CHECK(dev_upload(ctx, &L->mult_items, sw.items.data(), N));
  ALFI_CHECK(dev_upload(ctx, &L->mult_pred0, sw.pred0.data(), N));
  ALFI_CHECK(dev_alloc(ctx, &L->mult_pred, N));
  ALFI_CHECK(dev_upload(ctx, &L->mult_succ_ptr, sw.succ_ptr.data(), N + 1));
  ALFI_CHECK(dev_upload(ctx, &L->mult_succ, sw.succ.data(), (int64_t)sw.succ.size()));
  ALFI_CHECK(dev_alloc(ctx, &L->mult_ctl, 4));
  L->sweep.nitems = sw.nitems;                           // last: until every table is there the sweeps launch per wavefront
  if (refactor) ALFI_CHECK(alfi_patches_factor(L));
  return 0;
}

int alfi_patches_set_multiplicative(alfi_level* L, int64_t nit, const int64_t* iterset, int symmetrise) {
  return set_multiplicative_impl(L, nit, iterset, symmetrise, false);
}

int alfi_patches_set_multiplicative_condensed(alfi_level* L, int64_t nit, const int64_t* iterset, int symmetrise) {
  // without the caller's groups (a level that condensed itself included: it goes back to dense inverses) this is the call above
  const bool keep = nit != 0 && cond_by_caller(L);
  if (keep && level_is_partitioned(L))
    return alfi_set_error(L->ctx, ALFI_E_ARG, "alfi_patches_set_multiplicative_condensed: sweeps over condensed factors on a "
                                              "partitioned level are not built");
  return set_multiplicative_impl(L, nit, iterset, symmetrise, keep);
}

int alfi_patches_set_partition_of_unity(alfi_level* L, int on) {
  if (on && L->mult) return alfi_set_error(L->ctx, ALFI_E_STATE, "partition of unity applies to the additive smoother");
  L->pou = on != 0;
  return 0;
}

int alfi_patches_multiplicative_levels(alfi_level* L, int64_t* nwave) {
  *nwave = L->mult ? (int64_t)L->sweep.wave_ptr.size() - 1 : 0;
  return 0;
}

// ---- the factorisation: decide (condensation, storage), prepare the storage, one pass per range of patches -----------------------

// Who decides about condensation, if nobody has for this patch set.
static int decide_condensation(alfi_level* L) {
  alfi_ctx* ctx = L->ctx;
  // an FP32 level does not condense, whatever its dense bytes and the threshold: it counts as decided (groups the library found
  // at an earlier FP64 factorisation go)
  if (wants_f32(L)) (void)auto_cond_to_dense(L);
  if (L->cond_by != COND_UNDECIDED) return 0;
  // first factorisation of a patch set the caller gave no groups for: an additive level whose dense inverses would take
  // condense_min_bytes or more looks for groups in its own sparsity (find_groups.h) and stores condensed factors if it finds
  // any.  On a partitioned level all of this is the rank's own business: its patches (ghost dofs included: the local operator
  // holds their rows over the local columns), its sparsity, its inverse bytes against the threshold -- no collective, and
  // ranks of one level may decide differently (the block factorisation is exact for any valid grouping).
  L->cond_by = COND_DENSE;
  const int64_t thr = ctx->condense_min_bytes;
  // (never a Burman level: its sparsity couples cells across facets, alfi_level_set_facet_blocks, and PCPATCH's facet rule,
  // alfi_patches_set_facet_correction, changes the patch matrices)
  const bool facets = L->facet_blocks || L->fc_ptr;
  if (thr < 0 || L->mult || facets || L->npatch == 0 || 8 * L->lay.inv_doubles < thr) return 0;
  std::vector<int32_t> group((size_t)L->lay.sum_n), rowptr, colidx;
  int64_t grouped = 0;
  ALFI_CHECK(find_groups(L, group.data(), &grouped, &rowptr, &colidx));
  if (grouped == 0) return 0;
  // (the finder keeps to the limits of the format; a failure here is an error like any other, and leaves no condensed storage)
  const std::vector<int32_t>* sparsity[2] = {&rowptr, &colidx};
  const int rc = set_groups_impl(L, group.data(), sparsity);
  if (rc != 0) {
    free_cond(L);
    return rc;
  }
  L->cond_by = COND_BY_LIBRARY;
  return 0;
}

// The storage the factorisation writes to, and the ranges of patches it runs in: one, [0, npatch), except for an FP32 level of
// big patches.  An FP32 level is factored -- gather, Gauss-Jordan, probe, repair, all unchanged -- in the ctx's FP64 work buffer
// and keeps the single-precision copy made from it; small patches need the whole level there, big patches pass through range by
// range (plan_f32_ranges, alfi_ctx_set_f32_work_bytes).
static int prepare_factor_storage(alfi_level* L, PatchStoreHeld target, std::vector<int64_t>* ranges) {
  alfi_ctx* ctx = L->ctx;
  ranges->assign({0, L->npatch});
  if (target == HELD_F32) {
    ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    L->factored = false;                           // from here to the end of the factorisation the level holds nothing an apply may read
    if (L->held == HELD_F64) ALFI_CHECK(inv_to_placeholder(L));   // FP64 inverses of an earlier factorisation
    if (!L->inv32) {
      L->inv32_floats = plan_f32_offsets(L->npatch, L->lay.patch_ptr.data(), &L->f32_ptr);
      ALFI_CHECK(dev_upload(ctx, &L->inv32_ptr, L->f32_ptr.data(), L->npatch + 1));
      ALFI_CHECK(dev_alloc(ctx, &L->inv32, L->inv32_floats));
      ++ctx->f32_levels;
      ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->inv32, 0, sizeof(float) * (size_t)std::max<int64_t>(L->inv32_floats, 1), ctx->stream));
    }
    int64_t work = L->lay.inv_doubles;
    if (L->lay.max_np > SMALL_PATCH_MAX)
      work = plan_f32_ranges(L->npatch, L->lay.inv_ptr.data(), std::max<int64_t>(ctx->f32_work_cap / 8, 1), ranges);
    if (ctx->f32_work_doubles < work) {
      dev_free(ctx->f32_work);
      ctx->f32_work = nullptr;
      ctx->f32_work_doubles = 0;
      ALFI_CHECK(dev_alloc(ctx, &ctx->f32_work, work));
      ctx->f32_work_doubles = work;
    }
    return 0;
  }
  if (L->inv32) {                                  // back to FP64
    ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    L->factored = false;
    free_f32(L);
  }
  if (target == HELD_F64 && L->held != HELD_F64) { // first dense factorisation of this patch set
    ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    dev_free(L->inv);
    L->inv = nullptr;
    ALFI_CHECK(dev_alloc(ctx, &L->inv, L->lay.inv_doubles));
    set_held(L, HELD_F64);
  }
  return 0;
}

// Where the kernels of the pass that starts at patch p0 find the dense FP64 inverses they work on: they address patch p at
// base + inv_ptr[p].  An FP64 level is factored in place.  An FP32 level is factored in the ctx's work buffer, which holds the
// range's patches from its own start: the base is the buffer's address less the range's first offset, so that
// base + inv_ptr[p0] is the buffer and only the range's patches are touched.  (For p0 > 0 that address lies before the buffer;
// it is formed in integers and never dereferenced.)
static double* range_base(const alfi_level* L, PatchStoreHeld target, int64_t p0) {
  if (target != HELD_F32) return L->inv;
  return reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(L->ctx->f32_work) -
                                   sizeof(double) * (uintptr_t)L->lay.inv_ptr[(size_t)p0]);
}

// The factor kernels of one pass: the patches [p0, p1), inverses to inv + inv_ptr[p] (condensed factors and dense levels of small
// patches: the whole level).
static int launch_factor_range(alfi_level* L, PatchStoreHeld target, double* inv, int64_t p0, int64_t p1) {
  if (target == HELD_COND) return launch_cond_factor(L);      // group inverses + Schur complements
  if (L->lay.max_np > SMALL_PATCH_MAX) {
    // macro-star sized patches: blocked Gauss-Jordan on the matrix cores (facet rule and polish inside).  A patch's elimination
    // reads its own scratch only, so what is stored does not depend on the ranges.
    ALFI_CHECK(launch_big_factor_range(L, inv, p0, p1));
  } else {
    // (an FP32 level with a canonical order eliminates in that order and turns the inverses back: the rest sees patch_dofs' order)
    const bool ranked = target == HELD_F32 && L->canon_rank;
    ALFI_CHECK(launch_patch_gather_dense(L, inv, ranked));
    if (facet_rule_active(L)) ALFI_CHECK(launch_patch_facet_correct(L, 0, L->npatch, L->inv_ptr, inv, 0));
    ALFI_CHECK(launch_patch_invert(L, inv));
    if (ranked) ALFI_CHECK(launch_patch_unrank(L, inv));
  }
  return build_patch_il(L, inv);                  // small-patch levels: the wave-contiguous copy the apply streams
}

int alfi_patches_factor(alfi_level* L) {
  alfi_ctx* ctx = L->ctx;
  if (!L->patch_ptr) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_patches_factor before alfi_patches_set");
  ALFI_CHECK(decide_condensation(L));
  const PatchStoreHeld target = L->cond ? HELD_COND : wants_f32(L) ? HELD_F32 : HELD_F64;
  std::optional<ProfScope> prof;                   // the factor kernels of every pass (the first one: with the storage's allocation)
  prof.emplace(ctx, ALFI_EV_PATCH_FACTOR);
  ALFI_HIP_CHECK(ctx, hipMemsetAsync(L->status, 0, sizeof(int), ctx->stream));
  std::vector<int64_t> ranges;
  ALFI_CHECK(prepare_factor_storage(L, target, &ranges));
  if (target == HELD_COND && facet_rule_active(L))
    return alfi_set_error(ctx, ALFI_E_STATE, "condensed patch factors on a Burman level (the facet rule couples macro interiors)");
  // Every pass: the factor kernels, their status, then -- with the FP64 kernels on the FP64 inverses, whatever the level will
  // store -- the probe of every inverse (|| A_p X_p e - e ||), the pivoted re-inversion of the ones that fail (an unpivoted
  // elimination met a zero or tiny pivot; the reference's LAPACK / UMFPACK factorisations pivot) and the second probe; for an
  // FP32 level the rounding of the probed (and repaired) inverses into its copy.
  double* probe_vec = nullptr;                     // one per factorisation, made when the first pass has its inverses
  PatchCheckAcc acc;
  int rc = 0;
  for (size_t r = 0; r + 1 < ranges.size() && rc == 0; ++r) {
    const int64_t p0 = ranges[r], p1 = ranges[r + 1];
    double* inv = range_base(L, target, p0);
    if (!prof) prof.emplace(ctx, ALFI_EV_PATCH_FACTOR);
    rc = launch_factor_range(L, target, inv, p0, p1);
    prof.reset();
    int st = 0;
    if (rc == 0 && (hipMemcpyAsync(&st, L->status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                    hipStreamSynchronize(ctx->stream) != hipSuccess))
      rc = alfi_set_error(ctx, ALFI_E_HIP, "reading the factorisation status failed");
    if (rc == 0 && !probe_vec) rc = patch_probe_vector(L, &probe_vec);
    if (rc == 0) rc = patch_verify_and_repair_range(L, inv, st, p0, p1, probe_vec, &acc);
    if (rc == 0 && target == HELD_F32) rc = launch_patch_f32_convert_range(L, inv, p0, p1);
  }
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(probe_vec);
  patch_check_finish(L, acc);
  ALFI_CHECK(rc);
  set_held(L, target);                             // what was factored is what the level holds, and may be applied, from here on
  L->factored = true;
  return 0;
}


int alfi_patches_check(alfi_level* L, double* worst_residual, int64_t* flagged, int64_t* repaired, double* worst_after) {
  if (!L->factored) return alfi_set_error(L->ctx, ALFI_E_STATE, "alfi_patches_check before alfi_patches_factor");
  if (worst_residual) *worst_residual = L->chk_worst;
  if (flagged) *flagged = L->chk_flagged;
  if (repaired) *repaired = L->chk_repaired;
  if (worst_after) *worst_after = L->chk_flagged > 0 ? L->chk_worst_after : L->chk_worst;
  return 0;
}

int alfi_patch_apply(alfi_level* L, const double* dx, double* dy) {
  if (!level_pc_ready(L)) return alfi_set_error(L->ctx, ALFI_E_STATE, "alfi_patch_apply before alfi_patches_factor");
  if (dx == dy) return alfi_set_error(L->ctx, ALFI_E_ARG, "alfi_patch_apply: x and y must not alias");
  L->ctx->cur_tag = L->id;
  return level_patch_apply(L, dx, dy);
}

// TEST HOOK: the additive apply as two range launches, [0, split) and [split, npatch), then the dof-wise sum -- what the
// overlapped exchange of a partitioned level does with its patch ranges, on a serial level
int alfi_patch_apply_split(alfi_level* L, int64_t split, const double* dx, double* dy) {
  alfi_ctx* ctx = L->ctx;
  if (!L->factored) return alfi_set_error(ctx, ALFI_E_STATE, "alfi_patch_apply_split before alfi_patches_factor");
  if (dx == dy) return alfi_set_error(ctx, ALFI_E_ARG, "alfi_patch_apply_split: x and y must not alias");
  if (L->mult || L->jacobi || level_is_partitioned(L))
    return alfi_set_error(ctx, ALFI_E_STATE, "alfi_patch_apply_split: additive patch solves on a serial level only");
  if (split < 0 || split > L->npatch) return alfi_set_error(ctx, ALFI_E_ARG, "alfi_patch_apply_split: split out of range");
  ctx->cur_tag = L->id;
  ALFI_CHECK(launch_patch_apply_range(L, 0, split, dx));
  ALFI_CHECK(launch_patch_apply_range(L, split, L->npatch, dx));
  return launch_patch_sum(L, dx, dy);
}

int alfi_patches_stats(alfi_level* L, int64_t* npatch, int64_t* sum_n, int64_t* sum_n2) {
  if (npatch) *npatch = L->npatch;
  if (sum_n) *sum_n = L->lay.sum_n;
  if (sum_n2) *sum_n2 = L->lay.sum_n2;
  return 0;
}

// The dense inverse of a condensed patch, assembled on the host from its factors (a diagnostic: FP64 on the host, no kernel):
// column j is the block factorisation applied to e_j in the operation order of the apply,
//     t_g = X_g x_g,  rhs = x_S - sum_g B_g t_g,  y_S = inv(Sigma) rhs,  y_g = t_g - W_g y_S[S_g].
static int cond_get_inverse(alfi_level* L, int64_t p, double* out) {
  alfi_ctx* ctx = L->ctx;
  const CondDev& cd = L->cd;
  const int64_t off = L->lay.patch_ptr[p];
  const int n = (int)(L->lay.patch_ptr[p + 1] - off);
  const int64_t g0 = L->cplan.gptr[p], g1 = L->cplan.gptr[p + 1];
  const int ng = (int)(g1 - g0);
  const int s = (int)(L->cplan.sptr[p + 1] - L->cplan.sptr[p]), nI = n - s, ld = (s + 1) & ~1;
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return bytes == 0 ? hipSuccess : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  };
  std::vector<int32_t> slot(n), g_off(ng), g_m(ng), g_sc(ng);
  std::vector<int64_t> g_mat(ng), g_sidx(ng);
  std::vector<double> sinv((size_t)s * ld);
  int64_t sinv_off = 0;
  ALFI_HIP_CHECK(ctx, down(slot.data(), cd.slot + off, sizeof(int32_t) * n));
  ALFI_HIP_CHECK(ctx, down(g_off.data(), cd.g_off + g0, sizeof(int32_t) * ng));
  ALFI_HIP_CHECK(ctx, down(g_m.data(), cd.g_m + g0, sizeof(int32_t) * ng));
  ALFI_HIP_CHECK(ctx, down(g_sc.data(), cd.g_sc + g0, sizeof(int32_t) * ng));
  ALFI_HIP_CHECK(ctx, down(g_mat.data(), cd.g_mat + g0, sizeof(int64_t) * ng));
  ALFI_HIP_CHECK(ctx, down(g_sidx.data(), cd.g_sidx + g0, sizeof(int64_t) * ng));
  ALFI_HIP_CHECK(ctx, down(&sinv_off, cd.sinv_ptr + p, sizeof(int64_t)));
  ALFI_HIP_CHECK(ctx, down(sinv.data(), cd.sinv + sinv_off, sizeof(double) * sinv.size()));
  std::vector<std::vector<double>> mat(ng);
  std::vector<std::vector<int32_t>> si(ng);
  for (int g = 0; g < ng; ++g) {
    mat[g].resize((size_t)cond_group_doubles(g_m[g], g_sc[g]));
    si[g].resize(g_sc[g]);
    ALFI_HIP_CHECK(ctx, down(mat[g].data(), cd.mat + g_mat[g], sizeof(double) * mat[g].size()));
    ALFI_HIP_CHECK(ctx, down(si[g].data(), cd.sidx + g_sidx[g], sizeof(int32_t) * g_sc[g]));
  }
  std::vector<double> x(n), y(n), rhs(s);
  for (int j = 0; j < n; ++j) {                    // column j of the inverse in the condensed order
    std::fill(x.begin(), x.end(), 0.0);
    x[j] = 1.0;
    for (int i = 0; i < s; ++i) rhs[i] = x[nI + i];
    for (int g = 0; g < ng; ++g) {
      const int m = g_m[g], sc = g_sc[g], o = g_off[g], ldm = cond_ldim(m), ldsc = cond_ldim(sc);
      const double* X = mat[g].data();
      const double* B = X + (size_t)ldm * m;
      for (int i = 0; i < m; ++i) {
        double acc = 0.0;
        for (int k = 0; k < m; ++k) acc += X[(size_t)k * ldm + i] * x[o + k];
        y[o + i] = acc;                            // t_g
      }
      for (int i = 0; i < sc; ++i) {
        double acc = 0.0;
        for (int k = 0; k < m; ++k) acc += B[(size_t)k * ldsc + i] * y[o + k];
        rhs[si[g][i]] -= acc;
      }
    }
    for (int i = 0; i < s; ++i) {
      double acc = 0.0;
      for (int k = 0; k < s; ++k) acc += sinv[patch_inv_index(i, k, s, ld)] * rhs[k];
      y[nI + i] = acc;
    }
    for (int g = 0; g < ng; ++g) {
      const int m = g_m[g], sc = g_sc[g], o = g_off[g], ldm = cond_ldim(m);
      const double* W = mat[g].data() + (size_t)ldm * m + (size_t)cond_ldim(sc) * m;
      for (int i = 0; i < m; ++i) {
        double acc = 0.0;
        for (int k = 0; k < sc; ++k) acc += W[(size_t)k * ldm + i] * y[nI + si[g][k]];
        y[o + i] -= acc;
      }
    }
    for (int i = 0; i < n; ++i) out[(int64_t)slot[i] * n + slot[j]] = y[i];
  }
  return 0;
}

int alfi_patch_get_inverse(alfi_level* L, int64_t p, double* out) {
  alfi_ctx* ctx = L->ctx;
  if (!L->factored) return alfi_set_error(ctx, ALFI_E_STATE, "patches not factored");
  if (p < 0 || p >= L->npatch) return alfi_set_error(ctx, ALFI_E_ARG, "patch index out of range");
  if (L->cond) return cond_get_inverse(L, p, out);
  const int64_t n = L->lay.patch_ptr[p + 1] - L->lay.patch_ptr[p];
  if (L->held == HELD_F32) {                       // the stored floats, widened
    std::vector<float> tmp32((size_t)(n * f32_ld((int)n)));
    ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ALFI_HIP_CHECK(ctx, hipMemcpy(tmp32.data(), L->inv32 + L->f32_ptr[(size_t)p], tmp32.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < n; ++j) out[i * n + j] = (double)tmp32[(size_t)f32_inv_index((int)i, (int)j, (int)n)];
    return 0;
  }
  const int64_t ld = (n + 1) & ~(int64_t)1;
  std::vector<double> tmp(n * ld);
  ALFI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ALFI_HIP_CHECK(ctx, hipMemcpy(tmp.data(), L->inv + L->lay.inv_ptr[p], tmp.size() * sizeof(double),
                                hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) out[i * n + j] = tmp[patch_inv_index((int)i, (int)j, (int)n, (int)ld)];
  return 0;
}
