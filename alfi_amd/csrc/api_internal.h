// Shared by the api_*.hip files (the C ABI of libalfi_hip.so, include/alfi_hip.h): device allocation helpers and the functions one
// concern's file offers the others.  Not part of the ABI.  The public entry points get their C linkage from alfi_hip.h.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include "common.h"
#include "hs_layout.h"

template <typename T>
inline int dev_alloc(alfi_ctx* ctx, T** p, int64_t count) {
  *p = nullptr;
  if (count <= 0) count = 1;
  ALFI_HIP_CHECK(ctx, hipMalloc((void**)p, (size_t)count * sizeof(T)));
  return 0;
}
template <typename T>
inline int dev_upload(alfi_ctx* ctx, T** p, const T* host, int64_t count) {
  ALFI_CHECK(dev_alloc(ctx, p, count));
  if (count > 0) ALFI_HIP_CHECK(ctx, hipMemcpy(*p, host, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
inline void dev_free(void* p) {
  if (p) (void)hipFree(p);
}
// an array of a level's condensed patch factors: uploaded, remembered for free_cond
template <typename T>
inline int cond_upload(alfi_level* L, const T** dst, const std::vector<T>& src) {
  T* d = nullptr;
  ALFI_CHECK(dev_upload(L->ctx, &d, src.data(), (int64_t)src.size()));
  L->cond_allocs.push_back(d);
  *dst = d;
  return 0;
}

// api_ctx.hip
int check_dev_err(alfi_ctx* ctx);      // the sticky device-side error word (bounded waits of persistent kernels), read after a sync
int build_chunk_tables(alfi_ctx* ctx, DevBSR* d, const int32_t* rowptr, int64_t nbrows, int64_t break_row,
                       int64_t* nchunks_before = nullptr);
int upload_bsr(alfi_ctx* ctx, DevBSR* d, const alfi_bsr_host* h, int bs);
void free_bsr(DevBSR* d);
void free_cond(alfi_level* L);
int comm_allreduce(alfi_level* L, int64_t offset, int64_t count);
int halo_fwd(alfi_level* L, double* v);
int halo_fwd_begin(alfi_level* L, const double* v);
int halo_fwd_end(alfi_level* L, double* v);
int halo_rev(alfi_level* L, double* v);
int halo_sum(alfi_level* L, double* v);
int halo_rev_begin(alfi_level* L, const double* v);
int halo_rev_end(alfi_level* L, double* v);
// api_level.hip
void free_assembly(AssemblyDev* S);
int level_spmv(alfi_level* L, const double* dx, double* dy, const double* db, int mode, bool ghosts_current = false);
int level_patch_apply(alfi_level* L, const double* dx, double* dy, bool* ghosts_current = nullptr);
// the level has what its preconditioner application needs: factored patches, or the point-Jacobi switch
inline bool level_pc_ready(const alfi_level* L) { return L->factored || L->jacobi; }
// the entry points that exist on serial levels only (Chebyshev smoother, W-cycle, CG, Arnoldi, point Jacobi)
inline bool level_is_partitioned(const alfi_level* L) { return L->distributed || L->has_halo || L->n_own != L->n; }
// ---- the state of a level's patch factors (common.h: store_req, held, cond_by) ------------------------------------------------
// the only writer of `held`, and of `cond` with it
inline void set_held(alfi_level* L, PatchStoreHeld h) {
  L->held = h;
  L->cond = h == HELD_COND;
}
inline bool wants_f32(const alfi_level* L) { return L->store_req != STORE_REQ_F64; }               // the next factorisation
inline bool is_or_will_be_f32(const alfi_level* L) { return wants_f32(L) || L->held == HELD_F32; }
inline bool cond_by_caller(const alfi_level* L) { return L->cond && L->cond_by == COND_BY_CALLER; }
inline bool cond_by_own_choice(const alfi_level* L) { return L->cond && L->cond_by == COND_BY_LIBRARY; }
// PCPATCH's facet rule changes the patch matrices of this level
inline bool facet_rule_active(const alfi_level* L) { return L->fc_ptr && L->fc_scale != 0.0; }
// api_patches.hip
// every factor storage of the level -- dense FP64, interleaved copy, FP32, condensed -- and the requests that go with a patch
// set; the ctx's FP64 work buffer goes with its last FP32 level.  Callers have synchronised the stream.
void free_patch_factors(alfi_level* L);
void free_mult_schedule(alfi_level* L);
// a level that condensed itself goes back to dense inverses for good (api_patches.hip); true: it was factored, factor it again
bool auto_cond_to_dense(alfi_level* L);
// api_smoother.hip
int ensure_fgmres_workspace(alfi_level* L, int k);
int ensure_cheb_workspace(alfi_level* L);
bool smoother_takes_fused_iteration(const alfi_level* L, int k, bool* flat_spmv = nullptr);   // alfi_smooth_fgmres on this level
// The general path of the FGMRES(k) smoother on the 1 .. BLOCK_NV columns `cols` of B and X, slot s of ws for column cols.c[s]:
// alfi_smooth_fgmres with one column on L->ws, the lockstep mode of alfi_smooth_fgmres_block on L->blk_ws.  Unchecked.
int smooth_fgmres_general(alfi_level* L, const KrylovWs& ws, int k, const BlockCols& cols, const double* B, int64_t ldb, double* X,
                          int64_t ldx, int nonzero_guess);
// api_block.hip: the two workspace types of krylov_ws.h on the device.  Whoever changes a workspace synchronises the stream,
// frees, allocates and zeroes (hs; a slot buffer whole) here and nowhere else.
// ws becomes `slots` workspaces of FGMRES(K) for vectors of n entries (ldv = krylov_ldv(n)); nothing happens if it is that already
int krylov_ws_ensure(alfi_ctx* ctx, KrylovWs* ws, int slots, int K, int64_t n);
void krylov_ws_release(KrylovWs* ws);
// buf serves a chunk of ncol columns of `per` doubles each (grow-only: slot_buf_needed) / holds exactly `slots` of them
int slot_buf_ensure(alfi_ctx* ctx, SlotBuf* buf, int ncol, int64_t per);
int slot_buf_resize(alfi_ctx* ctx, SlotBuf* buf, int slots, int64_t per);
void slot_buf_release(SlotBuf* buf);
// Lifetime of every workspace of the two types.  Callers have synchronised the stream.
void block_release_patch_buffers(alfi_level* L);   // what a new patch set invalidates: the buffers sized by the old one
void release_workspaces(alfi_level* L);            // all of a level's (alfi_level_destroy)
void release_workspaces(alfi_saddle* S);           // all of a saddle's (alfi_saddle_destroy)
// the block forms on one chunk of 1 .. 4 columns, arguments unchecked: entry i of ic names the column that is read (X, B), entry
// i of oc the column its result goes to (block_patch_apply, block_spmv); the smoother works on the columns cols of B and X
struct BlockCols;
struct BlockOperand {      // a column-major operand of a block call
  const double* p;
  int64_t ld;
  bool written;
};
// ALFI_E_ARG unless L is a serial level, (ncol, cols, nx) a column list, every operand non-NULL with an even leading dimension
// >= L->n, and no written operand overlaps another one
int check_block_call(alfi_level* L, const char* what, int ncol, const int* cols, int nx, const BlockOperand* ops, int nops);
int check_block_operands(alfi_ctx* ctx, const char* what, int64_t n, int ncol, const int* cols, int nx, const BlockOperand* ops,
                         int nops);
// api_cycles.hip: one full cycle on the columns `cols` of B and X, unchecked
int mg_fcycle_block_chunk(alfi_mg* mg, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx);
int block_patch_apply(alfi_level* L, const BlockCols& ic, const BlockCols& oc, const double* X, int64_t ldx, double* Y, int64_t ldy);
int block_spmv(alfi_level* L, const BlockCols& ic, const BlockCols& oc, const double* X, int64_t ldx, double* Y, int64_t ldy,
               const double* B, int64_t ldb, int mode);
int block_smooth_fgmres(alfi_level* L, int k, const BlockCols& cols, const double* B, int64_t ldb, double* X, int64_t ldx,
                        int nonzero_guess);
// api_saddle.hip
int upload_csr(alfi_ctx* ctx, DevCSR* d, const alfi_csr_host* h);
void free_csr(DevCSR* d);
