// The two kinds of lazily allocated device workspace of the host drivers: the arithmetic of their layout.  Host only, no HIP (as
// block_cols.h): the api_*.hip files include it, and so can a stand-alone program built with host sanitizers.  Allocation and
// lifetime: krylov_ws_ensure / _release, slot_buf_ensure / _resize / _release (api_internal.h, api_block.hip).
#pragma once
#include <cstdint>
#include "block_cols.h"
#include "hs_layout.h"

// stride of Krylov vectors of n entries: n rounded up to even, so that every basis vector starts on a 16-byte boundary (the
// BLAS-1 kernels read entry pairs; n = 3 x nodes is odd on half of the 3-D levels)
inline int64_t krylov_ldv(int64_t n) { return (n + 1) & ~(int64_t)1; }

// `slots` FGMRES(K) workspaces for vectors of stride ldv, each array ONE allocation, so that the Krylov vectors of the slots
// are the columns of a block operand: v_j of slot s at V + s * (K + 1) * ldv + j * ldv (j <= K), z_j at Z + s * K * ldv + j * ldv
// (j < K), the work vector at w + s * ldv, the Hessenberg data (hs_layout.h) at hs + s * HsLayout(K).total.  The single call's
// workspace is the one-slot case; a slot of a block call belongs to one column of its chunk.
struct KrylovWs {
  double *V = nullptr, *Z = nullptr, *w = nullptr, *hs = nullptr;
  int K = 0, slots = 0;      // (0, 0: not allocated)
  int64_t ldv = 0;
  int64_t vs() const { return (int64_t)(K + 1) * ldv; }      // between two slots' bases
  int64_t zs() const { return (int64_t)K * ldv; }
  int64_t hstride() const { return HsLayout(K).total; }
  double* v(int s, int j) const { return V + s * vs() + j * ldv; }
  double* z(int s, int j) const { return Z + s * zs() + j * ldv; }
  double* wv(int s) const { return w + s * ldv; }
  double* h(int s) const { return hs + s * hstride(); }
};
// doubles of the four allocations
struct KrylovWsDoubles {
  int64_t V, Z, w, hs;
};
inline KrylovWsDoubles krylov_ws_doubles(int slots, int K, int64_t ldv) {
  KrylovWs t;
  t.K = K;
  t.ldv = ldv;
  return {slots * t.vs(), slots * t.zs(), slots * ldv, slots * t.hstride()};
}

// `slots` column slots of `per` doubles each (0 slots: not allocated).  `per` is fixed while the buffer lives.
struct SlotBuf {
  double* p = nullptr;
  int slots = 0;
  int64_t per = 0;
  double* slot(int s) const { return p + s * per; }
};
// the slots a buffer has to hold to serve a call of ncol columns: the one grow rule of block_cols.h
inline int slot_buf_needed(const SlotBuf& b, int ncol) { return block_slots_needed(b.slots, ncol); }
