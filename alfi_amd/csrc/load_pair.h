// One aligned 16-byte load of a pair of doubles: what the applies of the interleaved copy of the small-patch inverses read with
// (kernels_patch.hip, kernels_block_fused.hip).  Moved here verbatim from kernels_patch.hip.
#pragma once
#include <hip/hip_runtime.h>

typedef double alfi_d2 __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ double2 load_pair(const double* p) {   // one aligned 16-byte load
  const alfi_d2* q = reinterpret_cast<const alfi_d2*>(p);
  const alfi_d2 v = NT ? __builtin_nontemporal_load(q) : *q;
  return make_double2(v.x, v.y);
}
