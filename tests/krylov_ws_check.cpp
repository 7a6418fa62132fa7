// Stand-alone check of csrc/krylov_ws.h under host sanitizers (tests/test_krylov_ws.py builds and runs it; nothing is loaded into
// Python).  For slots 1..4, K in {1, 2, 15, 30}, n in {1, 2, 7}: the four arrays are malloc'ed at the sizes the header reports,
// the first and the last entry of every v(s, j), z(s, j), wv(s), h(s) are written (AddressSanitizer sees an overrun), no two
// regions overlap, and the strides are the formulas the drivers used to spell out -- restated long-hand here.  Then the slot
// buffer's grow rule against block_slots_needed for every (have, ncol) in 0..4 x 1..9.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "krylov_ws.h"

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
      ++fails;                                                    \
    }                                                             \
  } while (0)

// the Hessenberg array of FGMRES(K), long-hand (hs_layout.h): 8 scalars, K columns of K + 1, cosines, sines, K + 1 rotated
// right-hand side entries, y, K + 1 dots
static int64_t hs_total(int K) { return 8 + (int64_t)K * (K + 1) + K + K + (K + 1) + K + (K + 1); }

int main() {
  int cases = 0;
  for (int slots = 1; slots <= 4; ++slots)
    for (int K : {1, 2, 15, 30})
      for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)7}) {
        const int64_t ldv = krylov_ldv(n);
        CHECK(ldv == (n % 2 ? n + 1 : n) && ldv >= n && ldv % 2 == 0);
        const KrylovWsDoubles d = krylov_ws_doubles(slots, K, ldv);
        CHECK(d.V == (int64_t)slots * (K + 1) * ldv);
        CHECK(d.Z == (int64_t)slots * K * ldv);
        CHECK(d.w == (int64_t)slots * ldv);
        CHECK(d.hs == (int64_t)slots * hs_total(K));
        KrylovWs ws;
        ws.V = (double*)std::malloc(sizeof(double) * d.V);
        ws.Z = (double*)std::malloc(sizeof(double) * d.Z);
        ws.w = (double*)std::malloc(sizeof(double) * d.w);
        ws.hs = (double*)std::malloc(sizeof(double) * d.hs);
        ws.K = K;
        ws.slots = slots;
        ws.ldv = ldv;
        CHECK(ws.vs() == (int64_t)(K + 1) * ldv && ws.zs() == (int64_t)K * ldv && ws.hstride() == hs_total(K));
        CHECK(HsLayout(K).total == hs_total(K));
        std::vector<std::pair<double*, double*>> regions;      // [first, last] of every vector
        auto touch = [&](double* p, int64_t len) {
          p[0] = 1.0;
          p[len - 1] = 2.0;
          regions.push_back({p, p + len - 1});
        };
        for (int s = 0; s < slots; ++s) {
          for (int j = 0; j <= K; ++j) {
            CHECK(ws.v(s, j) == ws.V + (int64_t)s * (K + 1) * ldv + (int64_t)j * ldv);
            touch(ws.v(s, j), n);
          }
          for (int j = 0; j < K; ++j) {
            CHECK(ws.z(s, j) == ws.Z + (int64_t)s * K * ldv + (int64_t)j * ldv);
            touch(ws.z(s, j), n);
          }
          CHECK(ws.wv(s) == ws.w + (int64_t)s * ldv);
          touch(ws.wv(s), n);
          CHECK(ws.h(s) == ws.hs + (int64_t)s * hs_total(K));
          touch(ws.h(s), hs_total(K));
        }
        std::sort(regions.begin(), regions.end());
        for (size_t i = 1; i < regions.size(); ++i) CHECK(regions[i - 1].second < regions[i].first);
        CHECK((int)regions.size() == slots * (2 * K + 3));
        std::free(ws.V);
        std::free(ws.Z);
        std::free(ws.w);
        std::free(ws.hs);
        ++cases;
      }
  // the slot buffer: grow-only, at most one chunk, and slot s starts s * per doubles in
  for (int have = 0; have <= 4; ++have)
    for (int ncol = 1; ncol <= 9; ++ncol) {
      SlotBuf b;
      b.slots = have;
      b.per = 5;
      const int need = slot_buf_needed(b, ncol);
      CHECK(need == block_slots_needed(have, ncol));
      CHECK(need == std::max(have, std::min(ncol, 4)));
      std::vector<double> mem((size_t)need * b.per);
      b.p = mem.data();
      for (int s = 0; s < need; ++s) {
        CHECK(b.slot(s) == b.p + (int64_t)s * b.per);
        b.slot(s)[0] = b.slot(s)[b.per - 1] = 3.0;
      }
      ++cases;
    }
  if (fails) return 1;
  std::printf("OK %d cases\n", cases);
  return 0;
}
