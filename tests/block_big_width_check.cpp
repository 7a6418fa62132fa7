// Stand-alone check of the host-only arithmetic that decides how a level of dense macro-star inverses batches block right-hand
// sides: the width rule block_big_lds / block_big_width (csrc/block_cols.h), the work split big_split that the single and the
// block launcher share (csrc/patch_plan.h) and the cutting of a chunk into pieces.  Built and run by tests/test_block_rhs_macro.py
// with -fsanitize=address,undefined (host code only; never loaded into Python, never on a GPU):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I alfi_amd/csrc tests/block_big_width_check.cpp
// Every list lives in a heap block of exactly its length, so that a read past the end of `cols` is an error the sanitizer
// sees.  Prints "OK <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "patch_plan.h"
#include "block_cols.h"

static long checks = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    ++checks;                                                           \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

int main() {
  // LDS of a workgroup: nv x 8 bytes x the largest patch rounded up to even
  CHECK(block_big_lds(161, 1) == 8 * 162 && block_big_lds(162, 1) == 8 * 162 && block_big_lds(2175, 3) == 3 * 8 * 2176);
  CHECK(block_big_lds(4096, 4) == 131072 && block_big_lds(2048, 4) == 65536 && block_big_lds(512, 1) == 4096);
  // the width at the default budget of 64 KiB
  const int64_t def = 64 * 1024;
  const struct { int max_np, width; } at_default[] = {{160, 4}, {161, 4}, {2048, 4}, {2049, 3}, {2730, 3}, {2731, 2}, {4096, 2}};
  for (const auto& t : at_default) CHECK(block_big_width(t.max_np, def) == t.width);
  CHECK(block_big_width(2175, def) == 3 && block_big_width(2175, 69632) == 4);      // config 5's macro stars
  // budgets of 0, exactly nv x lds, one byte less
  const int sizes[] = {160, 161, 512, 2047, 2048, 2049, 2730, 2731, 4095, 4096};
  for (int m : sizes) {
    const int64_t one = block_big_lds(m, 1);
    CHECK(block_big_width(m, 0) == 0);
    CHECK(block_big_width(m, -1) == 0);
    CHECK(block_big_width(m, one) == 0);                          // one column fits: no batch
    CHECK(block_big_width(m, 2 * one - 1) == 0);
    CHECK(block_big_width(m, 2 * one) == 2);
    CHECK(block_big_width(m, 3 * one - 1) == 2);
    CHECK(block_big_width(m, 3 * one) == 3);
    CHECK(block_big_width(m, 4 * one - 1) == 3);
    CHECK(block_big_width(m, 4 * one) == 4);
    CHECK(block_big_width(m, 100 * one) == 4);                    // never wider than a chunk
    for (int nv = 1; nv <= BLOCK_NV; ++nv) CHECK(block_big_lds(m, nv) == nv * one && one % 16 == 0);
  }
  CHECK(block_big_width(0, def) == 0 && block_big_width(-3, def) == 0);      // no patches: no batch
  CHECK(BIG_BLOCK_MIN_PATCHES == 8);

  // workgroups per patch (the function both launchers read): levels of the issue's table and configs 5 / 5L
  CHECK(big_split(12, 2048) == 4 && big_split(27, 1599) == 4 && big_split(303, 1941) == 4);
  CHECK(big_split(1765, 2175) == 2 && big_split(5000, 4096) == 1);
  CHECK(big_split(12, 512) == 1 && big_split(8, 641) == 2 && big_split(8, 1155) == 3 && big_split(8, 2049) == 5 && big_split(8, 2731) == 6);
  for (int64_t np = 1; np <= 5000; np += 7)
    for (int m = 1; m <= PATCH_MAX; m += 61) {
      const int s = big_split(np, m);
      CHECK(s >= 1 && 4 * (s - 1) < (m + 127) / 128 + 3);          // no more waves than 128-row pieces (rounded up to a workgroup)
    }

  // pieces of 1 .. 9 columns at every width: every column exactly once, in order
  for (int ncol = 1; ncol <= 9; ++ncol) {
    std::unique_ptr<int[]> cols(new int[ncol]);
    for (int i = 0; i < ncol; ++i) cols[i] = (5 * i + 2) % 11;      // distinct: 5 is a unit mod 11
    for (int width = 0; width <= BLOCK_NV; ++width) {
      const int w = width < 1 ? 1 : width;
      std::vector<int> seen;
      for (int q = 0; q < block_chunks(ncol); ++q) {
        const BlockCols ch = block_chunk(ncol, cols.get(), q);
        for (int k = 0; k < block_pieces(ch.n, width); ++k) {
          const BlockCols pc = block_piece(ch, width, k);
          CHECK(pc.n >= 1 && pc.n <= w);
          CHECK(k + 1 < block_pieces(ch.n, width) ? pc.n == w : pc.n == ch.n - w * k);
          for (int i = 0; i < BLOCK_NV; ++i) CHECK(pc.c[i] == (i < pc.n ? ch.c[w * k + i] : pc.c[0]));
          for (int i = 0; i < pc.n; ++i) seen.push_back(pc.c[i]);
        }
      }
      CHECK((int)seen.size() == ncol);
      for (int i = 0; i < ncol; ++i) CHECK(seen[i] == cols[i]);
    }
  }
  std::printf("OK %ld\n", checks);
  return 0;
}
