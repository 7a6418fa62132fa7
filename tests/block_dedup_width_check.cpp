// Stand-alone check of the host-only arithmetic that decides how the de-duplicated level product batches block right-hand sides:
// the width rule block_dedup_lds / block_dedup_width (csrc/block_cols.h) and the cutting of a chunk into pieces.  Built and run by
// tests/test_block_rhs_dedup.py with -fsanitize=address,undefined (host code only; never loaded into Python, never on a GPU):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I alfi_amd/csrc tests/block_dedup_width_check.cpp
// Every list lives in a heap block of exactly its length, so that a read past the end of `cols` is an error the sanitizer
// sees.  Prints "OK <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
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
  // LDS of a workgroup: nv columns x bs doubles per distinct x entry of the fullest group
  CHECK(block_dedup_lds(1, 2, 1) == 16 && block_dedup_lds(1, 3, 1) == 24 && block_dedup_lds(1024, 3, 4) == 98304);
  CHECK(block_dedup_lds(1024, 2, 4) == 65536 && block_dedup_lds(682, 3, 4) == 65472 && block_dedup_lds(683, 3, 4) == 65568);
  CHECK(block_dedup_lds(910, 3, 3) == 65520 && block_dedup_lds(911, 3, 3) == 65592 && block_dedup_lds(1024, 3, 2) == 49152);
  // the width at the default budget of 64 KiB: bs 2 always 4; bs 3: 4 up to 682 distinct columns, 3 up to 910, 2 up to 1024
  const int64_t def = 64 * 1024;
  const struct { int max_uniq, w2, w3; } at_default[] = {{1, 4, 4}, {682, 4, 4}, {683, 4, 3}, {910, 4, 3}, {911, 4, 2}, {1024, 4, 2}};
  for (const auto& t : at_default) {
    CHECK(block_dedup_width(t.max_uniq, 2, def) == t.w2);
    CHECK(block_dedup_width(t.max_uniq, 3, def) == t.w3);
  }
  // budgets of 0, exactly nv x lds, one byte less
  for (int bs = 2; bs <= 3; ++bs)
    for (const auto& t : at_default) {
      const int m = t.max_uniq;
      const int64_t one = block_dedup_lds(m, bs, 1);
      CHECK(one == (int64_t)8 * bs * m);
      CHECK(block_dedup_width(m, bs, 0) == 0);
      CHECK(block_dedup_width(m, bs, -1) == 0);
      CHECK(block_dedup_width(m, bs, one) == 0);                          // one column fits: no batch
      CHECK(block_dedup_width(m, bs, 2 * one - 1) == 0);
      CHECK(block_dedup_width(m, bs, 2 * one) == 2);
      CHECK(block_dedup_width(m, bs, 3 * one - 1) == 2);
      CHECK(block_dedup_width(m, bs, 3 * one) == 3);
      CHECK(block_dedup_width(m, bs, 4 * one - 1) == 3);
      CHECK(block_dedup_width(m, bs, 4 * one) == 4);
      CHECK(block_dedup_width(m, bs, 100 * one) == 4);                    // never wider than a chunk
      for (int nv = 1; nv <= BLOCK_NV; ++nv) CHECK(block_dedup_lds(m, bs, nv) == nv * one);
    }
  CHECK(block_dedup_width(0, 3, def) == 0 && block_dedup_width(-5, 2, def) == 0 && block_dedup_width(100, 0, def) == 0);

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
