// Stand-alone check of the host-only arithmetic that decides how a condensed level batches block right-hand sides
// (csrc/block_cols.h): the width rule block_cond_width and the cutting of a chunk into pieces of that width.  Built and run by
// tests/test_block_rhs_condensed.py with -fsanitize=address,undefined (host code only; never loaded into Python, never on a GPU):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I alfi_amd/csrc tests/block_cond_width_check.cpp
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
  // the width rule: the largest NV of 4, 3, 2 with NV * max(lds_front, lds_back) <= budget; budgets of 0, exactly NV * lds and
  // one byte less; either launch may be the larger one
  const int64_t sizes[] = {8, 1248, 3000, 16384, 16385, 21845, 21846, 32768, 32769, 65536, 153600};
  for (int64_t lds : sizes) {
    for (int swap = 0; swap < 2; ++swap) {
      const int64_t other = lds / 3 + 1, f = swap ? other : lds, b = swap ? lds : other;
      CHECK(block_cond_width(f, b, 0) == 0);
      CHECK(block_cond_width(f, b, -1) == 0);
      CHECK(block_cond_width(f, b, lds) == 0);                    // one column fits: no batch
      CHECK(block_cond_width(f, b, 2 * lds - 1) == 0);
      CHECK(block_cond_width(f, b, 2 * lds) == 2);
      CHECK(block_cond_width(f, b, 3 * lds - 1) == 2);
      CHECK(block_cond_width(f, b, 3 * lds) == 3);
      CHECK(block_cond_width(f, b, 4 * lds - 1) == 3);
      CHECK(block_cond_width(f, b, 4 * lds) == 4);
      CHECK(block_cond_width(f, b, 100 * lds) == 4);              // never wider than a chunk
      const int def = block_cond_width(f, b, 64 * 1024);          // the default budget
      CHECK(def == (4 * lds <= 65536 ? 4 : 3 * lds <= 65536 ? 3 : 2 * lds <= 65536 ? 2 : 0));
    }
  }
  CHECK(block_cond_width(0, 0, 65536) == 0);                      // no plan: no batch
  CHECK(block_cond_width((int64_t)1 << 40, 8, (int64_t)1 << 42) == 4);   // 64-bit products

  // pieces: every column of the chunk exactly once, in order; pieces of the width and a shorter last one; a width below 2 gives
  // pieces of one column; unused slots name a column of the piece
  for (int ncol = 1; ncol <= 9; ++ncol) {
    std::unique_ptr<int[]> cols(new int[ncol]);
    for (int i = 0; i < ncol; ++i) cols[i] = (5 * i + 2) % 11;      // distinct: 5 is a unit mod 11
    for (int width = -1; width <= 6; ++width) {
      const int w = width < 1 ? 1 : width > BLOCK_NV ? BLOCK_NV : width;
      CHECK(block_piece_width(width) == w);
      std::vector<int> seen;
      for (int q = 0; q < block_chunks(ncol); ++q) {
        const BlockCols ch = block_chunk(ncol, cols.get(), q);
        CHECK(block_pieces(ch.n, width) == (ch.n + w - 1) / w);
        for (int k = 0; k < block_pieces(ch.n, width); ++k) {
          const BlockCols pc = block_piece(ch, width, k);
          CHECK(pc.n >= 1 && pc.n <= w);
          CHECK(k + 1 < block_pieces(ch.n, width) ? pc.n == w : pc.n == ch.n - w * k);
          for (int i = 0; i < BLOCK_NV; ++i) CHECK(pc.c[i] == (i < pc.n ? ch.c[w * k + i] : pc.c[0]));
          for (int i = 0; i < pc.n; ++i) seen.push_back(pc.c[i]);
        }
        CHECK(block_piece(ch, width, block_pieces(ch.n, width)).n == 0);     // past the end: an empty piece, valid indices
        CHECK(block_piece(ch, width, -1).n == 0);
      }
      CHECK((int)seen.size() == ncol);
      for (int i = 0; i < ncol; ++i) CHECK(seen[i] == cols[i]);
    }
  }
  CHECK(block_pieces(0, 4) == 0);
  // a width of 3 on a full chunk: 3 + 1; a width of 2: 2 + 2 (the second piece of 3 + 1 is the single-vector path)
  const BlockCols full = block_chunk(4, nullptr, 0);
  CHECK(block_pieces(4, 3) == 2 && block_piece(full, 3, 0).n == 3 && block_piece(full, 3, 1).n == 1 && block_piece(full, 3, 1).c[0] == 3);
  CHECK(block_pieces(4, 2) == 2 && block_piece(full, 2, 1).n == 2 && block_piece(full, 2, 1).c[0] == 2 && block_piece(full, 2, 1).c[1] == 3);
  CHECK(block_pieces(4, 4) == 1 && block_piece(full, 4, 0).n == 4);
  // the slots of a workspace serve the widest piece ever asked for, never more than a chunk
  CHECK(block_slots_needed(0, 3) == 3 && block_slots_needed(3, 2) == 3 && block_slots_needed(3, 4) == 4 && block_slots_needed(2, 9) == 4);
  std::printf("OK %ld\n", checks);
  return 0;
}
