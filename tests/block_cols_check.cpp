// Stand-alone check of csrc/block_cols.h, the host-only arithmetic of block right-hand sides: operand validation, the overlap
// test, chunking of column lists and the grow-only slot count of the lazily allocated workspaces.  Built and run by
// tests/test_block_rhs.py with -fsanitize=address,undefined (host code only; never loaded into Python, never on a GPU):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I alfi_amd/csrc tests/block_cols_check.cpp
// Every list lives in a heap block of exactly its length, so that a read past the end of `cols` is an error the sanitizer
// sees.  Prints "OK <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  // chunking: every column exactly once, in order, chunks of BLOCK_NV and a shorter last one; unused slots name a listed column
  for (int ncol = 1; ncol <= 23; ++ncol) {
    for (int with_list = 0; with_list < 2; ++with_list) {
      std::unique_ptr<int[]> cols(with_list ? new int[ncol] : nullptr);
      for (int i = 0; with_list && i < ncol; ++i) cols[i] = (7 * i + 3) % 29;       // distinct: 7 is a unit mod 29
      const int nx = with_list ? 29 : ncol;
      CHECK(block_operand_error(100, ncol, cols.get(), nx, 100) == nullptr);
      CHECK(block_chunks(ncol) == (ncol + BLOCK_NV - 1) / BLOCK_NV);
      std::vector<int> seen;
      for (int k = 0; k < block_chunks(ncol); ++k) {
        const BlockCols b = block_chunk(ncol, cols.get(), k);
        CHECK(b.n >= 1 && b.n <= BLOCK_NV);
        CHECK(k + 1 < block_chunks(ncol) ? b.n == BLOCK_NV : b.n == ncol - BLOCK_NV * k);
        for (int i = 0; i < BLOCK_NV; ++i) {
          CHECK(b.c[i] >= 0 && b.c[i] < nx);
          if (i < b.n) seen.push_back(b.c[i]);
          else CHECK(b.c[i] == b.c[0]);
        }
      }
      CHECK((int)seen.size() == ncol);
      for (int i = 0; i < ncol; ++i) CHECK(seen[i] == (with_list ? cols[i] : i));
      CHECK(block_chunk(ncol, cols.get(), block_chunks(ncol)).n == 0);              // past the last chunk: empty, no read
    }
  }
  // validation
  {
    std::unique_ptr<int[]> c(new int[3]{0, 2, 3});
    CHECK(block_operand_error(288, 3, c.get(), 4, 294) == nullptr);
    CHECK(block_operand_error(288, 0, c.get(), 4, 288) != nullptr);                 // ncol < 1
    CHECK(block_operand_error(288, -1, nullptr, 4, 288) != nullptr);
    CHECK(block_operand_error(288, 3, c.get(), 2, 288) != nullptr);                 // more columns than the operand has
    CHECK(block_operand_error(288, 3, c.get(), 4, 289) != nullptr);                 // odd
    CHECK(block_operand_error(288, 3, c.get(), 4, 286) != nullptr);                 // below n
    CHECK(block_operand_error(287, 3, c.get(), 4, 288) == nullptr);                 // odd n, even ld
    CHECK(block_operand_error(288, 3, c.get(), 3, 288) != nullptr);                 // index 3 of 3
    c[1] = -1;
    CHECK(block_operand_error(288, 3, c.get(), 4, 288) != nullptr);
    c[1] = 3;
    CHECK(block_operand_error(288, 3, c.get(), 4, 288) != nullptr);                 // listed twice
    CHECK(std::strcmp(block_operand_error(288, 3, c.get(), 4, 288), "column listed twice") == 0);
  }
  // overlap of column-major operands (addresses only: nothing is dereferenced)
  {
    std::vector<double> buf(4 * 300 + 8);
    double* X = buf.data();
    CHECK(block_operands_overlap(X, 300, X, 300, 4, 288));
    CHECK(block_operands_overlap(X, 300, X + 3 * 300 + 287, 300, 4, 288));          // the last entry of X is the first of Y
    CHECK(!block_operands_overlap(X, 300, X + 3 * 300 + 288, 300, 4, 288));
    CHECK(!block_operands_overlap(X, 300, X + 288, 300, 1, 288));
    CHECK(!block_operands_overlap(X, 300, X, 300, 0, 288) && !block_operands_overlap(X, 300, X, 300, 4, 0));
    CHECK(block_operands_overlap(X + 10, 300, X, 300, 2, 288));
  }
  // workspaces: grow-only, one chunk at the most, never fewer slots than the call's columns of one chunk
  {
    int have = 0;
    const int calls[] = {1, 3, 2, 5, 1, 4, 100};
    const int want[] = {1, 3, 3, 4, 4, 4, 4};
    for (int i = 0; i < 7; ++i) {
      const int need = block_slots_needed(have, calls[i]);
      CHECK(need == want[i] && need >= have && need <= BLOCK_NV);
      for (int k = 0; k < block_chunks(calls[i]); ++k) CHECK(block_chunk(calls[i], nullptr, k).n <= need);
      std::unique_ptr<double[]> ws(new double[(size_t)need * 6]);                    // slot s of the workspace: [6 s, 6 s + 6)
      for (int k = 0; k < block_chunks(calls[i]); ++k)
        for (int s = 0; s < block_chunk(calls[i], nullptr, k).n; ++s) ws[(size_t)s * 6 + 5] = 1.0;
      have = need;
    }
  }
  std::printf("OK %ld\n", checks);
  return 0;
}
