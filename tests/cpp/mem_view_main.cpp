// Stand-alone driver of csrc/mem_view.h's arithmetic layer for tests/test_mem_view.py (built
// with -fsanitize=address,undefined).
//   "sweep": every log_cap in 1..12, rl_capacity in 1..log_cap and rl_total in 0..5 log_cap
//            against brute force; prints how many combinations fell into each case.
//   "big":   the same check at rl_total near 2^40 with log_cap 200,000 + 4 x 65,536.
//   "window <rl_total> <rl_capacity> <log_cap>": prints the window, for the test to judge.
// The first violation is printed and the exit status is 1.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mem_view.h"

using namespace nfsp::mem;

enum { NOT_FULL, FULL_ONE_PIECE, ENDS_ON_LAST_ROW, WRAPPED, N_CASES };
static const char* const CASE_NAME[N_CASES] = {"not_full", "full_one_piece", "ends_on_last_row", "wrapped"};

// the window of (rl_total, rl_capacity, log_cap) against rows k % log_cap, k in [rl_total - live,
// rl_total), in that order; returns its case, or -1 after printing what is wrong
static int check(int64_t rl_total, int64_t rl_capacity, int64_t log_cap) {
  const int64_t live = live_count(rl_total, rl_capacity);
  const Window w = log_window(rl_total, live, log_cap);
  auto wrong = [&](const char* what) {
    printf("rl_total %" PRId64 " rl_capacity %" PRId64 " log_cap %" PRId64 ": %s\n", rl_total, rl_capacity, log_cap, what);
    return -1;
  };
  if (live != (rl_total < rl_capacity ? rl_total : rl_capacity)) return wrong("live count");
  if (w.n < 0 || w.n > 2) return wrong("more than two pieces");
  int64_t sum = 0;
  for (int k = 0; k < w.n; ++k) {
    if (w.len[k] <= 0) return wrong("an empty piece");
    if (w.row[k] < 0 || w.row[k] + w.len[k] > log_cap) return wrong("a piece outside the log");
    sum += w.len[k];
  }
  if (sum != live) return wrong("the pieces' lengths do not sum to the live count");
  int piece = 0;
  int64_t at = 0;
  for (int64_t k = rl_total - live; k < rl_total; ++k) {
    if (w.row[piece] + at != k % log_cap) return wrong("a row out of order");
    if (++at == w.len[piece]) {
      ++piece;
      at = 0;
    }
  }
  if (piece != w.n) return wrong("pieces left over");
  if (rl_total < rl_capacity) return NOT_FULL;
  if (w.n == 2) return WRAPPED;
  return w.row[0] + w.len[0] == log_cap ? ENDS_ON_LAST_ROW : FULL_ONE_PIECE;
}

static int report(const char* name, const int64_t count[N_CASES]) {
  printf("%s ok", name);
  for (int c = 0; c < N_CASES; ++c) printf(" %s=%" PRId64, CASE_NAME[c], count[c]);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  int64_t count[N_CASES] = {0, 0, 0, 0};
  if (argc == 2 && !strcmp(argv[1], "sweep")) {
    for (int64_t log_cap = 1; log_cap <= 12; ++log_cap)
      for (int64_t cap = 1; cap <= log_cap; ++cap)
        for (int64_t total = 0; total <= 5 * log_cap; ++total) {
          const int c = check(total, cap, log_cap);
          if (c < 0) return 1;
          ++count[c];
        }
    return report("sweep", count);
  }
  if (argc == 2 && !strcmp(argv[1], "big")) {
    const int64_t cap = 200000, log_cap = cap + 4 * 65536;
    const int64_t k0 = ((int64_t)1 << 40) / log_cap * log_cap;     // record k0 lies at row 0
    // windows that end at rows 1, cap - 1, cap (the first without a wrap), cap + 1, log_cap - 1
    // and log_cap (exactly on the last row), and 2^40 itself
    const int64_t ends[] = {1, cap - 1, cap, cap + 1, log_cap - 1, log_cap};
    for (int64_t end : ends) {
      const int c = check(k0 + end, cap, log_cap);
      if (c < 0) return 1;
      ++count[c];
    }
    if (check((int64_t)1 << 40, cap, log_cap) < 0) return 1;
    return report("big", count);
  }
  if (argc == 5 && !strcmp(argv[1], "window")) {
    const int64_t total = atoll(argv[2]), cap = atoll(argv[3]), log_cap = atoll(argv[4]);
    const int64_t live = live_count(total, cap);
    const Window w = log_window(total, live, log_cap);
    printf("live %" PRId64 " pieces", live);
    for (int k = 0; k < w.n; ++k) printf(" %" PRId64 ":%" PRId64, w.row[k], w.len[k]);
    printf("\n");
    return 0;
  }
  fprintf(stderr, "usage: mem_view_main sweep | big | window <rl_total> <rl_capacity> <log_cap>\n");
  return 2;
}
