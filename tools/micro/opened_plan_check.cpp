// opened_plan_check.cpp -- drives himg_amd/csrc/opened_plan.h on the host (tests/test_opened_plan_host.py).
// Input, whitespace separated:
//   H n_streams rows                 a fresh handle
//   C n h chunk  (s x y) x n         a call of n windows of height h; its list cut into entries of `chunk` rows
//   R n h chunk  (s x y) x n         the same call refused by its checks: planned, nothing marked
// Output per call: "n_list list_rows counted" and the list's entries "s a b", all on one line.
#include <cstdio>
#include <vector>

#include "opened_plan.h"

int main() {
  himg_dev::OpenedRows rows;
  char op;
  while (std::scanf(" %c", &op) == 1) {
    if (op == 'H') {
      int n_streams, nrows;
      if (std::scanf("%d %d", &n_streams, &nrows) != 2) return 2;
      rows.reset(n_streams, nrows);
      continue;
    }
    if (op != 'C' && op != 'R') return 2;
    int n, h, chunk;
    if (std::scanf("%d %d %d", &n, &h, &chunk) != 3 || n < 1) return 2;
    std::vector<int32_t> so((size_t)n), org(2 * (size_t)n);
    for (int k = 0; k < n; ++k)
      if (std::scanf("%d %d %d", &so[k], &org[2 * k], &org[2 * k + 1]) != 3) return 2;
    std::vector<himg_dev::OpenedRun> runs;
    const long long list_rows = rows.pending(so.data(), org.data(), n, h, &runs);
    std::vector<uint32_t> list;
    himg_dev::opened_cut(runs, chunk, &list);
    if (op == 'C') rows.mark(runs);
    std::printf("%zu %lld %lld", list.size() / 3, list_rows, rows.counted());
    for (size_t i = 0; i < list.size(); ++i) std::printf(" %u", list[i]);
    std::printf("\n");
  }
  return 0;
}
