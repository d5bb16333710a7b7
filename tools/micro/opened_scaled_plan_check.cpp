// opened_scaled_plan_check.cpp -- himg_amd/csrc/opened_plan.h fed the windows of a SCALED call on an
// opened-streams handle (tests/test_opened_scaled_host.py).  A window w x h at (x, y) of the picture at scale
// 2^-sl enters OpenedRows::pending as the full-resolution rectangle it covers, R^: origin (F x, F y), height F h,
// F = 2^sl (sl = 0: a full-resolution window as it is) -- the mapping of himg_hip.hip's opened_launch.
// Input, whitespace separated:
//   H n_streams rows             a fresh handle
//   C sl n h  (s x y) x n        a call of n windows of height h at scale 2^-sl, planned and marked
// Output per call: "list_rows counted" and the runs "s a b", all on one line.
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
    if (op != 'C') return 2;
    int sl, n, h;
    if (std::scanf("%d %d %d", &sl, &n, &h) != 3 || n < 1 || sl < 0 || sl > 2) return 2;
    const int F = 1 << sl;
    std::vector<int32_t> so((size_t)n), org(2 * (size_t)n);
    for (int k = 0; k < n; ++k) {
      int x, y;
      if (std::scanf("%d %d %d", &so[k], &x, &y) != 3) return 2;
      org[2 * k] = F * x; org[2 * k + 1] = F * y;
    }
    std::vector<himg_dev::OpenedRun> runs;
    const long long list_rows = rows.pending(so.data(), org.data(), n, F * h, &runs);
    rows.mark(runs);
    std::printf("%lld %lld", list_rows, rows.counted());
    for (const himg_dev::OpenedRun &u : runs) std::printf(" %d %d %d", u.s, u.a, u.b);
    std::printf("\n");
  }
  return 0;
}
