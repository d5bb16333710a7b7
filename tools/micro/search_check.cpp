// search_check.cpp -- the encoder's quality search (himg_amd/csrc/search_step.h) driven on the host
// the way the device entry points drive k_search_step: a fixed number of probes, each at the quality
// the step before left, then the result.  No GPU, no HIP: g++ -std=c++11 -I himg_amd/csrc.
//
// stdin, line by line:
//   C v0 v1 ... v100            define the next curve (its index counts from 0): the value at every quality
//   S dir qmin qmax limit curve run a search: dir 0 = the first probe at qmin (a byte budget),
//                               1 = at qmax (a distortion target)
// stdout, a line per S: the result (-1: none), then the qualities probed while the frame was unsettled.
#include <stdint.h>
#include <stdio.h>

#include <array>
#include <vector>

#include "search_step.h"

// himg_hip_budget_probes (include/himg_hip.h).
static int probe_count(int qmin, int qmax) {
  int n = qmin == qmax ? 1 : 2;
  for (int d = qmax - qmin; d > 1; d = (d + 1) >> 1) ++n;
  return n;
}

int main() {
  std::vector<std::array<uint64_t, 101>> curves;
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'C') {
      std::array<uint64_t, 101> c;
      for (uint64_t &v : c) {
        unsigned long long x;
        if (scanf("%llu", &x) != 1) return 2;
        v = x;
      }
      curves.push_back(c);
    } else if (kind == 'S') {
      int dir, qmin, qmax;
      unsigned long long limit;
      size_t ci;
      if (scanf("%d %d %d %llu %zu", &dir, &qmin, &qmax, &limit, &ci) != 5) return 2;
      if ((dir != 0 && dir != 1) || qmin < 0 || qmax > 100 || qmin > qmax || ci >= curves.size()) return 2;
      himg_dev::SearchFrame s = {};
      s.limit = limit;
      s.quality = dir == himg_dev::kSearchFromMin ? qmin : qmax;   // (what the host stages in front of the first probe)
      std::vector<int> probed;
      const int probes = probe_count(qmin, qmax);
      for (int p = 0; p < probes; ++p) {
        if (s.quality < qmin || s.quality > qmax) return 3;   // a probe outside the range
        if (p == 0 || s.state == himg_dev::kSearchRunning) probed.push_back(s.quality);
        himg_dev::search_step(s, p, dir, qmin, qmax, 0, curves[ci][(size_t)s.quality]);
      }
      if (s.state == himg_dev::kSearchRunning) return 4;   // the probe count did not settle the frame
      printf("%d", (int)himg_dev::search_result(s));
      for (int q : probed) printf(" %d", q);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
