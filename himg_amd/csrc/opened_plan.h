// opened_plan.h -- what a call on an opened-streams handle (include/himg_hip.h, himg_hip_opened_regions_device)
// plans on the host, as plain C++: the block rows its windows touch that no earlier call on the handle has
// counted, as the count kernels' list.  himg_hip.hip runs it per call, tools/micro/opened_plan_check.cpp on its
// own.
#ifndef HIMG_OPENED_PLAN_H_
#define HIMG_OPENED_PLAN_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace himg_dev {

struct OpenedRun { int32_t s, a, b; };   // block rows [a, b) of stream s

// The (stream, block row) pairs of a handle whose records a count kernel has been queued for.
class OpenedRows {
 public:
  void reset(int n_streams, int rows) {
    n_streams_ = n_streams; rows_ = rows; counted_ = 0;
    bits_.assign(((size_t)n_streams * (size_t)rows + 63) / 64, 0ull);
  }
  int n_streams() const { return n_streams_; }
  int rows() const { return rows_; }
  long long counted() const { return counted_; }
  bool test(int s, int r) const {
    const size_t i = (size_t)s * (size_t)rows_ + (size_t)r;
    return (bits_[i >> 6] >> (i & 63)) & 1ull;
  }

  // The rows of n windows of height h -- window k: rows [y_k / 8, ceil((y_k + h) / 8)) of stream stream_of[k],
  // y_k = org[2 k + 1], both checked by the caller -- that are not marked, as maximal runs sorted by stream and
  // row: each stream's [r0, r1) merged, the marked rows cut out.  Returns the rows the runs hold.
  long long pending(const int32_t *stream_of, const int32_t *org, int n, int h, std::vector<OpenedRun> *out) const {
    std::vector<OpenedRun> v((size_t)n);
    for (int k = 0; k < n; ++k) v[k] = OpenedRun{stream_of[k], org[2 * k + 1] / 8, (org[2 * k + 1] + h + 7) / 8};
    std::sort(v.begin(), v.end(), [](const OpenedRun &x, const OpenedRun &y) {
      return x.s != y.s ? x.s < y.s : x.a != y.a ? x.a < y.a : x.b < y.b;
    });
    out->clear();
    long long total = 0;
    for (size_t i = 0; i < v.size();) {
      OpenedRun m = v[i++];
      for (; i < v.size() && v[i].s == m.s && v[i].a <= m.b; ++i) m.b = v[i].b > m.b ? v[i].b : m.b;
      for (int r = m.a; r < m.b;) {
        if (test(m.s, r)) { ++r; continue; }
        int e = r + 1;
        while (e < m.b && !test(m.s, e)) ++e;
        out->push_back(OpenedRun{m.s, r, e});
        total += e - r;
        r = e;
      }
    }
    return total;
  }

  void mark(const std::vector<OpenedRun> &runs) {
    for (const OpenedRun &u : runs)
      for (int r = u.a; r < u.b; ++r) {
        const size_t i = (size_t)u.s * (size_t)rows_ + (size_t)r;
        if (!((bits_[i >> 6] >> (i & 63)) & 1ull)) { bits_[i >> 6] |= 1ull << (i & 63); ++counted_; }
      }
  }

 private:
  int n_streams_ = 0, rows_ = 0;
  long long counted_ = 0;
  std::vector<uint64_t> bits_;
};

// The runs as the count kernels' list: (stream, first row, end row) entries of at most `chunk` rows, appended.
inline void opened_cut(const std::vector<OpenedRun> &runs, int chunk, std::vector<uint32_t> *list) {
  for (const OpenedRun &u : runs)
    for (int a = u.a; a < u.b; a += chunk) {
      list->push_back((uint32_t)u.s); list->push_back((uint32_t)a);
      list->push_back((uint32_t)(u.b - a > chunk ? a + chunk : u.b));
    }
}

}  // namespace himg_dev
#endif  // HIMG_OPENED_PLAN_H_
