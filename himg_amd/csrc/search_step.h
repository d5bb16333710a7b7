// search_step.h -- one frame's step of the encoder's quality searches (encode to a byte budget, encode
// to a distortion target; include/himg_hip.h), as plain C++: k_search_step runs it one lane per frame,
// tools/micro/search_check.cpp on the host.
#ifndef HIMG_SEARCH_STEP_H_
#define HIMG_SEARCH_STEP_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define HIMG_HOST_DEVICE __host__ __device__
#else
#define HIMG_HOST_DEVICE
#endif

namespace himg_dev {

enum { kSearchRunning = 0, kSearchFound = 1, kSearchMissed = 2, kSearchError = 3 };
// Which end of [qmin, qmax] must satisfy the limit, the first probe's: the search returns the quality
// nearest to the OTHER end that satisfies it (as far as a bisection sees).
enum { kSearchFromMin = 0,    // a byte budget: size(qmin) must fit, the largest fitting quality wins
       kSearchFromMax = 1 };  // a distortion target: sse(qmax) must meet it, the smallest such quality wins

struct SearchFrame {
  int32_t quality;       // the next probe; of a settled frame its result (qmin without one): what the final encode takes
  uint64_t limit;        // the largest value that satisfies
  uint64_t best;         // the value at `ok` (a frame that misses: at the first probe's end)
  int32_t ok, bad;       // the bound known to satisfy the limit / known not to
  int32_t state, err;    // kSearch*; a probe's own failure status, kept through the later probes
};

// Behind probe `probe` of a frame -- 0: at the end that must satisfy, 1: at the far end, then at the
// midpoint (ok + bad) >> 1 that the step before chose -- whose status and value are `status` and
// `value`.  Probe 0 sets the frame up (only `limit` is read).  A settled frame stays as it is: its
// later probes repeat at its result.
HIMG_HOST_DEVICE inline void search_step(SearchFrame &s, int probe, int dir, int qmin, int qmax, int32_t status,
                                         uint64_t value) {
  const int first = dir == kSearchFromMin ? qmin : qmax, far = dir == kSearchFromMin ? qmax : qmin;
  if (probe == 0) { s.state = kSearchRunning; s.ok = first; s.bad = far; s.err = 0; s.best = 0; }
  if (s.state == kSearchRunning) {
    const bool meets = value <= s.limit;
    if (status != 0) { s.state = kSearchError; s.err = status; }
    else if (probe == 0) {
      s.best = value;
      if (!meets) s.state = kSearchMissed;
      else if (qmax == qmin) s.state = kSearchFound;
    } else if (probe == 1) {
      if (meets) { s.ok = far; s.best = value; s.state = kSearchFound; }
    } else {
      const int mid = (s.ok + s.bad) >> 1;   // (what this probe was at)
      if (meets) { s.ok = mid; s.best = value; } else s.bad = mid;
    }
    const int gap = s.bad > s.ok ? s.bad - s.ok : s.ok - s.bad;
    if (s.state == kSearchRunning && probe >= 1 && gap <= 1) s.state = kSearchFound;
  }
  s.quality = s.state == kSearchRunning ? (probe == 0 ? far : (s.ok + s.bad) >> 1)
                                        : (s.state == kSearchFound ? s.ok : qmin);
}

// What the last step reports as the frame's quality.
HIMG_HOST_DEVICE inline int32_t search_result(const SearchFrame &s) { return s.state == kSearchFound ? s.ok : -1; }

}  // namespace himg_dev
#endif  // HIMG_SEARCH_STEP_H_
