"""The search of an encode to a distortion target (include/himg_hip.h, "encode to a distortion
target"), as a model for the tests: a dozen lines that share nothing with the product; and the
distortion itself in int64 numpy."""
import numpy as np


def search(sse_of_q, target, qmin, qmax):
    """(quality or -1, [probed qualities]) for a frame whose exact distortion at quality q is
    sse_of_q(q): qmax must meet the target; qmin wins if it meets it; else bisect with hi meeting
    it, lo not."""
    probes = [qmax]
    if sse_of_q(qmax) > target:
        return -1, probes
    if qmin == qmax:
        return qmax, probes
    probes.append(qmin)
    if sse_of_q(qmin) <= target:
        return qmin, probes
    lo, hi = qmin, qmax
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        probes.append(mid)
        if sse_of_q(mid) <= target:
            hi = mid
        else:
            lo = mid
    return hi, probes


def sse(img, dec):
    """The sum of the squared differences of two uint8 pictures of one shape, an exact Python int."""
    d = np.asarray(img, np.int64) - np.asarray(dec, np.int64)
    return int((d * d).sum())


def inversions(sses):
    """The qualities q with sses[q + 1] > sses[q] (sses: a sequence indexed by quality)."""
    return [q for q in range(len(sses) - 1) if sses[q + 1] > sses[q]]
