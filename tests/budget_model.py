"""The search of an encode to a byte budget (include/himg_hip.h, "encode to a byte budget"), as a
model for the tests: a dozen lines that share nothing with the product."""


def search(size_of_q, budget, qmin, qmax):
    """(quality or -1, [probed qualities]) for a frame whose exact stream size at quality q is
    size_of_q(q): qmin must fit; qmax wins if it fits; else bisect with lo fitting, hi not."""
    probes = [qmin]
    if size_of_q(qmin) > budget:
        return -1, probes
    if qmax == qmin:
        return qmin, probes
    probes.append(qmax)
    if size_of_q(qmax) <= budget:
        return qmax, probes
    lo, hi = qmin, qmax
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        probes.append(mid)
        if size_of_q(mid) <= budget:
            lo = mid
        else:
            hi = mid
    return lo, probes


def probe_count(qmin, qmax):
    """The launch's fixed number of probes: the longest probe list any frame can have."""
    if qmin == qmax:
        return 1
    n, d = 2, qmax - qmin
    while d > 1:
        d = (d + 1) >> 1
        n += 1
    return n


def inversions(sizes):
    """The qualities q with sizes[q + 1] < sizes[q] (sizes: a sequence indexed by quality)."""
    return [q for q in range(len(sizes) - 1) if sizes[q + 1] < sizes[q]]
