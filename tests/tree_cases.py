"""The histogram corpus for the encoder's tree kernel: token histograms no picture produces.

cases() returns a list of (family, subset, hist) with hist a uint32[261]; deterministic, numpy only.
A family is a list of counts; a subset says which symbols carry them (in ascending symbol order, which
is the node order the tie-breaking depends on):

  prefix     symbols 0 .. n-1
  gaps       a seeded random choice of n of the 261 symbols
  straddle   the n symbols nearest to the edges 63/64, 127/128, 191/192 and 255/256 of the kernel's
             64-lane ballots (two symbols straddle the first, eight all four; 256..260 come early)

What each family is for is said where it is built.  tests/test_tree_model_host.py proves on the CPU that
the corpus reaches the parts of k_tree it is meant for (batches alone, the serial loop alone, a hand-over
with and without a left-over node, depths 32 and beyond) and records the counts in
tests/golden/tree_reach.json; tests/test_gpu_trees.py runs the kernel over all of it.

The empty histogram is left out: the format never produces it.
"""
import json
import os

import numpy as np

NUM_SYM = 261
INT_MAX = 2 ** 31 - 1          # the reference keeps counts in int (huffman_enc.cpp:183-238), k_tree's cnt[] likewise
SUBSETS = ("prefix", "gaps", "straddle")
_EDGES = (63.5, 127.5, 191.5, 255.5)
_STRADDLE_ORDER = sorted(range(NUM_SYM), key=lambda s: (min(abs(s - e) for e in _EDGES), s))
PICTURE_HISTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_picture_hists.json")


def subset(kind, n, seed=0):
    if kind == "prefix":
        return list(range(n))
    if kind == "gaps":
        return sorted(int(x) for x in np.random.default_rng(1000 + 7 * n + seed).choice(NUM_SYM, n, replace=False))
    return sorted(_STRADDLE_ORDER[:n])


def place(counts, symbols):
    assert len(counts) == len(symbols) and all(c > 0 for c in counts) and sum(counts) <= INT_MAX, (len(counts), sum(counts))
    h = np.zeros(NUM_SYM, np.uint32)
    h[symbols] = counts
    return h


def fib(k):
    a, b = 1, 1        # fib(1) = fib(2) = 1
    for _ in range(k - 1):
        a, b = b, a + b
    return a


def comb(depth):
    """depth + 1 Fibonacci counts 1, 1, 2, 3, 5, ...: every merge joins the running node with the next
    leaf, so the tree is a comb whose longest code has exactly `depth` bits."""
    return [fib(k) for k in range(1, depth + 2)]


def _families():
    """(family name, counts) pairs; every one of them is placed at each of SUBSETS by cases()."""
    out = []
    rng = np.random.default_rng(20240601)

    # All counts equal, every n: up to 64 leaves one batch takes them all; from 65 on no threshold separates
    # them and the serial loop does the whole tree, with a run of equal internal nodes that grows as it goes.
    for n in range(2, NUM_SYM + 1):
        out.append(("equal1/n%d" % n, [1] * n))
        out.append(("equalbig/n%d" % n, [8000000] * n))          # 261 * 8e6 < 2^31

    # Two- and three-valued counts: ties everywhere, between leaves and between internal nodes.
    for n in (5, 33, 64, 65, 100, 130, 200, 261):
        for vals in ((1, 2), (3, 5), (7, 14), (1000, 1001), (1, 2, 3), (2, 3, 5), (1, 2, 4), (5, 10, 20)):
            for rep in range(2):
                out.append(("valued%s/n%d/%d" % ("_".join(map(str, vals)), n, rep), [int(x) for x in rng.choice(vals, n)]))

    # A run of equal leaves longer than a batch takes, with k lighter leaves below it and heavier ones above:
    # the batches consume what is lighter (an odd k leaves a node in hand), then stop at the run and hand over.
    for run in (63, 64, 65, 66, 128, 129, 200):
        room = NUM_SYM - run
        for k in list(range(0, min(room, 24) + 1)) + [min(room, 40), room]:
            for c in (5, 64):
                low = [1 + (j % c if c > 5 else j % 4) for j in range(k)]          # lighter than the run, ties among them
                for where, high in (("bottom" if k == 0 else "middle", [c * 3 + 7 * j for j in range(room - k)]),
                                    ("top", [])):
                    if where == "top" and k == 0:
                        continue
                    out.append(("run%d/%s/k%d/c%d" % (run, where, k, c), low + [c] * run + high))
        # the same with distinct lighter leaves whose sums tie with the run's count
        out.append(("run%d/tie" % run, [1, 1, 2, 4, 8] + [16] * run + [16 * 3] * min(5, room - 5)))

    # Internal nodes that tie with leaves and with each other.
    for pairs in (3, 8, 16, 30):
        out.append(("pow2pairs/%d" % pairs, [1 << (j // 2) for j in range(2 * pairs)]))          # 1,1,2,2,4,4,...
    for m in range(1, 6):
        K = 0
        while m * (2 ** (K + 2) - 1) <= INT_MAX and m * (K + 2) <= NUM_SYM:
            K += 1
        for kk in sorted({3, 10, K}):
            out.append(("pow2x%d/k%d" % (m, kk), [1 << j for j in range(kk + 1) for _ in range(m)]))
    out.append(("ones256/heavy5", [1] * 256 + [128, 300, 1000, 65536, 70000]))          # 128 equal internal nodes
    out.append(("ones256/heavy2", [1] * 256 + [2, 2, 2, 2, 4]))
    for ones, heavy in ((200, [100, 100, 4000]), (130, [65, 65, 130]), (128, [64, 127, 128, 129])):
        out.append(("ones%d/heavy%d" % (ones, len(heavy)), [1] * ones + heavy))

    # Combs of an exact depth, around the limit of 32 bits (status 3 beyond it).
    for d in (31, 32, 33, 34, 40):
        c = comb(d)
        out.append(("comb%d/asc" % d, c))
        out.append(("comb%d/desc" % d, c[::-1]))
        out.append(("comb%d/shuffled" % d, [c[j] for j in np.random.default_rng(d).permutation(len(c))]))
        out.append(("comb%d/doubled" % d, [2 * x for x in c]))
        out.append(("comb%d/heavy" % d, c + [sum(c) + 1]))          # one more level on top
    # a comb beside a bushy part: long codes and a batchable bulk in one tree
    out.append(("comb32/bushy", comb(32) + [3] * 100))
    out.append(("comb30/bushy", comb(30) + [1000] * 70 + [1] * 40))

    # Totals at the reference's int limit.
    for n in (2, 3, 64, 65, 200, 261):
        q, r = divmod(INT_MAX, n)
        out.append(("intmax/even/n%d" % n, [q + (1 if j < r else 0) for j in range(n)]))
        tail = [int(x) for x in rng.integers(1, 1000, n - 1)]
        out.append(("intmax/dominant/n%d" % n, tail + [INT_MAX - sum(tail)]))
        out.append(("intmax/dominant_first/n%d" % n, [INT_MAX - sum(tail)] + tail))
    out.append(("intmax/comb40", comb(40)[:-1] + [INT_MAX - sum(comb(40)[:-1])]))

    # Smooth distributions.
    for n in (7, 64, 65, 129, 181, 261):
        for ratio in (1.05, 1.3, 2.0):
            out.append(("geometric%.2f/n%d" % (ratio, n), [min(int(ratio ** k) + 1, INT_MAX // NUM_SYM) for k in range(n)]))
        out.append(("pareto/n%d" % n, [int(x) for x in rng.pareto(1.0, n) * 10 + 1]))
        out.append(("uniform/n%d" % n, [int(x) for x in rng.integers(1, 1000000, n)]))
        out.append(("tokenlike/n%d" % n, sorted(int(x) for x in rng.pareto(0.7, n) * 3 + 1)))
    return out


def _random_cases(count=2000):
    """Seeded random histograms, n uniform in 1..261, on random symbols: the kinds cycle through ties
    everywhere, wide uniform, heavy tails, geometric and narrow ranges."""
    rng = np.random.default_rng(77)
    out = []
    for t in range(count):
        n = int(rng.integers(1, NUM_SYM + 1))
        kind = t % 6
        if kind == 0:
            c = rng.integers(1, 4, n)
        elif kind == 1:
            c = rng.integers(1, 1000000, n)
        elif kind == 2:
            c = np.minimum(rng.pareto(0.8, n) * 5 + 1, 5e6)
        elif kind == 3:
            c = np.minimum(1.0 + rng.uniform(1.02, 1.6) ** rng.permutation(n), 5e6)
        elif kind == 4:
            c = rng.integers(1, 21, n)
        else:
            c = rng.choice([1, 2, 4, 8, 16, 64, 4096], n)
        syms = sorted(int(x) for x in rng.choice(NUM_SYM, n, replace=False))
        out.append(("random%d/%d" % (kind, t), "random", place([int(x) for x in c], syms)))
    return out


def picture_cases():
    """The LRES and FRES token histograms the oracle traces for a handful of real pictures, the deep
    pictures of tests/deep_pictures.py among them (tests/test_tree_model_host.py holds the file against the
    oracle)."""
    if not os.path.exists(PICTURE_HISTS):
        return []
    with open(PICTURE_HISTS) as f:
        rec = json.load(f)
    out = []
    for name in sorted(rec):
        for strm in ("lres", "fres"):
            out.append(("picture/" + name, strm, np.array(rec[name][strm + "_hist"], np.uint32)))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out = []
        for s in (0, 1, 63, 64, 255, 256, 257, 260):          # one symbol: a 1-bit code 0
            for c in (1, 1000, INT_MAX):
                out.append(("one/c%d" % c, "sym%d" % s, place([c], [s])))
        for a, b in ((0, 1), (63, 64), (127, 128), (255, 256), (0, 260), (259, 260)):
            for ca, cb in ((1, 1), (1, 2), (2, 1), (5, 5), (1, INT_MAX - 1)):
                out.append(("two/c%d_%d" % (ca, cb), "sym%d_%d" % (a, b), place([ca, cb], [a, b])))
        for name, counts in _families():
            for kind in SUBSETS:
                if len(counts) == NUM_SYM and kind != "prefix":
                    continue          # (all 261 symbols: the three subsets are the same)
                out.append((name, kind, place(counts, subset(kind, len(counts)))))
        out += _random_cases()
        out += picture_cases()
        _CASES = out
    return _CASES


_EXPECTED = None


def expected():
    """tree_model of every case, computed once per process: a list of (lens, codes, tree, nbytes)."""
    global _EXPECTED
    if _EXPECTED is None:
        from tree_model import tree_model
        _EXPECTED = [tree_model(h.tolist()) for _, _, h in cases()]
    return _EXPECTED
