"""The argument behind k_tree's batched merge (himg_amd/csrc/kernels_enc.hip), checked on the CPU.

The reference builds its Huffman tree by joining, again and again, the two lightest nodes under
the total order (count ascending, node index DESCENDING) -- huffman_enc.cpp:183-238, trap T5: the
tie-breaking is part of the format.  k_tree does not take those merges one by one: with x1, x2
the two lightest nodes and s = count(x1) + count(x2), every node created from now on weighs at
least s, so all nodes lighter than s are consumed first, in that order and in consecutive pairs;
an odd last one is left over for the next batch.  This file states that batching in plain Python
(same thresholds and the same 64-per-kind cap as the kernel; what a batch does not take goes to
the serial loop, like there; the two functions live in tests/tree_model.py) and compares the
sequence of merges with the O(n^2) definition on tie-heavy, geometric, heavy-tailed, uniform and
all-equal histograms.  The kernel itself is checked byte for byte by the GPU parity tests and, on
histograms no picture produces, by tests/test_gpu_trees.py; this pins the reasoning it rests on."""
import numpy as np

from tree_model import merges_by_definition, merges_in_batches


def _hist(kind, n, rng):
    if kind == 0:
        return [int(x) for x in rng.integers(1, 4, n)]                 # ties everywhere
    if kind == 1:
        return [int(x) for x in rng.integers(1, 1000000, n)]
    if kind == 2:
        return [int(1.3 ** k) + 1 for k in range(n)]                    # geometric: one merge per batch
    if kind == 3:
        return [7] * n                                                  # all equal: the serial loop's case beyond 64
    return [int(x) for x in (rng.pareto(1.0, n) * 10 + 1)]              # heavy tail


def test_batches_reproduce_the_definition():
    rng = np.random.default_rng(5)
    batched_steps = serial_steps = 0
    for t in range(300):
        n = int(rng.integers(2, 262))
        h = _hist(t % 5, n, rng)
        want = merges_by_definition(h)
        got, rounds, serial = merges_in_batches(h)
        assert got == want, (t % 5, n)
        if t % 5 in (1, 2, 4):     # (kinds 0 and 3 are the long runs of equal counts the serial loop is kept for)
            batched_steps += len(want) - serial
            serial_steps += serial
    assert batched_steps > 10 * serial_steps      # elsewhere the batches do the bulk of the work


def test_token_like_histogram_takes_few_batches():
    """Counts like a frame's token histogram (a few huge bins, a long tail of small ones)."""
    rng = np.random.default_rng(9)
    h = sorted(int(x) for x in (rng.pareto(0.7, 180) * 3 + 1))
    want = merges_by_definition(h)
    got, rounds, serial = merges_in_batches(h)
    assert got == want and serial == 0 and rounds < len(want) // 3
