"""The encoder's Huffman tree by definition, in plain Python, and the argument behind k_tree's batches.

tree_model(hist) restates make_tree / store_tree of oracle/himg_oracle.c (huffman_enc.cpp:148-238)
literally: the leaves in ascending symbol order; again and again one scan over all nodes with `<=`
for the two lightest (so among equal counts the node with the HIGHEST index is the lightest, trap
T5), child_a the lighter; then a pre-order walk that writes a branch as bit 0, a leaf as bit 1 plus
9 symbol bits, and hands child_b the code bit of its depth (LSB first).  A single symbol is a leaf
with the 1-bit code 0.  No batching, no sorting, no shortcuts: this is what k_tree
(himg_amd/csrc/kernels_enc.hip) has to reproduce bit for bit.

merges_by_definition / merges_in_batches state the merge order and k_tree's batched form of it
(same thresholds, the same cap of 64 per kind; what a batch does not take goes to the serial loop,
like there).  tests/test_tree_batches.py holds the two against each other;
tests/test_tree_model_host.py uses batch_profile() to prove which part of the kernel a histogram of
the corpus (tests/tree_cases.py) drives.
"""
import sys

NUM_SYM = 261
SYMBOL_BITS = 9


def tree_model(hist):
    """hist: 261 counts.  Returns (lens[261], codes[261] as Python ints LSB first, tree bytes, byte count)."""
    assert len(hist) == NUM_SYM
    count, child_a, child_b, symbol = [], [], [], []
    for k in range(NUM_SYM):
        if hist[k] > 0:
            symbol.append(k); count.append(int(hist[k])); child_a.append(-1); child_b.append(-1)
    num = len(count)
    assert num > 0, "the empty histogram is not part of the format"
    root, left = -1, num
    while left > 1:
        n1 = n2 = -1
        for k in range(len(count)):
            if count[k] > 0:
                if n1 < 0 or count[k] <= count[n1]:
                    n2, n1 = n1, k
                elif n2 < 0 or count[k] <= count[n2]:
                    n2 = k
        root = len(count)
        child_a.append(n1); child_b.append(n2); symbol.append(-1)
        count.append(count[n1] + count[n2])
        count[n1] = count[n2] = 0
        left -= 1

    lens, codes, bits = [0] * NUM_SYM, [0] * NUM_SYM, []

    def store(n, code, depth):
        if symbol[n] >= 0:
            bits.append(1)
            bits.extend((symbol[n] >> b) & 1 for b in range(SYMBOL_BITS))
            codes[symbol[n]], lens[symbol[n]] = code, depth
            return
        bits.append(0)
        store(child_a[n], code, depth + 1)
        store(child_b[n], code + (1 << depth), depth + 1)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 2 * NUM_SYM + 100))
    try:
        if root >= 0:
            store(root, 0, 0)
        else:
            store(0, 0, 1)
    finally:
        sys.setrecursionlimit(limit)
    nbytes = (len(bits) + 7) // 8
    tree = bytearray(nbytes)
    for i, b in enumerate(bits):
        tree[i >> 3] |= b << (i & 7)
    return lens, codes, bytes(tree), nbytes


def merges_by_definition(counts):
    cnt = list(counts)
    alive = list(range(len(cnt)))
    out = []
    while len(alive) > 1:
        alive.sort(key=lambda i: (cnt[i], -i))
        a, b = alive[0], alive[1]
        cnt.append(cnt[a] + cnt[b])
        out.append((a, b))
        alive = alive[2:] + [len(cnt) - 1]
    return out


def merges_in_batches(counts, cap=64, report=None):
    """report (optional dict): filled with what the hand-over to the serial loop looked like --
    "leftover" (was the batches' odd node in hand), "serial_nodes" (nodes it started from),
    "grew" (how often a node the serial loop created joined a run of equal internal nodes that was
    still waiting: `grows` in the kernel) -- left untouched when the batches finish alone."""
    n = len(counts)
    cnt = list(counts)
    leaves = sorted(range(n), key=lambda i: (cnt[i], -i))
    lh, qh, nxt, y = 0, n, n, None
    out, rounds, serial = [], 0, 0
    while (n - lh) + (nxt - qh) + (y is not None) >= 2:
        heads = ([cnt[y]] if y is not None else []) + [cnt[leaves[k]] for k in range(lh, min(lh + 2, n))] \
            + [cnt[q] for q in range(qh, min(qh + 2, nxt))]
        heads.sort()
        s = heads[0] + heads[1]
        if lh + cap < n and cnt[leaves[lh + cap]] < s:
            s = cnt[leaves[lh + cap]]
        if qh + cap < nxt and cnt[qh + cap] < s:
            s = cnt[qh + cap]
        L = [leaves[k] for k in range(lh, min(lh + cap, n)) if cnt[leaves[k]] < s]
        I = [q for q in range(qh, min(qh + cap, nxt)) if cnt[q] < s]
        yin = y is not None and cnt[y] < s
        m = int(yin) + len(L) + len(I)
        if m < 2:      # the serial loop takes the rest
            rest = ([y] if y is not None else []) + [leaves[k] for k in range(lh, n)] + list(range(qh, nxt))
            if report is not None:
                report["leftover"] = y is not None
                report["serial_nodes"] = len(rest)
                report["grew"] = 0
            while len(rest) > 1:
                rest.sort(key=lambda i: (cnt[i], -i))
                a, b = rest[0], rest[1]
                cnt.append(cnt[a] + cnt[b])
                out.append((a, b))
                rest = rest[2:] + [len(cnt) - 1]
                serial += 1
                if report is not None and len(rest) > 1:
                    # the new node has the count of internal nodes that are still waiting: the last run
                    # of equal counts grows under the serial loop's hands (`grows` in the kernel)
                    new = len(cnt) - 1
                    if any(i >= n and i != new and cnt[i] == cnt[new] for i in rest):
                        report["grew"] += 1
            return out, rounds, serial
        # rank inside the batch exactly as the kernel computes it
        ranked = {}
        base = int(yin)
        if yin:
            ranked[0] = y
        for a, leaf in enumerate(L):
            le = sum(1 for q in I if cnt[q] <= cnt[leaf])
            ranked[base + a + le] = leaf
        for b, q in enumerate(I):
            run_b = b
            while run_b > 0 and cnt[I[run_b - 1]] == cnt[q]:
                run_b -= 1
            run_e = b + 1
            while run_e < len(I) and cnt[I[run_e]] == cnt[q]:
                run_e += 1
            kb = run_b + (run_e - 1 - b)
            lt = sum(1 for leaf in L if cnt[leaf] < cnt[q])
            ranked[base + kb + lt] = q
        assert sorted(ranked) == list(range(m)), "ranks are a permutation"
        B = [ranked[k] for k in range(m)]
        for k in range(m // 2):
            cnt.append(cnt[B[2 * k]] + cnt[B[2 * k + 1]])
            out.append((B[2 * k], B[2 * k + 1]))
        y = B[m - 1] if m & 1 else None
        lh, qh, nxt, rounds = lh + len(L), qh + len(I), nxt + m // 2, rounds + 1
    return out, rounds, serial


def batch_profile(hist):
    """Which part of k_tree's merge a histogram drives: dict with n (symbols), rounds (batches), serial
    (steps of the serial loop), leftover / grew (see merges_in_batches), and the merges themselves."""
    counts = [int(c) for c in hist if c > 0]
    rep = {}
    merges, rounds, serial = merges_in_batches(counts, report=rep)
    return {"n": len(counts), "rounds": rounds, "serial": serial, "leftover": bool(rep.get("leftover", False)),
            "grew": int(rep.get("grew", 0)), "merges": merges}
