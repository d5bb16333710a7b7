"""Pictures whose own token histograms give deep Huffman trees: long codes through the whole encoder.

All of them are RGBA, encoded at quality 100 without the colour lift (every shift 0, both companding
tables the identity on small values), built from numpy and the tree model alone; tests/test_deep_pictures_host.py holds
what they reach against the oracle's trace and records it in tests/golden/deep_reach.json.

A comb of depth d needs Fibonacci-like counts 1, 1, 2, 3, 5, ... and so about F(d + 3) tokens; the work
is in producing such a histogram WITHOUT stray symbols, which would fill the bottom of the tree and make
it bushy.  The low-res sample of a tile is a box from -3 to +4 around the tile's corner, rounded
(sample_image), so:

FRES (fres_deep).  Every tile is 128 plus a pattern so small that each box still rounds to 128: the
low-res plane is exactly flat, the LRES symbols are all zero and the FRES residual is the pattern itself.
  * A tile whose pixel (0, 0) is 128 + v (|v| <= 12) has all 64 Hadamard coefficients equal to v: 64
    tokens of one symbol and no zero.  Block rows filled with such tiles carry the bulk of the counts.
  * A tile 128 + a (-1)^(x + y) (|a| <= 18) has one non-zero coefficient, 64 a: one token.  The box sums
    of a checkerboard are +-a over any part of the tile, so alone among flat tiles it moves no box by more
    than 18, and beside a row of pixel tiles by no more than 30: still rounded away.  These give the rare
    classes their exact counts; they sit two tiles apart in otherwise flat block rows ("sparse rows"),
    whose zero runs add just two more symbols (one zero, and the longest run class with its 14 extra bits).
The counts are chosen leaf by leaf so that the running node of the comb and the next leaf stay the two
lightest (every count at least the sum of all counts two places below it), the zero-run symbols of the
sparse rows included, until tree_model says the depth is the one asked for.

LRES (lres_deep).  The picture is constant on every sampling box, so the box averages are free; they are
solved, in raster order, for a low-res plane (after the 15:1 blend) whose steps from sample to sample
under the "left" predictor are the wanted tokens: every sample a non-zero delta, the classes again
Fibonacci-like.  The left predictor wins every macro block because rows are independent random walks.
"""
import numpy as np

from tree_model import tree_model

NUM_SYM = 261
QUALITY = 100
USE_YCBCR = False
_CHECKER = (-1) ** np.add.outer(np.arange(8), np.arange(8))
_CHECKER_INDEX = 63          # where the checkerboard's coefficient lands among a tile's 64 symbol planes


def _alternating(n):
    """+1, -1, +2, -2, ... (n values)."""
    return [(k // 2 + 1) * (1 if k % 2 == 0 else -1) for k in range(n)]


def _sym8(v):
    return v & 255


def _fmap_symbol(value):
    """The full-res companding of +-64 a for |a| <= 18 (mapper.cpp:54-71): the table entry nearest to it."""
    table = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28,
             29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 51, 52, 54, 57, 59,
             62, 65, 68, 72, 76, 81, 86, 92, 98, 105, 113, 121, 130, 140, 151, 163, 176, 190, 205, 221, 239, 259,
             280, 303, 327, 354, 382, 413, 446, 482, 520, 561, 605, 653, 703, 757, 815, 876, 942, 1013, 1087, 1167,
             1252, 1342]
    a = abs(value)
    k = min(range(len(table)), key=lambda i: abs(table[i] - a))
    return k if value > 0 else 256 - k


def _zero_tokens(row_syms):
    """Token histogram of the zero runs of one block row of symbols (huffman_enc.cpp:105-141)."""
    h = np.zeros(NUM_SYM, np.int64)
    nz = np.flatnonzero(row_syms)
    edges = np.concatenate(([-1], nz, [row_syms.size]))
    for run in np.diff(edges) - 1:
        run = int(run)
        while run > 0:
            z = min(run, 16662)
            h[0 if z == 1 else 256 if z == 2 else 257 if z <= 6 else 258 if z <= 22 else 259 if z <= 278 else 260] += 1
            run -= z
    return h


def _depth_of(counts):
    h = [0] * NUM_SYM
    h[:len(counts)] = counts
    return max(tree_model(h)[0])


def _comb_counts(fixed, depth, small_max, small_classes, unit, big_classes):
    """Counts of new leaves that, with the leaves `fixed` (whose counts are given), make the tree a comb
    `depth` deep: in ascending order every leaf is at least the sum of all leaves two places below it, and
    no larger than that asks for.  A fixed leaf is taken in where the sequence reaches its count.  New counts
    up to small_max are exact (at most small_classes of them), larger ones multiples of `unit`.  Returns
    (small counts, big counts), both ascending."""
    pending = sorted(fixed)
    seq, small, big = [], [], []
    while _depth_of(seq + pending) < depth:
        need = 1 if len(seq) < 2 else max(seq[-1], sum(seq[:-1]))
        if pending and pending[0] <= need + need // 4:
            seq.append(pending.pop(0))
            seq.sort()
            continue
        if need <= small_max and len(small) < small_classes:
            small.append(need)
        else:
            need = -(-need // unit) * unit
            assert len(big) < big_classes, "out of symbols"
            big.append(need)
        seq.append(need)
    return small, big


def fres_deep(width, depth, sparse_rows=8, walsh_max=400, seed=1):
    """An RGBA picture `width` wide whose FRES tree has a longest code of `depth` bits.  Returns
    (pixels [H][W][4] uint8, design) with design the intended token histogram (dict symbol -> count) and
    the block rows that hold the rare tokens."""
    assert width % 8 == 0 and width >= 64
    cols, C = width // 8, 4
    rng = np.random.default_rng(seed)
    row_block = C * 64 * cols

    # The rare classes are checkerboard tiles with exact counts in the sparse rows; the bulk is pixel tiles,
    # 64 tokens each.  The zero runs of the sparse rows depend on how many rare tokens there are, and the
    # counts on those runs: a few rounds settle it.
    values = _alternating(24)                            # pixel tiles: +-1 .. +-12
    per_stretch = (cols - 4) // 2                        # tiles 2, 4, 6, ... of a channel's stretch, clear of both edges
    zero_hist = np.zeros(NUM_SYM, np.int64)
    zero_hist[260], zero_hist[0] = 4 * sparse_rows, 300
    for _ in range(12):
        fixed = [int(x) for x in zero_hist[zero_hist > 0]]
        w_counts, p_counts = _comb_counts(fixed, depth, walsh_max, 36, 64, len(values))
        amps = _alternating(len(w_counts))
        tokens = [a for a, n in zip(amps, w_counts) for _ in range(n)]
        tokens = [tokens[k] for k in np.random.default_rng(seed).permutation(len(tokens))]
        n_rows = max(sparse_rows, -(-len(tokens) // (3 * per_stretch)))   # channels 0..2 of each sparse row
        sparse = [[] for _ in range(n_rows)]             # per sparse row: list of (channel, tile, amplitude)
        for k, a in enumerate(tokens):                   # round robin over (row, channel)
            st = k % (n_rows * 3)
            sparse[st % n_rows].append((st // n_rows, 2 + 2 * (k // (n_rows * 3)), a))
        zh = np.zeros(NUM_SYM, np.int64)
        for tiles in sparse:
            row = np.zeros(row_block, np.uint8)
            for c, u, a in tiles:
                row[(c * 64 + _CHECKER_INDEX) * cols + u] = 1
            zh += _zero_tokens(row)
        if np.array_equal(zh, zero_hist):
            break
        zero_hist = zh
    else:
        raise AssertionError("the zero runs of the sparse rows did not settle")
    sparse_rows = n_rows
    slots = sum(p_counts) // 64
    dense_rows = -(-slots // (cols * C))
    p_counts[-1] += (dense_rows * cols * C - slots) * 64  # the last row is filled up with the commonest class
    # rare values get the large magnitudes: the commonest class is +1
    p_values = values[:len(p_counts)][::-1]
    pool = np.repeat(np.array(p_values, np.int16), [n // 64 for n in p_counts])
    # Shuffled over the dense rows, except the tiles of the four rarest pixel classes: they lie side by side in one
    # row, so that a stretch of consecutive symbols there is all long codes (more bits than an emit lane holds
    # privately).
    n_rare = min(sum(p_counts[:4]) // 64, cols)
    rest = pool[n_rare:][rng.permutation(pool.size - n_rare)]
    cut = (dense_rows // 2) * C * cols
    pool = np.concatenate([rest[:cut], pool[:n_rare], rest[cut:]]).reshape(dense_rows, C, cols)

    rows = dense_rows + sparse_rows
    at = set(int(x) for x in np.linspace(0, rows - 1, sparse_rows).round())   # sparse rows spread over the picture, first and last included
    assert len(at) == sparse_rows and dense_rows >= sparse_rows
    img = np.full((rows * 8, width, C), 128, np.uint8)
    d = s = 0
    sparse_at = []
    for r in range(rows):
        if r in at:
            for c, u, a in sparse[s]:
                img[8 * r:8 * r + 8, 8 * u:8 * u + 8, c] = 128 + a * _CHECKER
            sparse_at.append(r)
            s += 1
        else:
            img[8 * r, 0::8, :] = (128 + pool[d].T).astype(np.uint8)
            d += 1
    design = {}
    for a, n in zip(amps, w_counts):
        design[_fmap_symbol(64 * a)] = n
    for v, n in zip(p_values, p_counts):
        design[_sym8(v)] = n
    for k in np.flatnonzero(zero_hist):
        design[int(k)] = int(zero_hist[k])
    return img, {"hist": design, "sparse_rows": sparse_at, "depth": depth}


def lres_deep(width, height, seed=2):
    """An RGBA picture whose LRES tree is as deep as its low-res plane (width/8 x height/8 x 4 samples,
    a token each) allows.  Returns (pixels, design) with design["hist"] the intended token histogram."""
    assert width % 128 == 0 and height % 128 == 0
    rows, cols, C = height // 8, width // 8, 4
    n = rows * cols * C
    rng = np.random.default_rng(seed)
    mrows, mcols = rows // 16, cols // 16
    run = mrows * mcols                                  # the predictor bytes of a channel: one run of zeros
    zero_hist = _zero_tokens(np.concatenate([np.zeros(run, np.uint8), [1]])) * C
    fixed = [int(x) for x in zero_hist[zero_hist > 0]]
    # classes until the samples are used up (the zero runs taken in where the sequence reaches their count);
    # the commonest takes what is left
    pending, seq, counts = sorted(fixed), [], []
    while True:
        need = 1 if len(seq) < 2 else max(seq[-1], sum(seq[:-1]))
        if pending and pending[0] <= need + need // 4:
            seq.append(pending.pop(0))
            seq.sort()
            continue
        if sum(counts) + need > n:
            break
        counts.append(need)
        seq.append(need)
    counts[-1] += n - sum(counts)
    values = _alternating(len(counts))[::-1]             # the commonest class is +1, then -1, +2, ...
    assert max(abs(v) for v in values) <= 40             # (the low-res companding is the identity there)
    pool = np.repeat(np.array(values, np.int64), counts)
    pool = pool[rng.permutation(n)].tolist()

    lo, hi = 24, 231
    m = np.zeros((C, rows, cols), np.int64)
    k = 0
    for c in range(C):
        for mv in range(mrows):
            for mu in range(mcols):
                for dv in range(16):
                    for du in range(16):
                        v, u = mv * 16 + dv, mu * 16 + du
                        pred = m[c, v, u - 1] if du > 0 else m[c, v - 1, u] if dv > 0 else 128
                        j = k
                        while not lo <= pred + pool[j] <= hi:   # keep the walk inside: take a later token instead
                            j += 1
                        pool[k], pool[j] = pool[j], pool[k]
                        m[c, v, u] = pred + pool[k]
                        k += 1
    # box averages A whose 15:1 blend (sample_image) is exactly m, in raster order
    A = np.zeros((C, rows, cols), np.int64)
    for c in range(C):
        for v in range(rows):
            r1 = max(v - 1, 0)
            for u in range(cols):
                c1 = max(u - 1, 0)
                want = int(m[c, v, u])
                guess = want if (v == 0 or u == 0) else int(round((want * 256 - 15 * (A[c, r1, u] + A[c, v, c1]) - A[c, r1, c1]) / 225.0))
                for x in sorted(range(max(guess - 6, 0), min(guess + 7, 256)), key=lambda t: abs(t - guess)):
                    x12 = x if r1 == v else int(A[c, r1, u])
                    x21 = x if c1 == u else int(A[c, v, c1])
                    x11 = x if (r1 == v and c1 == u) else x12 if c1 == u else x21 if r1 == v else int(A[c, r1, c1])
                    a1 = (x11 + 15 * x12 + 8) >> 4
                    a2 = (x21 + 15 * x + 8) >> 4
                    if (a1 + 15 * a2 + 8) >> 4 == want:
                        A[c, v, u] = x
                        break
                else:
                    raise AssertionError("no box average gives the wanted low-res sample")
    yi = np.minimum((np.arange(height) + 3) // 8, rows - 1)
    xi = np.minimum((np.arange(width) + 3) // 8, cols - 1)
    img = A[:, yi][:, :, xi].transpose(1, 2, 0).astype(np.uint8)
    design = {_sym8(v): cnt for v, cnt in zip(values, counts)}
    for s in np.flatnonzero(zero_hist):
        design[int(s)] = int(zero_hist[s])
    return np.ascontiguousarray(img), {"hist": design}


# The pictures of the tests: name -> (builder, what the issue asks of it).
def fres_wide():
    return fres_deep(1024, 32)


def fres_narrow():
    return fres_deep(256, 28)


def lres_picture():
    return lres_deep(1024, 1536)


_CACHE = {}


def picture(name):
    """"fres_wide" (row_block 32768, the wide emit form), "fres_narrow" (row_block 8192) or "lres": (pixels, design)."""
    if name not in _CACHE:
        _CACHE[name] = {"fres_wide": fres_wide, "fres_narrow": fres_narrow, "lres": lres_picture}[name]()
    return _CACHE[name]


NAMES = ("fres_wide", "fres_narrow", "lres")
_TRACED = {}


def traced(name):
    """(pixels, design, the oracle's stream, the oracle's trace) of a picture, encoded once per process."""
    if name not in _TRACED:
        import oracle_lib as ol
        img, design = picture(name)
        _TRACED[name] = (img, design) + tuple(ol.oracle_encode(img, QUALITY, USE_YCBCR, trace=True))
    return _TRACED[name]
