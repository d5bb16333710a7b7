"""numpy model of the slots k_tok (kernels_enc.hip) writes for a block row of FRES symbols, and the
crafted pictures that drive a token segment to the edge of its capacity.

Test infrastructure only -- nothing under himg_amd/ imports this module.

k_tok's rules, restated from the kernel:
  * a non-zero symbol is one slot (it carries up to 255 zeros in front of it);
  * more than 255 zeros in front of a non-zero symbol are a run on its own in front of that slot:
    three slots (mark, length, a no-op that keeps the pair even-aligned) per started 16 662 zeros;
  * the row's trailing zeros (one or more) are such a run behind the row's last symbol;
  * the run in front of a symbol counts zeros of earlier segments of the row, never of another row;
  * a segment's slot count (tok_cnt) is what its symbols need; the tail written to memory is
    padded to a multiple of 8 slots;
  * a wavefront walks a segment 2048 symbols at a time; with c (< 8) slots carried over, an
    iteration whose slots fit the stage (c + total <= stage) is staged at once, otherwise its
    first 1024 symbols (lanes 0..31) and then the rest; whole groups of 8 slots leave, the
    remainder is carried.
"""
import ctypes as C

import numpy as np

import oracle_lib as ol

RUN_PIECE = 16662     # the reference's greedy split of a long run
MAX_LITERAL_RUN = 255
ITER = 2048           # symbols per wavefront iteration
STAGE = 1152          # slots of a wavefront's stage (kTokStage)

# L-shell scan order of a tile's coefficients (oracle/himg_oracle.c kIndexLUT): scan position i is
# coefficient INDEX_LUT[i] (row-major) of the tile.
INDEX_LUT = np.array([
    0, 1, 9, 8, 16, 17, 18, 10, 2, 3, 11, 19, 27, 26, 25, 24,
    32, 33, 34, 35, 36, 28, 20, 12, 4, 5, 13, 21, 29, 37, 45, 44,
    43, 42, 41, 40, 48, 49, 50, 51, 52, 53, 54, 46, 38, 30, 22, 14,
    6, 7, 15, 23, 31, 39, 47, 55, 63, 62, 61, 60, 59, 58, 57, 56], np.int64)


def _pieces(n):
    return (n + RUN_PIECE - 1) // RUN_PIECE


def slot_cost(row):
    """Slots every symbol position of one block row contributes (int64 [row_block])."""
    row = np.asarray(row)
    n = row.size
    cost = np.zeros(n, np.int64)
    nz = np.flatnonzero(row)
    if nz.size:
        lead = np.diff(np.concatenate(([-1], nz))) - 1      # zeros in front of every non-zero symbol
        cost[nz] = 1 + np.where(lead > MAX_LITERAL_RUN, 3 * _pieces(lead), 0)
    trail = n - 1 - (int(nz[-1]) if nz.size else -1)
    if trail:
        cost[n - 1] += 3 * _pieces(trail)                   # emitted by the lane that holds the row's end
    return cost


def row_demand(row, seg, nseg, stage=STAGE):
    """One block row: (slots per segment as tok_cnt holds them, int64 [nseg]; slots staged at every
    flush of the row's wavefronts, a list of (segment, staged, half): half is True for the two
    flushes of an iteration that did not fit the stage at once)."""
    row = np.asarray(row)
    n = row.size
    assert (nseg - 1) * seg < n <= nseg * seg and n % 64 == 0
    cs = np.concatenate(([0], np.cumsum(slot_cost(row))))
    counts = np.zeros(nseg, np.int64)
    staged = []
    for s in range(nseg):
        p0, p1 = s * seg, min((s + 1) * seg, n)
        counts[s] = cs[p1] - cs[p0]
        c = 0
        for q in range(p0, p1, ITER):
            e = min(q + ITER, p1)
            total = int(cs[e] - cs[q])
            if c + total <= stage:
                staged.append((s, c + total, False))
                c = (c + total) & 7
            else:
                m = min(q + ITER // 2, e)
                mid = int(cs[m] - cs[q])
                staged.append((s, c + mid, True))
                c = (c + mid) & 7
                staged.append((s, c + total - mid, True))
                c = (c + total - mid) & 7
    return counts, staged


def frame_demand(fres_sym, rows, seg, nseg, stage=STAGE):
    """A frame's FRES symbols (the oracle's trace): tok_cnt as k_tok leaves it (int64 [rows][nseg])
    and the most slots any flush stages.  (An iteration staged at once fits by the kernel's own
    test; only the halves of one that did not can outgrow the stage.)"""
    sym = np.asarray(fres_sym).reshape(rows, -1)
    counts = np.zeros((rows, nseg), np.int64)
    worst = 0
    for r in range(rows):
        counts[r], st = row_demand(sym[r], seg, nseg, stage)
        worst = max(worst, max(x for _, x, _ in st))
    return counts, worst


def padded(counts):
    """Slots written to memory: the tail padded to a whole 16-byte piece."""
    return (np.asarray(counts) + 7) // 8 * 8


# ---- the crafted pictures ----------------------------------------------------------------------

def pattern(seed, skip=()):
    """An 8 x 8 pattern (int16) whose forward transform is +-64 at scan positions 32..63 (seeded
    signs; not at the positions in `skip`) and 0 elsewhere: the oracle's inverse transform of it."""
    rng = np.random.RandomState(seed)
    coef = np.zeros(64, np.int16)
    for i in range(32, 64):
        sign = 1 if rng.randint(2) else -1
        if i not in skip:
            coef[INDEX_LUT[i]] = 64 * sign
    out = np.zeros(64, np.int16)
    ol.oracle().himg_oracle_hadamard_inverse(out.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p))
    fwd = np.zeros(64, np.int16)
    ol.oracle().himg_oracle_hadamard_forward(fwd.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(fwd, coef), "the forward transform gives the coefficients back"
    return out.reshape(8, 8)


VARIANTS = ("alpha", "chan2", "chan0", "fifth", "lastcol")


def crafted(variant, w, h, seed=1):
    """RGBA, every channel 128, plus -- identical in every tile, so that every box average is 128,
    the low-res plane flat and the residual the pattern itself (encode with use_ycbcr=False,
    q100 or q50: every +-64 survives the quantiser):
      alpha   the pattern in channel 3: a block row is 7/8 zeros, then a fully dense last segment;
      chan2   in channel 2: dense behind 5/8 of a row, then a trailing run of 1/8 of a row;
      chan0   in channel 0: dense behind 1/8 of a row, then a trailing run of 6/8 of a row;
      fifth   channel 3, every fifth tile column from a pattern without scan position 32: isolated
              zeros in the dense segment;
      lastcol channel 3 of the last tile column only: 32 literals behind almost a whole row of zeros.
    The pictures differ from a picture of period 8 in x by whole tile columns only."""
    assert w % 8 == 0 and h % 8 == 0 and variant in VARIANTS
    pat = pattern(seed)
    img = np.full((h, w, 4), 128, np.int16)
    ch = {"alpha": 3, "chan2": 2, "chan0": 0, "fifth": 3, "lastcol": 3}[variant]
    tiles_y, tiles_x = h // 8, w // 8
    if variant == "lastcol":
        img[:, w - 8:, ch] += np.tile(pat, (tiles_y, 1))
    else:
        img[:, :, ch] += np.tile(pat, (tiles_y, tiles_x))
        if variant == "fifth":
            alt = np.tile(pattern(seed, skip=(32,)), (tiles_y, 1))
            for u in range(0, tiles_x, 5):
                img[:, 8 * u:8 * u + 8, ch] = 128 + alt
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8)


def crafted_height(w):
    """Three block rows; two at 32768 pixels (the picture stays within a few MB)."""
    return 16 if w >= 32768 else 24
