"""Inputs of the tests of scaled windows on an opened-streams handle (test_opened_scaled_host.py,
test_gpu_opened_scaled.py): the picture's size at a scale, the independence windows of stream_region_cases mapped
to each scale with what the models say of them, and the calls of the shared-counts test.  Built with the oracle
and numpy alone, so the CPU suite can prove that the GPU cases are not vacuous.

Test infrastructure only.
"""
import functools

import numpy as np

import damage_model as dm
import scaled_model as sm
import stream_region_cases as sc
from scaled_region_rects import up_rect

SCALES = (1, 2, 3)
# The independence windows' size at each scale: stream_region_cases.WIN (24 x 17) covers three block rows at most,
# and so do these (S = 4, 2, 1 samples of a tile's side).
WIN = {1: (12, 9), 2: (6, 5), 3: (3, 3)}


def size(W, H, s):
    """The picture at scale 2^-s: ceil(W / F) x ceil(H / F) (s = 3: the low-res plane, cols x rows)."""
    F = 1 << s
    return (W + F - 1) // F, (H + F - 1) // F


def rows_of(s, y, h):
    """The block rows [r0, r1) a window of height h at y of the picture at scale 2^-s touches (s = 0: full size)."""
    S = 8 >> s
    return y // S, (y + h + S - 1) // S


def windows(s):
    """stream_region_cases.windows() at scale 2^-s: (stream_of, origins (x // F, y // F)); the size is WIN[s]."""
    so, org = sc.windows()
    return so, (org >> s).astype(np.int32)


@functools.lru_cache(maxsize=None)
def expected(name, s):
    """Per window of windows(s), s = 1 or 2: (code, crop or None).  The verdict is damage_model.expect_region's of
    the covered full-resolution rectangle R^; the pixels of a window that passes are the crop of the scaled model
    of the stream the window sees (damage_model.scaled).  The head case: FORMAT for every window of stream 0."""
    good, bad, clean = sc.independence_cases()[name]
    so, org = windows(s)
    w, h = WIN[s]
    rc, clean_img = sm.expected(clean, s)
    assert rc == 0
    out = []
    for k, (x, y) in zip(so, org):
        x, y = int(x), int(y)
        if k == 1:
            out.append((dm.OK, clean_img[y:y + h, x:x + w]))
        elif name == "head":
            out.append((dm.FORMAT, None))
        else:
            code, _, X = dm.expect_region(good, bad, up_rect(sc.W, sc.H, s, (x, y, w, h)), False)
            out.append((code, dm.scaled(X, s, False)[y:y + h, x:x + w] if code == dm.OK else None))
    return out


# The shared-counts test, on stream 1 of a handle over two streams of stream_region_cases' geometry, in order:
# (scale_log2, (x, y), (w, h), the block rows touched, count launches, rows_counted afterwards).
COUNT_STEPS = [
    (0, (33, 20), (24, 17), (2, 5), 1, 3),    # full resolution: rows 2, 3, 4 are new
    (1, (16, 10), (12, 9), (2, 5), 0, 3),     # 1/2 scale over the same rows: nothing to count
    (2, (2, 6), (10, 8), (3, 7), 1, 5),       # 1/4 scale: rows 5 and 6 are new
    (3, (0, 0), size(sc.W, sc.H, 3), None, 0, 5),   # 1/8 scale, the whole picture: no row is touched
    (0, (7, 16), (40, 39), (2, 7), 0, 5),     # full resolution over rows counted by three entry points
]
