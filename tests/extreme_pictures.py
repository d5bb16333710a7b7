"""Pictures that drive the codec's arithmetic to its limits (numpy only, deterministic; test
infrastructure).  Every pattern is laid out per 8 x 8 tile on the padded tile grid and cropped to
w x h, so ragged sizes keep the pattern of their full tiles.  tests/test_extreme_host.py proves, with
the oracle, what each kind reaches (tests/golden/extreme_reach.json).

    walsh      tile t (row-major over the tile grid) carries one separable 8 x 8 Walsh basis as
               0 / 255.  Four arrangements in turn, by (t + (t >> 7)) & 3:
                 0  every channel basis t mod 64, signs + - + - over the channels (B against G and R
                    against G: Cb and Cr swing 0 .. 255 while Y stays flat)
                 1  every channel basis t mod 64, one sign (Y swings 0 .. 255)
                 2, 3  the same two with channel c at basis (t + 16 c) mod 64
               and every sign flipped in tiles with (t >> 6) odd: within 128 tiles every basis
               appears with both signs in every channel.
    step       tiles cycle by (u + v) mod 4 (u, v the tile's column and row): left half 255 / right
               half 0, all 255, bottom half 255 / top half 0, all 0 -- the bilinear low-res
               prediction leans the wrong way across the tile.  R, G, B step together (so Y does),
               except that G is inverted where ((u + v) >> 2) is odd (so Cb and Cr do); alpha is
               inverted.
    tilecheck  whole tiles alternate 0 / 255; alpha inverted.
    bin        independent 0 / 255 bytes.
    cube       per tile one of the eight corners of the RGB cube (alpha 0 or 255); every second tile
               alternates the corner and its opposite per pixel in a checkerboard, e.g. (255, 0, 255)
               against (0, 255, 0): Cb and Cr at 0 and 255 while Y stays mid-range.
    ties       flat 128 plus a per-pixel offset in -2 .. 2: most quantised values sit at 0 / +-1,
               across the rounding boundary of the sign-magnitude shift.
"""
import numpy as np

KINDS = ("walsh", "step", "tilecheck", "bin", "cube", "ties")

# H8[k][x] = (-1) ** popcount(k & x): the eight Walsh functions (natural order).
H8 = np.array([[1 - 2 * (bin(k & x).count("1") & 1) for x in range(8)] for k in range(8)], np.int32)


def _expand(tiles):
    """[rows][cols][8][8][C] -> [rows * 8][cols * 8][C]."""
    rows, cols, _, _, c = tiles.shape
    return tiles.transpose(0, 2, 1, 3, 4).reshape(rows * 8, cols * 8, c)


def _walsh(rows, cols, channels):
    t = np.arange(rows * cols).reshape(rows, cols)
    arrangement = (t + (t >> 7)) & 3
    out = np.empty((rows, cols, 8, 8, channels), np.uint8)
    for c in range(channels):
        basis = (t + 16 * (c & 3) * (arrangement >= 2)) & 63
        minus = ((t >> 6) + (c & 1) * (1 - (arrangement & 1))) & 1
        pat = H8[basis >> 3][:, :, :, None] * H8[basis & 7][:, :, None, :]       # [rows][cols][y][x]
        pat = pat * (1 - 2 * minus)[:, :, None, None]
        out[..., c] = np.where(pat > 0, 255, 0)
    return _expand(out)


def _step(rows, cols, channels):
    v, u = np.mgrid[0:rows, 0:cols]
    y, x = np.mgrid[0:8, 0:8]
    pats = np.stack([np.where(x < 4, 255, 0), np.full((8, 8), 255), np.where(y >= 4, 255, 0), np.zeros((8, 8), int)])
    p = pats[(u + v) & 3].astype(np.uint8)                                        # [rows][cols][8][8]
    out = np.repeat(p[..., None], channels, axis=-1)
    if channels >= 2:
        g_inv = (((u + v) >> 2) & 1).astype(bool)
        out[..., 1] = np.where(g_inv[:, :, None, None], 255 - p, p)
    if channels >= 4:
        out[..., 3] = 255 - p
    return _expand(out)


def _tilecheck(rows, cols, channels):
    v, u = np.mgrid[0:rows, 0:cols]
    p = (((u + v) & 1) * 255).astype(np.uint8)
    out = np.repeat(np.broadcast_to(p[:, :, None, None], (rows, cols, 8, 8))[..., None], channels, axis=-1).copy()
    if channels >= 4:
        out[..., 3] = 255 - out[..., 3]
    return _expand(out)


def _cube(rows, cols, channels, seed):
    v, u = np.mgrid[0:rows, 0:cols]
    y, x = np.mgrid[0:8, 0:8]
    corner = (u + 3 * v + seed) & 7
    # every second tile: the opposite corner on the odd pixels of a checkerboard
    flip = (((u + v) & 1)[:, :, None, None] * ((x + y) & 1)[None, None]).astype(bool)
    k = np.where(flip, 7 - corner[:, :, None, None], corner[:, :, None, None])
    out = np.empty((rows, cols, 8, 8, channels), np.uint8)
    for c in range(channels):
        if c < 3:
            out[..., c] = ((k >> c) & 1) * 255
        else:
            out[..., c] = np.broadcast_to(((((u >> 1) + v) & 1) * 255)[:, :, None, None], (rows, cols, 8, 8))
    return _expand(out)


def picture(kind, w, h, channels=4, seed=0):
    """uint8 (h, w, channels) picture of `kind` (KINDS) for any w, h >= 1."""
    if w < 1 or h < 1 or channels < 1:
        raise ValueError("picture: w, h and channels must be at least 1")
    rows, cols = (h + 7) // 8, (w + 7) // 8
    if kind == "walsh":
        full = _walsh(rows, cols, channels)
    elif kind == "step":
        full = _step(rows, cols, channels)
    elif kind == "tilecheck":
        full = _tilecheck(rows, cols, channels)
    elif kind == "cube":
        full = _cube(rows, cols, channels, seed)
    elif kind == "bin":
        full = (np.random.default_rng(seed).integers(0, 2, (rows * 8, cols * 8, channels)) * 255).astype(np.uint8)
    elif kind == "ties":
        full = (128 + np.random.default_rng(seed).integers(-2, 3, (rows * 8, cols * 8, channels))).astype(np.uint8)
    else:
        raise ValueError("picture: unknown kind %r" % (kind,))
    return np.ascontiguousarray(full[:h, :w])
