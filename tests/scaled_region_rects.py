"""Rectangles of the picture at 1/2 and 1/4 scale for the scaled region decode's tests (CPU and GPU)."""
import himg_amd


def up_rect(W, H, s, rect):
    """R^: the full-resolution rectangle a rectangle of the picture at scale 2^-s covers."""
    F = 1 << s
    x, y, w, h = rect
    return (F * x, F * y, min(F * w, W - F * x), min(F * h, H - F * y))


def rects(W, H, s):
    """Every x mod S and y mod S, single samples, the last (ragged) tile, the whole picture, a full-width
    row and a full-height column."""
    S = 8 >> s
    ow, oh = himg_amd.scaled_size(W, H, s)
    out = [(0, 0, ow, oh), (ow - 1, oh - 1, 1, 1), (0, 0, 1, 1), (ow - 1, 0, 1, 1), (0, oh - 1, 1, 1)]
    out += [(0, oh // 2, ow, 1), (ow // 2, 0, 1, oh)]
    lx, ly = (ow - 1) // S * S, (oh - 1) // S * S   # the last tile's first sample
    out += [(lx, ly, ow - lx, oh - ly), (max(0, lx - 1), max(0, ly - 1), ow - max(0, lx - 1), oh - max(0, ly - 1))]
    for dy in range(S):
        for dx in range(S):
            x, y = min(S + dx, ow - 1), min(S + dy, oh - 1)
            out.append((x, y, 1, 1))
            out.append((x, y, max(1, (ow - x) // 2), max(1, (oh - y) // 2)))
            out.append((x, y, ow - x, oh - y))
    return sorted(set(out))
