"""Inputs of the tests of many windows per stream (test_stream_regions_host.py, test_gpu_stream_regions.py):
the streams, the damaged streams of the independence cases and the windows laid above, across and below the
damage.  Built with the oracle and numpy alone, so the CPU suite can prove that the GPU cases are not vacuous.

Test infrastructure only.
"""
import functools
import struct

import numpy as np

import himg_amd
import oracle_lib as ol
import damage_model as dm
from test_gpu_region import _ends_after_row, _full   # (that module imports torch, but needs no GPU to be imported)

W, H, C = 96, 72, 4          # nine block rows, twelve tile columns
WIN = (24, 17)               # three block rows at most
ROWS = (H + 7) // 8
# y of the windows: block rows [0, 3), [2, 5), [3, 6), [5, 8), [6, 9)
YS = (0, 20, 30, 40, 55)
XS = (0, 7, 33, 72, 5)


@functools.lru_cache(maxsize=None)
def stream(kind="randtile", w=W, h=H, c=C, q=50, seed=0, ycbcr=True):
    img = himg_amd.synth(kind, seed, w, h)
    if c != img.shape[2]:
        img = np.ascontiguousarray(img[:, :, :c])
    s = np.frombuffer(ol.oracle_encode(img, q, ycbcr), np.uint8).copy()
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def full(kind="randtile", w=W, h=H, c=C, q=50, seed=0, ycbcr=True):
    return _full(stream(kind, w, h, c, q, seed, ycbcr), needs_fix(kind, w, h, c, q, seed, ycbcr)).reshape(h, w, c)


@functools.lru_cache(maxsize=None)
def needs_fix(kind="randtile", w=W, h=H, c=C, q=50, seed=0, ycbcr=True):
    """A stream the reference rejects as it stands (trap T2): decoded under HIMG_OPT_FIX_T2, as test_gpu_region does."""
    return ol.oracle_decode(stream(kind, w, h, c, q, seed, ycbcr))[0] != 0


def origins12(W, H, w, h, rng):
    """Twelve origins of a w x h window: the corners, (7, 7), (8, 8), (5, 3) and seeded random ones."""
    X, Y = W - w, H - h
    o = [(0, 0), (X, Y), (X, 0), (0, Y)] + [(min(a, X), min(b, Y)) for a, b in [(7, 7), (8, 8), (5, 3)]]
    o += [(int(rng.integers(0, X + 1)), int(rng.integers(0, Y + 1))) for _ in range(5)]
    return np.array(o, np.int32)


def _fres(b):
    """(offset of the FRES chunk's size field, the chunk's end): the last chunk of the stream."""
    i = 12
    while True:
        sz = int.from_bytes(b[i + 4:i + 8].tobytes(), "little")
        if b[i:i + 4].tobytes() == b"FRES":
            return i + 4, i + 8 + sz
        i += 8 + sz


def payload_rejected(b, row):
    """b with bits of block row `row`'s payload flipped (seeded) until the oracle rejects that row."""
    offs, lens = himg_amd.index_host(b)[3:5]
    rng = np.random.default_rng(11)
    for _ in range(400):
        d = b.copy()
        for _ in range(3):
            d[int(offs[row]) + int(rng.integers(0, int(lens[row])))] ^= 1 << int(rng.integers(0, 8))
        if dm.expect_rows(b, d, range(row, row + 1), False)[0] == dm.FORMAT:
            return d
    raise AssertionError("no rejected mutation found")


def header_overruns(b, row):
    """b with the size header of block row `row` made to overrun the chunk."""
    offs = himg_amd.index_host(b)[3]
    d = b.copy()
    d[int(offs[row]) - 2], d[int(offs[row]) - 1] = 0xFF, 0x7F
    return d


def surplus_byte(b):
    """b with one byte more in its FRES chunk behind the last block row: half a size header, which only a walk
    to the end of the chunk meets."""
    at, end = _fres(b)
    assert end == len(b)
    d = np.concatenate([b, np.zeros(1, np.uint8)])
    d[at:at + 4] = np.frombuffer(struct.pack("<I", end + 1 - at - 4), np.uint8)
    d[4:8] = np.frombuffer(struct.pack("<I", len(d) - 8), np.uint8)
    return d


def head_damaged(b):
    """b with the QCFG chunk's tag spoilt: the reference fails in a head stage."""
    i = b.tobytes().index(b"QCFG")
    d = b.copy()
    d[i] ^= 0x20
    return d


@functools.lru_cache(maxsize=None)
def independence_cases():
    """{name: (good stream 0, its damaged form, clean stream 1)}."""
    g0, g1 = stream(seed=0).copy(), stream(seed=1).copy()
    return {"payload": (g0, payload_rejected(g0, 4), g1), "header": (g0, header_overruns(g0, 5), g1),
            "cut": (g0, _ends_after_row(g0, 6), g1), "surplus": (g0, surplus_byte(g0), g1),
            "head": (g0, head_damaged(g0), g1)}


def windows():
    """(stream_of, origins): the five windows of YS in stream 0 and in stream 1, interleaved and out of order."""
    so, org = [], []
    for k, (x, y) in enumerate(zip(XS, YS)):
        for s in ((0, 1) if k % 2 else (1, 0)):
            so.append(s)
            org.append((x, y))
    return np.array(so, np.int32), np.array(org, np.int32)


def expected(name):
    """Per window of windows(): (code, crop or None) -- damage_model.expect_region for stream 0's windows (the
    head case: FORMAT for all of them, by the oracle's own head verdict), the clean crop for stream 1's."""
    good, bad, clean = independence_cases()[name]
    so, org = windows()
    out = []
    for s, (x, y) in zip(so, org):
        rect = (int(x), int(y)) + WIN
        if s == 1:
            out.append((dm.OK, full(seed=1)[y:y + WIN[1], x:x + WIN[0]]))
        elif name == "head":
            rc, _ = ol.oracle_decode(bad)
            assert -6 <= rc <= -1, rc
            out.append((dm.FORMAT, None))
        else:
            code, crop, _ = dm.expect_region(good, bad, rect, False)
            out.append((code, crop))
    return out
