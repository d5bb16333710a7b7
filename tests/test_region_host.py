"""CPU: the host side of the region decode -- the C entry points, himg_hip_region_peek's plan
against the full row index (himg_amd.index_host) on golden and oracle-encoded streams, the
rectangle checks, and which row headers the bounded walk reads."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import himg_amd
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "*.himg")))
HEADER = os.path.join(os.path.dirname(HERE), "include", "himg_hip.h")
ENTRIES = ("himg_hip_region_peek", "himg_hip_decode_region_to", "himg_hip_decode_region_device")


def _stream(kind, w, h, c=4, q=50, ycbcr=True, seed=0):
    img = himg_amd.synth(kind, seed, w, h)
    if c != img.shape[2]:
        img = np.ascontiguousarray(img[:, :, :c])
    return np.frombuffer(ol.oracle_encode(img, q, ycbcr), np.uint8).copy()


def _rects(W, H):
    out = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1)]
    out += [(min(8, W - 1), min(8, H - 1), 1, 1), (W // 3, H // 3, max(1, W // 3), max(1, H // 3))]
    if H > 9:
        out += [(0, 7, W, 2), (1, 9, W - 1, H - 9)]
    return out


def _check_plan(b, rect, fix_t2=False):
    W, H, Cn, offs, lens, first = himg_amd.index_host(b, fix_t2)
    x, y, w, h = rect
    p = himg_amd.region_peek(b, x, y, w, h, fix_t2)
    r0, r1 = y // 8, (y + h + 7) // 8
    assert (p["width"], p["height"], p["num_channels"]) == (W, H, Cn)
    assert (p["row0"], p["row1"]) == (r0, r1)
    assert p["head_bytes"] == first
    one_row = fix_t2 and (H + 7) // 8 == 1
    hdr = 0 if one_row else (4 if lens[r0] >= 0x8000 else 2)
    assert p["rows_begin"] == offs[r0] - hdr, rect
    assert p["rows_end"] == offs[r1 - 1] + lens[r1 - 1], rect


def test_entries_exported_and_declared():
    L = himg_amd.lib()
    head = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\(" % name, head), name
    assert "himg_hip_region_plan" in head


def test_null_context_is_arg_error():
    L = himg_amd.lib()
    b = np.frombuffer(open(GOLDEN[0], "rb").read(), np.uint8)
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    dst = np.zeros(64, np.uint8)
    assert L.himg_hip_decode_region_to(None, b.ctypes.data, b.nbytes, 0, 0, 1, 1, dst.ctypes.data, dst.nbytes,
                                       C.byref(w), C.byref(h), C.byref(c)) == himg_amd.HIMG_ERR_ARG
    sizes = np.array([b.nbytes], np.uint32)
    assert L.himg_hip_decode_region_device(None, b.ctypes.data, 256, sizes.ctypes.data, 1, 64, 64, 4, 0, 0, 1, 1,
                                           dst.ctypes.data, dst.ctypes.data, None) == himg_amd.HIMG_ERR_ARG
    assert L.himg_hip_region_peek(None, 0, 0, 0, 0, 1, 1, None) == himg_amd.HIMG_ERR_ARG


def test_plan_matches_index_on_golden_streams():
    assert GOLDEN
    for path in GOLDEN:
        b = np.frombuffer(open(path, "rb").read(), np.uint8)
        W, H = himg_amd.index_host(b)[:2]
        for rect in _rects(W, H):
            _check_plan(b, rect)


@pytest.mark.parametrize("kind,w,h,c,q,ycbcr", [
    ("randtile", 16384, 40, 4, 50, True),
    ("rand", 4360, 40, 4, 90, True),
    ("grad", 1920, 40, 3, 100, False),
    ("gradn", 100, 37, 1, 10, True),
    ("randtile", 61, 19, 2, 50, True),
])
def test_plan_matches_index_on_oracle_streams(kind, w, h, c, q, ycbcr):
    b = _stream(kind, w, h, c, q, ycbcr)
    for rect in _rects(w, h):
        _check_plan(b, rect)


def test_one_block_row_stream():
    b = _stream("randtile", 64, 8)
    for fix in (False, True):
        try:
            himg_amd.index_host(b, fix)
        except himg_amd.HimgError:
            continue   # (not indexed this way: region_peek refuses it alike)
        for rect in [(0, 0, 64, 8), (3, 2, 5, 5), (63, 7, 1, 1)]:
            _check_plan(b, rect, fix)


def test_bad_rectangles():
    b = np.frombuffer(open(GOLDEN[0], "rb").read(), np.uint8)
    W, H = himg_amd.index_host(b)[:2]
    for rect in [(0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 1, 1), (0, -1, 1, 1), (W - 1, 0, 2, 1), (0, H - 1, 1, 2),
                 (W, 0, 1, 1), (0, 0, W + 1, H), (1 << 30, 0, 1 << 30, 1)]:
        with pytest.raises(himg_amd.HimgError) as e:
            himg_amd.region_peek(b, *rect)
        assert e.value.code == himg_amd.HIMG_ERR_ARG, rect


def _damage_header(b, row):
    """A copy of b whose row `row` size header claims more bytes than the chunk holds."""
    offs, lens = himg_amd.index_host(b)[3:5]
    d = b.copy()
    hdr = offs[row] - (4 if lens[row] >= 0x8000 else 2)
    d[hdr] = 0xff
    d[hdr + 1] = 0x7f
    if lens[row] >= 0x8000:
        d[hdr + 1] = 0xff
        d[hdr + 2] = 0xff
        d[hdr + 3] = 0xff
    return d


def test_damaged_header_after_r1_not_seen():
    b = _stream("randtile", 256, 64)   # 8 block rows
    rows = 8
    with pytest.raises(himg_amd.HimgError):
        himg_amd.index_host(_damage_header(b, 5))
    d = _damage_header(b, 5)
    p = himg_amd.region_peek(d, 0, 0, 256, 40)     # rows 0 .. 4: the header of row 5 is not read
    assert (p["row0"], p["row1"]) == (0, 5)
    _check_plan(b, (0, 0, 256, 40))
    assert p["rows_end"] == himg_amd.region_peek(b, 0, 0, 256, 40)["rows_end"]
    for rect in [(0, 0, 256, 41), (0, 40, 8, 8), (0, 0, 256, 64)]:   # rows up to 5 or the whole frame: seen
        with pytest.raises(himg_amd.HimgError) as e:
            himg_amd.region_peek(d, *rect)
        assert e.value.code == himg_amd.HIMG_ERR_FORMAT, rect
    d = _damage_header(b, 2)
    with pytest.raises(himg_amd.HimgError) as e:
        himg_amd.region_peek(d, 0, 40, 8, 8)   # row 5: the walk passes row 2's header
    assert e.value.code == himg_amd.HIMG_ERR_FORMAT
    assert rows == (64 + 7) // 8


def test_chunk_ending_behind_the_last_touched_row():
    """A FRES chunk cut right behind row r1 - 1: the plan is whole for rectangles above that row, and a
    rectangle that reaches it finds the missing header."""
    b = _stream("randtile", 256, 64)
    offs, lens = himg_amd.index_host(b)[3:5]
    end = int(offs[4]) + int(lens[4])
    d = b[:end].copy()
    i = 12
    while True:
        sz = int.from_bytes(d[i + 4:i + 8].tobytes(), "little")
        if d[i:i + 4].tobytes() == b"FRES":
            d[i + 4:i + 8] = np.frombuffer((end - i - 8).to_bytes(4, "little"), np.uint8)
            break
        i += 8 + sz
    d[4:8] = np.frombuffer((end - 8).to_bytes(4, "little"), np.uint8)
    p = himg_amd.region_peek(d, 0, 0, 256, 40)
    assert (p["row1"], p["rows_end"]) == (5, end)
    with pytest.raises(himg_amd.HimgError) as e:
        himg_amd.region_peek(d, 0, 0, 256, 41)
    assert e.value.code == himg_amd.HIMG_ERR_FORMAT
