"""CPU: the host side of the 1/8-scale preview (himg_hip_preview_peek) on the golden streams
-- the preview's geometry, where the LRES chunk ends, and the verdict of the reference's
first three stages plus the search for LRES (decoder.cpp:95-118, 428-461)."""
import glob
import os
import struct

import numpy as np
import pytest

import himg_amd
import oracle_lib as ol

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*.himg")))


def _walk(b):
    """[(tag, body offset, size)] of the chunks behind the RIFF header."""
    out, i = [], 12
    while i + 8 <= len(b):
        sz = struct.unpack("<I", b[i + 4:i + 8])[0]
        out.append((b[i:i + 4], i + 8, sz))
        i += 8 + sz
    return out


def _lres_end(b):
    for tag, off, sz in _walk(b):
        if tag == b"LRES":
            return off + sz
    raise AssertionError("no LRES chunk")


def _frmt(b):
    for tag, off, sz in _walk(b):
        if tag == b"FRMT":
            w, h = struct.unpack("<II", b[off + 1:off + 9])
            return w, h, b[off + 9]
    raise AssertionError("no FRMT chunk")


def test_golden_streams():
    assert GOLDEN
    for path in GOLDEN:
        b = open(path, "rb").read()
        w, h, c = _frmt(b)
        pw, ph, pc, head = himg_amd.preview_peek(b)
        assert (pw, ph, pc) == ((w + 7) // 8, (h + 7) // 8, c), path
        assert head == _lres_end(b), path
        assert 0 < head < len(b)


def _code(fn):
    with pytest.raises(himg_amd.HimgError) as e:
        fn()
    return e.value


def test_bad_riff():
    b = bytearray(open(GOLDEN[0], "rb").read())
    bad = bytearray(b)
    bad[0] ^= 1                                  # magic
    assert _code(lambda: himg_amd.preview_peek(bad)).code == himg_amd.HIMG_ERR_FORMAT
    bad = bytearray(b)
    bad[4] ^= 4                                  # RIFF size: file_size + 8 != packed_size
    assert _code(lambda: himg_amd.preview_peek(bad)).code == himg_amd.HIMG_ERR_FORMAT
    # the RIFF check needs the whole stream's size, not the bytes present
    assert _code(lambda: himg_amd.preview_peek(b, packed_size=len(b) - 1)).code == himg_amd.HIMG_ERR_FORMAT
    bad = bytearray(b)
    bad[8] ^= 1                                  # HIMG
    assert _code(lambda: himg_amd.preview_peek(bad)).code == himg_amd.HIMG_ERR_FORMAT


def test_bad_frmt_and_lmap():
    b = bytes(open(GOLDEN[0], "rb").read())
    ch = {t: (o, s) for t, o, s in _walk(b)}
    bad = bytearray(b)
    bad[ch[b"FRMT"][0]] = 2                      # version
    assert _code(lambda: himg_amd.preview_peek(bad)).code == himg_amd.HIMG_ERR_FORMAT
    assert ol.oracle_decode(np.frombuffer(bytes(bad), np.uint8))[0] == -2
    bad = bytearray(b)
    bad[ch[b"LMAP"][0]] ^= 1                     # single-byte items: the table's size no longer matches
    assert _code(lambda: himg_amd.preview_peek(bad)).code == himg_amd.HIMG_ERR_FORMAT
    assert ol.oracle_decode(np.frombuffer(bytes(bad), np.uint8))[0] == -3
    bad = bytearray(b)
    o = ch[b"LRES"][0] - 8
    bad[o:o + 4] = b"XRES"                       # no LRES chunk: the search runs off the end
    assert _code(lambda: himg_amd.preview_peek(bad)).code == himg_amd.HIMG_ERR_FORMAT
    assert ol.oracle_decode(np.frombuffer(bytes(bad), np.uint8))[0] == -4


def test_capacity_until_the_head_is_present():
    for path in GOLDEN:
        b = open(path, "rb").read()
        head = _lres_end(b)
        lres_hdr = head - dict((t, s) for t, _, s in _walk(b))[b"LRES"]   # end of the LRES header
        for avail in (0, 11, 12, 40, lres_hdr - 1):
            e = _code(lambda: himg_amd.preview_peek(b[:avail], packed_size=len(b)))
            assert e.code == himg_amd.HIMG_ERR_CAPACITY and e.head_bytes == 0, (path, avail)
        for avail in (lres_hdr, head - 1):
            e = _code(lambda: himg_amd.preview_peek(b[:avail], packed_size=len(b)))
            assert e.code == himg_amd.HIMG_ERR_CAPACITY and e.head_bytes == head, (path, avail)
        # the bytes behind avail are never looked at
        junk = bytearray(b)
        junk[head:] = b"\xff" * (len(b) - head)
        r = himg_amd.preview_peek(junk, avail=head)
        assert r[3] == head
        assert himg_amd.preview_peek(b[:head], packed_size=len(b)) == himg_amd.preview_peek(b)


def test_unknown_chunk_before_lres_is_skipped():
    b = bytes(open([p for p in GOLDEN if p.endswith("randtile_s0_64x64_q50.himg")][0], "rb").read())
    assert ol.oracle_decode(np.frombuffer(b, np.uint8))[0] == 0
    ch = {t: (o, s) for t, o, s in _walk(b)}
    at = ch[b"LRES"][0] - 8
    extra = b"JUNK" + struct.pack("<I", 6) + b"abcdef"
    s = bytearray(b[:at] + extra + b[at:])
    s[4:8] = struct.pack("<I", len(s) - 8)       # RIFF size fixed up
    rc, pix = ol.oracle_decode(np.frombuffer(bytes(s), np.uint8))
    assert rc == 0
    pw, ph, c, head = himg_amd.preview_peek(s)
    assert head == _lres_end(b) + len(extra)
    assert (pw, ph, c) == himg_amd.preview_peek(b)[:3]
