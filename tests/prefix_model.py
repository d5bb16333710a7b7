"""The decode of a stream prefix (himg_hip_decode_prefix_*) as its definition in include/himg_hip.h, in
numpy and plain Python: the walk over the bytes present, and the picture -- block rows below k from the
oracle's decode of the whole stream, the others from the oracle decoder's low-res plane through
scaled_model.lowres_blocks, a clamp and scaled_model.ycc_to_rgb.

Test infrastructure only.
"""
import struct

import numpy as np

import oracle_lib as ol
import scaled_model as sm

OK, FORMAT, CAPACITY = 0, -4, -5
TREE_STAGE = 384        # bytes of a chunk the container parse looks at (kTreeStride)
MAX_NODES = 2 * 261 - 1


class _Short(Exception):
    """The walk needs a byte that is not present."""


class _Format(Exception):
    """A check of the decoder fails on bytes that are present."""


def _u32(b, i):
    return struct.unpack_from("<I", b, i)[0]


def empty_plan():
    return dict(width=0, height=0, num_channels=0, rows=0, rows_complete=0, packed_size=0, head_bytes=0,
                used_bytes=0, next_bytes=0)


def _head(b, fix_t2, p):
    """The chunk headers and the length of the FRES tree: (first row header, end of the FRES chunk)."""
    avail = len(b)
    if avail < 12:
        raise _Short
    T = _u32(b, 4) + 8
    if b[0:4] != b"RIFF" or T > 0x7fffffff or T < 12 or b[8:12] != b"HIMG":
        raise _Format
    p["packed_size"] = T
    if avail > T:
        raise _Format
    state = {"idx": 12, "need": 0}

    def find(tag):
        while True:
            i = state["idx"]
            if i + 8 > T:
                raise _Format
            if i + 8 > avail:
                raise _Short
            hit, sz = b[i:i + 4] == tag, _u32(b, i + 4)
            state["idx"] = i = i + 8
            if sz > 0x7fffffff or i + sz > T:
                raise _Format
            if hit:
                return sz
            state["idx"] = i + sz

    try:
        sz = find(b"FRMT")
        i = state["idx"]
        if sz < 11:
            raise _Format
        if i + 11 > avail:
            raise _Short
        if b[i] != 1:
            raise _Format
        W, H, C = _u32(b, i + 1), _u32(b, i + 5), b[i + 9]
        ycc = b[i + 10] != 0 and C >= 3
        p.update(width=W, height=H, num_channels=C, rows=(H + 7) // 8)
        state["idx"] = i + sz
        for tag in (b"LMAP", b"LRES", b"QCFG", b"FMAP"):
            sz = find(tag)
            if tag == b"QCFG" and sz != (64 if ycc else 32):
                raise _Format
            state["need"] = max(state["need"], state["idx"] + min(sz, TREE_STAGE))
            state["idx"] += sz
        csz = find(b"FRES")
        if not fix_t2 and not ((W + 7) // 8 * C * 64 < csz):   # trap T2
            raise _Format
    except _Format:
        # The decoder reports the first failure in ITS order of checks: a chunk in front that is not
        # whole below avail may hold an earlier one.
        if state["need"] > avail:
            raise _Short
        raise
    coff = state["idx"]
    cnt = min(csz, TREE_STAGE)
    have = max(0, min(avail - coff, cnt))
    bit, opened, count = 0, 1, 0
    while opened > 0:
        if count >= MAX_NODES or bit >= 8 * cnt:
            raise _Format
        if (bit >> 3) >= have:
            raise _Short
        count += 1
        if (b[coff + (bit >> 3)] >> (bit & 7)) & 1:
            if bit + 10 > 8 * cnt:
                raise _Format
            bit += 10
            opened -= 1
        else:
            bit += 1
            opened += 1
    tb = (bit + 7) >> 3
    q, end = coff + tb, coff + csz
    if q >= end:
        raise _Format
    p["head_bytes"] = q
    if tb > have:
        raise _Short
    return q, end


def _rows(b, fix_t2, p, q, end, upto=None, ranges=None):
    """The row headers from q by the decoder's rules (huffman_dec.cpp:232-248), for as long as a header and
    its payload lie wholly in b.  upto (a region's r1, below the frame's rows): the walk stops behind that
    many headers; None walks to the end of the chunk, as the full decode does.  ranges (a list): receives
    (payload offset, length) of every row the walk delimits, at most the frame's rows."""
    avail, T, rows = len(b), p["packed_size"], p["rows"]
    if upto is None or upto >= rows:
        upto = None
    p.update(rows_complete=0, used_bytes=q, next_bytes=T)
    if fix_t2 and rows == 1:   # one block row has no size header
        if end <= avail:
            p.update(rows_complete=1, used_bytes=end)
            if ranges is not None:
                ranges.append((q, end - q))
        else:
            p["next_bytes"] = end
        return
    r, cut = 0, False
    while q != end and (upto is None or r < upto):
        if q + 2 > end:
            raise _Format
        if q + 2 > avail:
            cut, p["next_bytes"] = True, q + 2
            break
        n, body = b[q] | (b[q + 1] << 8), q + 2
        if n & 0x8000:
            if body + 2 > end:
                raise _Format
            if body + 2 > avail:
                cut, p["next_bytes"] = True, body + 2
                break
            n = (n & 0x7fff) | ((b[body] | (b[body + 1] << 8)) << 15)
            body += 2
        if n > end - body:
            raise _Format
        if body + n > avail:
            cut, p["next_bytes"] = True, body + n
            break
        if r < rows:
            p["used_bytes"] = body + n
            if ranges is not None:
                ranges.append((body, n))
        r += 1
        q = body + n
    if not cut and r < (rows if upto is None else upto):
        raise _Format   # fewer blocks than block rows (than the rows asked for)
    p["rows_complete"] = min(r, rows)
    if p["rows_complete"] == rows:
        p["next_bytes"] = T


def walk(packed, avail=None, fix_t2=False):
    """(code, plan) of the first `avail` bytes of `packed`: nothing behind them is looked at."""
    b = bytes(np.asarray(packed, np.uint8)[:avail].tobytes()) if not isinstance(packed, bytes) else packed[:avail]
    p = empty_plan()
    try:
        q, end = _head(b, fix_t2, p)
        _rows(b, fix_t2, p, q, end)
    except _Short:
        return CAPACITY, p
    except _Format:
        return FORMAT, p
    return OK, p


def fill_picture(low, W, H, C, ycc):
    """The picture of a frame whose symbols are all zero: every tile its interpolated low-res block,
    clamped, through the colour inverse, clipped to W x H.  low: [C][rows][cols]."""
    rows, cols = (H + 7) // 8, (W + 7) // 8
    low = np.asarray(low).reshape(C, rows, cols)
    out = np.empty((rows * 8, cols * 8, C), np.uint8)
    for c in range(C):
        blk = np.clip(sm.lowres_blocks(low[c]), 0, 255)                        # [rows][cols][8][8]
        out[:, :, c] = blk.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)
    out = np.ascontiguousarray(out[:H, :W])
    return sm.ycc_to_rgb(out) if ycc else out


def stream_ycc(packed):
    b = bytes(np.asarray(packed, np.uint8).tobytes())
    o, _ = sm.find_chunks(b)["FRMT"]
    return b[o + 10] != 0 and b[o + 9] >= 3


class Model:
    """One stream the decoder accepts: its full decode and its all-zero picture, computed once."""

    def __init__(self, packed, fix_t2=False):
        self.packed = np.ascontiguousarray(packed, np.uint8)
        self.fix_t2 = fix_t2
        ol.oracle().himg_oracle_set_compat_fix(1 if fix_t2 else 0)
        try:
            rc, tr = ol.oracle_decode_trace(self.packed)
        finally:
            ol.oracle().himg_oracle_set_compat_fix(0)
        assert rc == 0, "the model needs a stream the decoder accepts"
        self.full = tr["pixels"]
        self.H, self.W, self.C = self.full.shape
        self.rows = (self.H + 7) // 8
        self.fill = fill_picture(tr["lowres"], self.W, self.H, self.C, stream_ycc(self.packed))
        self.T = self.packed.size
        self.plan = walk(self.packed, self.T, fix_t2)[1]

    def row_ends(self):
        """used_bytes for k = 0 .. rows: where each prefix of whole rows ends."""
        out, a = [self.plan["head_bytes"]], self.plan["head_bytes"]
        while len(out) <= self.rows:
            p = walk(self.packed, a, self.fix_t2)[1]
            while p["rows_complete"] < len(out):   # behind the next header (in one or two steps), then behind its payload
                assert p["next_bytes"] > a
                a = p["next_bytes"]
                p = walk(self.packed, a, self.fix_t2)[1]
            assert p["rows_complete"] == len(out) and p["used_bytes"] == a
            out.append(a)
        return out

    def picture(self, k):
        out = self.fill.copy()
        out[:8 * k] = self.full[:8 * k]
        return out

    def expect(self, avail):
        """(code, k or -1, picture or None) of the first avail bytes."""
        code, p = walk(self.packed, avail, self.fix_t2)
        if code:
            return code, -1, None
        return OK, p["rows_complete"], self.picture(p["rows_complete"])
