"""The model of the planes decode: the stream's own channel planes, taken from the oracle as it
stands.  A stream is rewritten so that the oracle applies no colour inverse (FRMT byte 10 = 0) and
dequantises every channel with ONE table: the 64-byte QCFG body becomes 32 bytes -- bytes 0..31 (the
luma table) for planes 0 and 3, bytes 32..63 (the chroma table) for planes 1 and 2.  Channel c of the
oracle's decode of the rewritten stream is plane c: the byte the reference decoder holds for that
channel immediately before YCbCrToRGB (decoder.cpp:372-423).  The FRES chunk keeps its size, so the
T2 verdict is the original stream's.  For colour space 0 or C < 3 the model is the oracle's decode.

Test infrastructure only -- nothing under himg_amd/ imports this module."""
import numpy as np

import oracle_lib as ol


def header(stream):
    """(W, H, C, colour space) from the FRMT chunk."""
    s = np.ascontiguousarray(stream, np.uint8)
    off = ol.chunk_payloads(s)["FRMT"][0]
    w = int.from_bytes(s[off + 1:off + 5].tobytes(), "little")
    h = int.from_bytes(s[off + 5:off + 9].tobytes(), "little")
    return w, h, int(s[off + 9]), int(s[off + 10])


def rewrite(stream, chroma):
    """The stream with colour space 0 and a 32-byte QCFG: its luma table, or (chroma) its chroma table."""
    s = np.ascontiguousarray(stream, np.uint8)
    ch = ol.chunk_payloads(s)
    frmt, (q_off, q_size) = ch["FRMT"][0], ch["QCFG"]
    assert q_size == 64 and s[frmt + 10] != 0, "a colour-space-1 stream of three or four channels"
    body = s[q_off + 32:q_off + 64] if chroma else s[q_off:q_off + 32]
    out = np.concatenate([s[:q_off], body, s[q_off + 64:]]).copy()
    out[frmt + 10] = 0
    out[q_off - 4:q_off] = np.frombuffer((32).to_bytes(4, "little"), np.uint8)
    out[4:8] = np.frombuffer((out.size - 8).to_bytes(4, "little"), np.uint8)
    return out


def planes(stream, fix_t2=False):
    """(rc, planes): the oracle's verdict on the stream under that mode and, when it decodes, its
    [C][H][W] planes."""
    w, h, c, cs = header(stream)
    if cs == 0 or c < 3:
        rc, img = ol.oracle_decode(stream, fix_t2=fix_t2)
        return rc, (None if rc else np.ascontiguousarray(img.reshape(h, w, c).transpose(2, 0, 1)))
    rc_l, luma = ol.oracle_decode(rewrite(stream, False), fix_t2=fix_t2)
    rc_c, chro = ol.oracle_decode(rewrite(stream, True), fix_t2=fix_t2)
    assert rc_l == rc_c
    if rc_l:
        return rc_l, None
    luma, chro = luma.reshape(h, w, c), chro.reshape(h, w, c)
    out = np.empty((c, h, w), np.uint8)
    for k in range(c):
        out[k] = (chro if k in (1, 2) else luma)[:, :, k]
    return 0, out


def select(pl, mask):
    """The planes of `mask` in ascending channel order: [P][H][W]."""
    return np.ascontiguousarray(pl[[c for c in range(pl.shape[0]) if (mask >> c) & 1]])


def to_picture(pl, colour_space):
    """The interleaved [H][W][C] picture behind the colour inverse (ycbcr.cpp:54-82) of [C][H][W] planes."""
    c = pl.shape[0]
    out = np.ascontiguousarray(pl.transpose(1, 2, 0)).copy()
    if colour_space and c >= 3:
        y = pl[0].astype(np.int32)
        cb = (pl[1].astype(np.int32) << 1) - 255
        cr = (pl[2].astype(np.int32) << 1) - 255
        g = y - ((cb + cr + 2) >> 2)
        out[:, :, 0] = np.clip(g + cr, 0, 255)
        out[:, :, 1] = np.clip(g, 0, 255)
        out[:, :, 2] = np.clip(g + cb, 0, 255)
    return out
