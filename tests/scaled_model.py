"""The scaled decode (himg_hip_decode_scaled_*) as its definition in include/himg_hip.h, in numpy:
from the oracle decoder's trace of a stream (the FRES symbols [rows][C][64][cols] and the
decoder's low-res plane), the stream's own QCFG and FMAP chunks and FRMT's colour space.

Test infrastructure only.  scale_log2 in (1, 2): F = 2 ** scale_log2 pixels per sample and side,
S = 8 // F coefficients per tile and side.
"""
import struct

import numpy as np

import oracle_lib as ol

# The coefficient scan (the format's table): position in the 8 x 8 block
# (row-major) of scan index k.  Its first S * S entries are the top-left S x S, for S = 2 and 4.
SCAN = np.array([0, 1, 9, 8, 16, 17, 18, 10, 2, 3, 11, 19, 27, 26, 25, 24,
                 32, 33, 34, 35, 36, 28, 20, 12, 4, 5, 13, 21, 29, 37, 45, 44,
                 43, 42, 41, 40, 48, 49, 50, 51, 52, 53, 54, 46, 38, 30, 22, 14,
                 6, 7, 15, 23, 31, 39, 47, 55, 63, 62, 61, 60, 59, 58, 57, 56])

# The S-point sequency-ordered Walsh matrices: WALSH[S][i][X] = w_i(X).
WALSH = {4: np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int32),
         2: np.array([[1, 1], [1, -1]], np.int32)}


def find_chunks(packed):
    """The chunks as the decoder's forward search meets them, each from behind the one before:
    {tag: (offset of the body, size)} for FRMT, LMAP, LRES, QCFG, FMAP, FRES (None: not found)."""
    b = bytes(packed)
    out, i = {}, 12
    for tag in (b"FRMT", b"LMAP", b"LRES", b"QCFG", b"FMAP", b"FRES"):
        while True:
            if i + 8 > len(b):
                return None
            hit = b[i:i + 4] == tag
            sz = struct.unpack("<i", b[i + 4:i + 8])[0]
            i += 8
            if sz < 0 or i + sz > len(b):
                return None
            if hit:
                out[tag.decode()] = (i, sz)
                i += sz
                break
            i += sz
    return out


def stream_tables(packed):
    """(ycbcr in effect, shift_luma[64], shift_chroma[64], unmap[256]) of a stream the decoder accepts:
    QCFG's nibbles, the FMAP table (n one-byte entries, then two-byte ones) mirrored onto the code
    byte as the decoder's unmap does (code -128 takes entry 127)."""
    b = bytes(packed)
    ch = find_chunks(b)
    o, _ = ch["FRMT"]
    channels, ycc = b[o + 9], b[o + 10] != 0 and b[o + 9] >= 3
    o, sz = ch["QCFG"]
    q = np.frombuffer(b[o:o + sz], np.uint8)
    nib = lambda a: np.stack([a >> 4, a & 15], 1).reshape(64).astype(np.int32)
    shift_l = nib(q[:32])
    shift_c = nib(q[32:64]) if ycc else np.zeros(64, np.int32)
    o, sz = ch["FMAP"]
    n1 = b[o]
    assert 1 + n1 + 2 * (127 - n1) == sz
    t = np.zeros(128, np.int32)
    t[1:1 + n1] = np.frombuffer(b[o + 1:o + 1 + n1], np.uint8)
    t[1 + n1:] = np.frombuffer(b[o + 1 + n1:o + sz], "<u2").astype(np.uint16).view(np.int16)
    code = np.arange(256).astype(np.uint8).view(np.int8).astype(np.int32)
    mag = t[np.minimum(np.abs(code), 127)]
    unmap = np.where(code >= 0, mag, -mag).astype(np.int16).astype(np.int32)
    return channels, ycc, shift_l, shift_c, unmap


def _i16(x):
    return x.astype(np.int16).astype(np.int32)


def _interp9(a0, a8):
    a = [None] * 9
    a[0], a[8] = a0, a8
    a[4] = (a[0] + a[8] + 1) >> 1
    a[2] = (a[0] + a[4] + 1) >> 1
    a[6] = (a[4] + a[8] + 1) >> 1
    a[1] = (a[0] + a[2] + 1) >> 1
    a[3] = (a[2] + a[4] + 1) >> 1
    a[5] = (a[4] + a[6] + 1) >> 1
    a[7] = (a[6] + a[8] + 1) >> 1
    return a


def lowres_blocks(m):
    """The interpolated low-res block of every tile of a plane m[rows][cols]: [rows][cols][8][8]."""
    m = m.astype(np.int32)
    rows, cols = m.shape
    v2 = np.minimum(np.arange(rows) + 1, rows - 1)
    u2 = np.minimum(np.arange(cols) + 1, cols - 1)
    left = _interp9(m, m[v2])
    right = _interp9(m[:, u2], m[v2][:, u2])
    out = np.empty((rows, cols, 8, 8), np.int32)
    for y in range(8):
        a = _interp9(left[y], right[y])
        for x in range(8):
            out[:, :, y, x] = a[x]
    return out


def ycc_to_rgb(p):
    """The colour inverse in int16 arithmetic, then the clamp; channels 3.. pass."""
    p = p.copy()
    y = p[..., 0].astype(np.int16)
    cb = (p[..., 1].astype(np.int16) << 1) - 255
    cr = (p[..., 2].astype(np.int16) << 1) - 255
    g = y - ((cb + cr + 2) >> 2)
    b = g + cb
    r = g + cr
    p[..., 0], p[..., 1], p[..., 2] = (np.clip(v, 0, 255).astype(np.uint8) for v in (r, g, b))
    return p


def short_inverse(d, S):
    """Steps 1's output d[..., j, i] (int32 holding int16 values) through both short passes:
    p[..., Y, X]."""
    w = WALSH[S]
    t = _i16(np.einsum("...ji,ix->...jx", d, w) >> 3)
    return _i16(np.einsum("...jx,jy->...yx", t, w) >> 3)


def scaled_from_trace(tr, packed, scale_log2, band=64):
    """The scaled picture [oh][ow][C] from a decode trace of `packed`."""
    S, F = 8 >> scale_log2, 1 << scale_log2
    h, w, c = tr["pixels"].shape
    rows, cols = (h + 7) // 8, (w + 7) // 8
    channels, ycc, shift_l, shift_c, unmap = stream_tables(packed)
    assert channels == c
    sym = tr["fres_sym"].reshape(rows, c, 64, cols)
    low = tr["lowres"].reshape(c, rows, cols)
    pos = SCAN[:S * S]
    oh, ow = (h + F - 1) // F, (w + F - 1) // F
    out = np.zeros((rows * S, cols * S, c), np.uint8)
    for r0 in range(0, rows, band):   # bands of block rows: a 16384^2 frame stays within memory
        r1 = min(rows, r0 + band)
        for ch in range(c):
            shift = shift_c if (ycc and ch in (1, 2)) else shift_l
            d = np.zeros((r1 - r0, cols, 8, 8), np.int32)
            for k in range(S * S):
                j, i = pos[k] >> 3, pos[k] & 7
                d[:, :, j, i] = _i16(unmap[sym[r0:r1, ch, k, :]] * (1 << int(shift[pos[k]])))
            p = short_inverse(d[:, :, :S, :S], S)
            lb = _lowres_band(low[ch], r0, r1)
            L = (lb.reshape(r1 - r0, cols, S, F, S, F).sum(axis=(3, 5)) + F * F // 2) >> (2 * scale_log2)
            smp = np.clip(_i16(p + L), 0, 255).astype(np.uint8)          # [r][u][Y][X]
            out[r0 * S:r1 * S, :, ch] = smp.transpose(0, 2, 1, 3).reshape((r1 - r0) * S, cols * S)
    out = out[:oh, :ow]
    if ycc:
        out = ycc_to_rgb(out)
    return np.ascontiguousarray(out)


def _lowres_band(m, r0, r1):
    """lowres_blocks of rows [r0, r1) only: with the row below, or, at the plane's last row, the
    clamp onto itself."""
    return lowres_blocks(m[r0:min(m.shape[0], r1 + 1)])[:r1 - r0]


def expected(packed, scale_log2, fix=False):
    """(the oracle's rc for the full decode, the scaled picture or None)."""
    ol.oracle().himg_oracle_set_compat_fix(1 if fix else 0)
    try:
        rc, tr = ol.oracle_decode_trace(packed)
    finally:
        ol.oracle().himg_oracle_set_compat_fix(0)
    if rc != 0:
        return rc, None
    return 0, scaled_from_trace(tr, packed, scale_log2)


def box_mean(img, scale_log2):
    """The rounded F x F box mean of a picture [h][w][c], edge boxes over the pixels present."""
    F = 1 << scale_log2
    h, w, c = img.shape
    oh, ow = (h + F - 1) // F, (w + F - 1) // F
    pad = np.zeros((oh * F, ow * F, c), np.int64)
    cnt = np.zeros((oh * F, ow * F, 1), np.int64)
    pad[:h, :w] = img
    cnt[:h, :w] = 1
    s = pad.reshape(oh, F, ow, F, c).sum(axis=(1, 3))
    n = cnt.reshape(oh, F, ow, F, 1).sum(axis=(1, 3))
    return ((2 * s + n) // (2 * n)).astype(np.uint8)


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean())
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


CLOSENESS_KINDS = ("randtile", "rand", "gradn")
CLOSENESS_SIZES = (256, 512)
CLOSENESS_Q = (10, 50, 90, 100)


def closeness_table(synth):
    """The closeness measurement: per picture, quality, colour space and scale the
    model M against T = the rounded box mean of the oracle's full decode and O = the same box
    mean of the original.  Streams the reference decoder rejects are left out (listed as such)."""
    rows = []
    for size in CLOSENESS_SIZES:
        for kind in CLOSENESS_KINDS:
            img = synth(kind, 3, size, size)
            for ycc in (0, 1):
                for q in CLOSENESS_Q:
                    packed = ol.oracle_encode(img, q, bool(ycc))
                    rc, tr = ol.oracle_decode_trace(packed)
                    for s in (1, 2):
                        row = {"kind": kind, "size": size, "q": q, "colour_space": ycc, "scale_log2": s}
                        if rc != 0:
                            row["rejected_by_reference"] = int(rc)
                            rows.append(row)
                            continue
                        M = scaled_from_trace(tr, packed, s)
                        T, O = box_mean(tr["pixels"], s), box_mean(img, s)
                        row.update(max_abs_M_T=int(np.abs(M.astype(np.int32) - T).max()),
                                   psnr_M_T=round(psnr(M, T), 4), psnr_T_O=round(psnr(T, O), 4),
                                   psnr_M_O=round(psnr(M, O), 4))
                        rows.append(row)
    return rows
