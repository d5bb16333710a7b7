"""CPU: the extreme pictures (tests/extreme_pictures.py) reach what they are for -- the saturating
code +-127, forward coefficients above the encoder's 8 192-entry magnitude table, chroma planes at
0 and 255 -- so that a later edit of the generator cannot quietly turn them back into easy pictures.

The forward path is restated here in numpy, per channel: the colour lift (ycbcr.cpp:32-37), the
residual against the interpolated low-res block (interp9) of the ORACLE's low-res plane, the 8 x 8
Walsh-Hadamard transform (hadamard.cpp:18-44, :78-88), the sign-magnitude shift (quantize.cpp:127-151)
and the oracle's own compander.  It is pinned to the oracle's FRES symbols, never to the engine.

tests/golden/extreme_reach.json is what the oracle and this model measure; the test recomputes it.
`python tests/test_extreme_host.py --write` rewrites it."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import extreme_pictures as xp
import oracle_lib as ol
from scaled_model import SCAN, lowres_blocks

REACH_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extreme_reach.json")
SHAPES = [(512, 64), (136, 72)]
QUALITIES = (0, 50, 100)
PIX_LUT = 8192          # kPixLut (himg_amd/csrc/kernels_enc.hip): magnitudes above PIX_LUT - 1 are clamped onto it


def _forward8_matrix():
    """hadamard.cpp:18-44 applied to the unit vectors: out = M @ in."""
    m = np.zeros((8, 8), np.int32)
    for k in range(8):
        i = np.zeros(8, np.int32)
        i[k] = 1
        a = [i[0] + i[4], i[1] + i[5], i[2] + i[6], i[3] + i[7], i[0] - i[4], i[1] - i[5], i[2] - i[6], i[3] - i[7]]
        b = [a[0] + a[2], a[1] + a[3], a[0] - a[2], a[1] - a[3], a[4] + a[6], a[5] + a[7], a[4] - a[6], a[5] - a[7]]
        m[:, k] = [b[0] + b[1], b[4] + b[5], b[6] + b[7], b[2] + b[3], b[2] - b[3], b[6] - b[7], b[4] - b[5], b[0] - b[1]]
    return m


WHT = _forward8_matrix()


def lift(img):
    """ycbcr.cpp:32-37 on channels 0..2; further channels pass."""
    out = img.copy()
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    out[..., 0] = (r + 2 * g + b + 2) >> 2
    out[..., 1] = (b - g + 256) >> 1
    out[..., 2] = (r - g + 256) >> 1
    return out


def tiles_of(plane):
    """encoder.cpp:26-52: [rows][cols][8][8] of a plane [h][w]; a ragged tile repeats its row's last pixel
    to the right and, below its last row, the last pixel it read."""
    h, w = plane.shape
    rows, cols = (h + 7) // 8, (w + 7) // 8
    p = np.empty((rows * 8, cols * 8), np.int32)
    p[:h, :w] = plane
    p[:h, w:] = plane[:, w - 1:w]
    t = p.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).copy()
    if h % 8:
        bw = np.minimum(w - 8 * np.arange(cols), 8)
        t[rows - 1, :, h % 8:, :] = t[rows - 1, np.arange(cols), h % 8 - 1, bw - 1][:, None, None]
    return t


def coefficients(img, ycc, tr):
    """The forward coefficients of every tile in the FRES plane's layout, [rows][C][64][cols] (index 1:
    channel, index 2: position in the coefficient scan), from the picture and the oracle trace's
    low-res plane.  The values must stay inside int16 (255 * 64): asserted."""
    h, w, c = img.shape
    rows, cols = tr["rows"], tr["cols"]
    src = lift(img) if (ycc and c >= 3) else img
    low = tr["lowres"].reshape(c, rows, cols)
    out = np.empty((rows, c, 64, cols), np.int32)
    for ch in range(c):
        res = tiles_of(src[..., ch]) - lowres_blocks(low[ch])
        coef = np.einsum("jy,rcyx,ix->rcji", WHT, res, WHT)                      # rows pass, then columns pass
        assert np.abs(coef).max() <= 32767
        out[:, ch] = coef.reshape(rows, cols, 64)[:, :, SCAN].transpose(0, 2, 1)
    return out


@functools.lru_cache(maxsize=None)
def _compand_table(fmap_bytes):
    fmap = np.frombuffer(fmap_bytes, np.int16).copy()
    f = ol.oracle().himg_oracle_map_to_8bit
    p = fmap.ctypes.data_as(C.c_void_p)
    return np.array([f(p, x) for x in range(32768)], np.uint8)


def symbols(coef, ycc, tr):
    """quantize.cpp:127-151 (the shift keeps the sign apart from the magnitude) and the oracle's
    compander: the FRES symbols of coefficients()."""
    lut = _compand_table(tr["fmap"].tobytes())
    c = coef.shape[1]
    out = np.empty(coef.shape, np.uint8)
    for ch in range(c):
        shift = (tr["shift_chroma"] if (ycc and c >= 3 and ch in (1, 2)) else tr["shift_luma"]).astype(np.int32)[SCAN]
        s = shift[None, :, None]
        mag = (np.abs(coef[:, ch]) + np.where(s > 0, 1 << np.maximum(s - 1, 0), 0)) >> s
        code = lut[mag]
        out[:, ch] = np.where(coef[:, ch] < 0, (-code.view(np.int8)).view(np.uint8), code)
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, w, h, ycc, q):
    """(picture, the oracle's stream, its trace, the model's coefficients, the trace's symbols [rows][C][64][cols] as int8)."""
    img = xp.picture(kind, w, h)
    packed, tr = ol.oracle_encode(img, q, ycc, trace=True)
    coef = coefficients(img, ycc, tr)
    sym = tr["fres_sym"].reshape(coef.shape).view(np.int8)
    return img, packed, tr, coef, sym


MODES = [pytest.param(True, id="ycbcr"), pytest.param(False, id="rgb")]


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", xp.KINDS)
def test_model_is_the_oracles_forward_path(kind, w, h, ycc):
    """At quality 100 every shift is 0, so the companded coefficient IS the symbol; at 50 and 0 the
    shift's rounding is in the way too.  Every kind, and a ragged size for the edge replication."""
    for q in (100, 50, 0):
        img, _, tr, coef, sym = _case(kind, w, h, ycc, q)
        if q == 100:
            assert not tr["shift_luma"].any() and not tr["shift_chroma"].any()
        assert np.array_equal(symbols(coef, ycc, tr).view(np.int8), sym), (kind, w, h, ycc, q)
    img = xp.picture(kind, 100, 52)
    _, tr = ol.oracle_encode(img, 100, ycc, trace=True)
    coef = coefficients(img, ycc, tr)
    assert np.array_equal(symbols(coef, ycc, tr), tr["fres_sym"].reshape(coef.shape)), (kind, "100x52", ycc)


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", ["walsh", "step", "tilecheck"])
def test_both_saturating_codes_occur(kind, w, h, ycc):
    _, _, _, _, sym = _case(kind, w, h, ycc, 100)
    assert (sym == 127).any() and (sym == -127).any(), (kind, w, h, ycc)
    if kind == "walsh":
        for ch in range(4):
            assert (sym[:, ch] == 127).any() and (sym[:, ch] == -127).any(), (w, h, ycc, "channel", ch)


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_step_leaves_the_pixel_stage_table(w, h, ycc):
    """A coefficient whose magnitude is above kPixLut - 1: the clamp of k_pix_fwd and k_front is taken."""
    for q in QUALITIES + (90, 10):
        _, _, _, coef, _ = _case("step", w, h, ycc, q)
        assert np.abs(coef).max() >= PIX_LUT, (w, h, ycc, q, int(np.abs(coef).max()))
    if ycc:   # and in a chroma plane too (G steps against R and B)
        _, _, _, coef, _ = _case("step", w, h, ycc, 100)
        assert np.abs(coef[:, 1:3]).max() >= PIX_LUT, int(np.abs(coef[:, 1:3]).max())


@pytest.mark.parametrize("w,h", SHAPES)
def test_cube_takes_chroma_to_both_ends(w, h):
    ycc = lift(xp.picture("cube", w, h))
    for ch in (1, 2):
        assert ycc[..., ch].min() == 0 and ycc[..., ch].max() == 255, (w, h, ch)
    # ... on pixels whose Y is mid-range
    ends = (ycc[..., 1] == 255) & (ycc[..., 2] == 255)
    assert ends.any() and 120 <= ycc[..., 0][ends].min() and ycc[..., 0][ends].max() <= 136


def test_ties_sit_on_the_rounding_boundary():
    """Quality 50: most quantised values are 0 or +-1, and both signs of 1 occur in every channel."""
    for ycc in (True, False):
        _, _, _, _, sym = _case("ties", 512, 64, ycc, 50)
        assert (np.abs(sym.astype(np.int32)) <= 1).mean() > 0.9
        for ch in range(4):
            assert (sym[:, ch] == 1).any() and (sym[:, ch] == -1).any(), (ycc, ch)


def test_pictures_are_deterministic_and_any_size():
    for kind in xp.KINDS:
        for w, h, c in ((1, 1, 4), (9, 7, 3), (100, 52, 4), (64, 64, 1), (17, 130, 2)):
            a = xp.picture(kind, w, h, c, seed=3)
            assert a.shape == (h, w, c) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
            assert np.array_equal(a, xp.picture(kind, w, h, c, seed=3))
            # the pattern is laid out per tile and cropped: a larger picture begins with the smaller one
            if kind not in ("bin", "ties") and kind != "walsh":
                assert np.array_equal(a, xp.picture(kind, w + 16, h + 8, c, seed=3)[:h, :w])
    assert not np.array_equal(xp.picture("bin", 64, 64, seed=0), xp.picture("bin", 64, 64, seed=1))
    with pytest.raises(ValueError):
        xp.picture("nope", 8, 8)


def test_walsh_bases_and_signs_within_128_tiles():
    """Every basis with both signs in every channel within 128 tiles: as tile patterns, 128 different ones
    per channel, closed under inversion."""
    img = xp.picture("walsh", 1024, 8)      # 128 tiles in one block row
    for ch in range(4):
        pats = {img[:, 8 * t:8 * t + 8, ch].tobytes() for t in range(128)}
        assert len(pats) == 128
        assert {(255 - np.frombuffer(p, np.uint8)).tobytes() for p in pats} == pats


FIELDS = ("max_abs_coefficient", "symbols_plus_127", "symbols_minus_127", "max_abs_symbol", "oracle_decode_rc",
          "oracle_decode_rc_fix_t2")


def reach_table():
    out = {}
    for kind in xp.KINDS:
        for w, h in SHAPES:
            for ycc in (True, False):
                row = {}
                for q in QUALITIES:
                    _, packed, _, coef, sym = _case(kind, w, h, ycc, q)
                    row["q%d" % q] = {"max_abs_coefficient": int(np.abs(coef).max()),
                                      "symbols_plus_127": int((sym == 127).sum()),
                                      "symbols_minus_127": int((sym == -127).sum()),
                                      "max_abs_symbol": int(np.abs(sym.astype(np.int32)).max()),
                                      "oracle_decode_rc": int(ol.oracle_decode(packed)[0]),
                                      "oracle_decode_rc_fix_t2": int(ol.oracle_decode(packed, fix_t2=True)[0])}
                out["%s_%dx%d_%s" % (kind, w, h, "ycbcr" if ycc else "rgb")] = row
    return out


def test_reach_table_is_what_the_oracle_measures():
    with open(REACH_JSON) as f:
        recorded = json.load(f)
    got = reach_table()
    assert recorded["fields"] == list(FIELDS)
    assert sorted(got) == sorted(recorded["rows"])
    for name in got:
        for q in got[name]:
            assert [got[name][q][k] for k in FIELDS] == recorded["rows"][name][q], (name, q)
    # what the GPU tests rely on: rejected streams (trap T2) are among them, and decode in the fixed mode
    rcs = [r[q]["oracle_decode_rc"] for r in got.values() for q in r]
    assert -7 in rcs and 0 in rcs
    assert all(r[q]["oracle_decode_rc_fix_t2"] == 0 for r in got.values() for q in r)


if __name__ == "__main__":
    if "--write" in sys.argv:
        table = reach_table()
        with open(REACH_JSON, "w") as f:   # one line per picture: per quality the values of "fields"
            f.write('{"fields": %s,\n "rows": {\n' % json.dumps(list(FIELDS)))
            f.write(",\n".join('  "%s": %s' % (name, json.dumps({q: [r[k] for k in FIELDS] for q, r in sorted(table[name].items())}))
                                for name in sorted(table)))
            f.write("\n }}\n")
    else:
        print(json.dumps(reach_table(), indent=1, sort_keys=True))
