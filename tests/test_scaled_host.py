"""CPU (-m "not gpu"): the host side of the scaled decode -- himg_hip_scaled_size, the exported
symbols, the sequency argument the feature rests on (pinned against the oracle's inverse
transform), and how close the decode at 1/2 and 1/4 scale is to the shrunken full decode."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import himg_amd
import oracle_lib as ol
import scaled_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scaled_size():
    for w, h in [(1, 1), (2, 3), (7, 9), (8, 8), (517, 61), (1920, 1080), (4096, 4096), (16384, 16383), (2147483647, 5)]:
        for s in (1, 2):
            f = 1 << s
            assert himg_amd.scaled_size(w, h, s) == ((w + f - 1) // f, (h + f - 1) // f)
    for bad in [(8, 8, 0), (8, 8, 3), (8, 8, -1), (0, 8, 1), (8, 0, 2), (-4, 8, 1)]:
        with pytest.raises(himg_amd.HimgError) as e:
            himg_amd.scaled_size(*bad)
        assert e.value.code == himg_amd.HIMG_ERR_ARG
    ow, oh = C.c_int(), C.c_int()
    assert himg_amd.lib().himg_hip_scaled_size(8, 8, 1, None, C.byref(oh)) == himg_amd.HIMG_ERR_ARG
    assert himg_amd.lib().himg_hip_scaled_size(8, 8, 1, C.byref(ow), None) == himg_amd.HIMG_ERR_ARG


def test_symbols_exported():
    L = himg_amd.lib()
    for name in ("himg_hip_scaled_size", "himg_hip_decode_scaled_device", "himg_hip_decode_scaled_to",
                 "himg_hip_decode_scaled_batch"):
        assert getattr(L, name) is not None
    for name in ("scaled_size",):
        assert callable(getattr(himg_amd, name))
    for name in ("decode_scaled", "decode_scaled_batch", "decode_scaled_device"):
        assert callable(getattr(himg_amd.Engine, name))


def test_scan_prefix_is_the_top_left_square():
    """The first S * S scan positions are exactly the top-left S x S (what makes a channel's needed
    symbols a contiguous prefix of its 64 segments)."""
    for S in (2, 4):
        want = sorted(8 * j + i for j in range(S) for i in range(S))
        assert sorted(int(p) for p in sm.SCAN[:S * S]) == want
    assert sorted(int(p) for p in sm.SCAN) == list(range(64))


@pytest.mark.parametrize("S", [4, 2])
def test_box_means_of_the_inverse_are_the_short_transform(S):
    """Blocks whose only non-zero coefficients are multiples of 64 in the top-left S x S: every
    F x F box of the oracle's 8 x 8 inverse transform is constant and equals the S-point transform."""
    F = 8 // S
    rng = np.random.default_rng(100 + S)
    inv = ol.oracle().himg_oracle_hadamard_inverse
    for _ in range(200):
        blk = np.zeros((8, 8), np.int16)
        blk[:S, :S] = 64 * rng.integers(-40, 41, (S, S))
        out = np.zeros((8, 8), np.int16)
        inv(out.ctypes.data_as(C.c_void_p), blk.ctypes.data_as(C.c_void_p))
        boxes = out.reshape(S, F, S, F).transpose(0, 2, 1, 3).reshape(S, S, F * F)
        assert (boxes == boxes[:, :, :1]).all()
        short = sm.short_inverse(blk[:S, :S].astype(np.int32), S)
        assert np.array_equal(short, boxes[:, :, 0].astype(np.int32))


def test_model_of_zero_residual_is_the_low_res_box_mean():
    """A flat picture (every FRES symbol zero; the fixed mode decodes it): the model is the box mean
    of the interpolated low-res blocks, which for a flat plane is the plane's value."""
    img = np.full((40, 72, 4), 93, np.uint8)
    packed = ol.oracle_encode(img, 50, False)
    for s in (1, 2):
        rc, m = sm.expected(packed, s, fix=True)
        assert rc == 0 and m.shape == (40 >> s, 72 >> s, 4) and (m == 93).all()


def test_closeness_to_the_shrunken_full_decode():
    """Measured, not assumed: M (the scaled decode's model) against T (the rounded box mean of the
    oracle's full decode) and O (the same of the original).  Asserted, for q <= 90:
    PSNR(M, T) > PSNR(T, O) -- the scaled decode differs from the shrunken full decode by less than
    the codec's own loss at that scale.  q100 is recorded only (the loss there is down at the
    rounding of the colour lift), and no bound on max |M - T| is asserted (clamping before or
    after the averaging differs where the decode overshoots).  profiles/scaled_closeness.json
    holds these figures (tools/scaled_closeness.py); the recomputed table must equal it."""
    rows = sm.closeness_table(himg_amd.synth)
    dec = [r for r in rows if "psnr_M_T" in r]
    assert len(rows) == 96 and len(dec) >= 60
    for r in dec:
        print(r)
    asserted = [r for r in dec if r["q"] <= 90]
    assert len(asserted) >= 48
    for r in asserted:
        assert r["psnr_M_T"] > r["psnr_T_O"], r
    with open(os.path.join(ROOT, "profiles", "scaled_closeness.json")) as fh:
        rec = json.load(fh)
    assert rec["dropped_from_assertion"] == []
    assert rec["cases"] == json.loads(json.dumps(rows))
