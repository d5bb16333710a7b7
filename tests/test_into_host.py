"""Host (no GPU): the destination descriptor and window rules of the decodes into pitched pictures
through himg_hip_dst_extent -- a hand-computed case, every refusal of include/himg_hip.h with its code
-- the new entries exported, declared with the documented signatures and wrapped, and the defaults of
himg_amd.dst_desc."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import himg_amd

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "himg_hip.h")
ARG = himg_amd.HIMG_ERR_ARG


def _extent_rc(dst, channels, origins, w, h):
    org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
    n = C.c_size_t(12345)
    rc = himg_amd.lib().himg_hip_dst_extent(C.byref(dst) if dst is not None else None, channels, len(org),
                                            org.ctypes.data, w, h, C.byref(n))
    return rc, n.value


def test_symbols_exported_declared_and_wrapped():
    L = himg_amd.lib()
    head = re.sub(r"\s+", " ", open(HEADER).read())
    # (the documented signatures: parameter types in order)
    want = {
        "himg_hip_dst_extent": "const himg_hip_dst *dst, int num_channels, int batch, const int32_t *h_origins, "
                               "int w, int h, size_t *bytes",
        "himg_hip_decode_into_device": "himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, "
                                       "const uint32_t *h_sizes, int batch, int width, int height, int num_channels, "
                                       "void *d_dst, const himg_hip_dst *dst, const int32_t *h_origins, "
                                       "int32_t *d_status, void *stream",
        "himg_hip_decode_regions_into_device": "himg_hip_ctx *ctx, const void *d_packed, size_t in_stride, "
                                               "const uint32_t *h_sizes, int batch, int width, int height, "
                                               "int num_channels, const int32_t *h_src_origins, int w, int h, "
                                               "void *d_dst, const himg_hip_dst *dst, const int32_t *h_dst_origins, "
                                               "int32_t *d_status, void *stream",
        "himg_hip_decode_into_to": "himg_hip_ctx *ctx, const uint8_t *packed, size_t packed_size, uint8_t *dst_data, "
                                   "const himg_hip_dst *dst, int x, int y, int *width, int *height, int *channels",
    }
    for name, params in want.items():
        assert hasattr(L, name), name
        assert "int %s(%s);" % (name, params) in head, name
        assert len(getattr(L, name).argtypes) == params.count(",") + 1, name
    assert C.sizeof(himg_amd.DstDesc) == 32
    assert [f for f, _ in himg_amd.DstDesc._fields_] == ["width", "height", "pixel_stride", "row_pitch", "frame_pitch"]
    for meth in ("decode_into_device", "decode_regions_into_device", "decode_into"):
        assert callable(getattr(himg_amd.Engine, meth)), meth


def test_dst_desc_defaults():
    t = himg_amd.dst_desc(64, 32, 3)
    assert (t.width, t.height, t.pixel_stride, t.row_pitch, t.frame_pitch) == (64, 32, 3, 192, 192 * 32)
    u = himg_amd.dst_desc(64, 32, 4, 300)
    assert (u.row_pitch, u.frame_pitch) == (300, 300 * 32)
    v = himg_amd.dst_desc(64, 32, 4, 300, 0)
    assert (v.row_pitch, v.frame_pitch) == (300, 0)


def test_extent_by_hand():
    # three pictures 131 x 77 of 4-byte pixels, rows 536 bytes apart, pictures 41280 bytes apart; windows
    # 100 x 52.  Frame 2 at (5, 3): 2 * 41280 + (3 + 51) * 536 + (5 + 100) * 4 = 82560 + 28944 + 420.
    d = himg_amd.dst_desc(131, 77, 4, 536, 41280)
    assert himg_amd.dst_extent(d, 4, [(31, 25), (0, 0), (5, 3)], 100, 52) == 111924
    # frame 0 alone in the bottom right corner: 76 * 536 + 131 * 4
    assert himg_amd.dst_extent(d, 4, [(31, 25)], 100, 52) == 41260
    # one picture (frame_pitch 0): the largest window end, whichever frame has it
    one = himg_amd.dst_desc(131, 77, 4, 536, 0)
    assert himg_amd.dst_extent(one, 4, [(0, 0), (31, 25), (5, 3)], 100, 52) == 41260
    # three channels into 4-byte pixels at an odd origin: whole pixels count -- (3 + 7) * 160 + (5 + 16) * 4
    rgba = himg_amd.dst_desc(40, 24, 4, 160, 0)
    assert himg_amd.dst_extent(rgba, 3, [(5, 3)], 16, 8) == 1684


def test_refusals():
    ok = dict(width=131, height=77, pixel_stride=4, row_pitch=131 * 4 + 12, frame_pitch=0)

    def rc(channels=4, origins=((5, 3),), w=100, h=52, dst=True, **over):
        d = himg_amd.dst_desc(**{**ok, **over}) if dst else None
        return _extent_rc(d, channels, origins, w, h)

    assert rc() == (0, 54 * (131 * 4 + 12) + 105 * 4)
    assert rc(dst=False)[0] == ARG                                        # dst NULL
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(height=-1)):
        assert rc(**bad)[0] == ARG, bad                                   # picture size not positive
    for w, h in [(0, 52), (100, 0), (-1, 52), (100, -7)]:
        assert rc(w=w, h=h)[0] == ARG, (w, h)                             # window size not positive
    assert rc(channels=4, pixel_stride=3, row_pitch=131 * 3)[0] == ARG    # pixel_stride < num_channels
    assert rc(channels=3, pixel_stride=3, row_pitch=131 * 3)[0] == 0
    for channels in (0, 5):
        assert rc(channels=channels)[0] == ARG, channels
    assert rc(row_pitch=131 * 4 - 4)[0] == ARG                            # row_pitch < width * pixel_stride
    assert rc(row_pitch=131 * 4)[0] == 0
    tight = 76 * (131 * 4 + 12) + 131 * 4
    assert rc(frame_pitch=tight - 4)[0] == ARG                            # frame_pitch neither 0 nor a picture
    assert rc(frame_pitch=4)[0] == ARG
    assert rc(frame_pitch=tight) == (0, 54 * (131 * 4 + 12) + 105 * 4)
    for org in [(-1, 3), (5, -1), (32, 3), (5, 26)]:                      # one pixel outside, every direction
        assert rc(origins=(org,))[0] == ARG, org
        assert rc(origins=((0, 0), org), frame_pitch=tight)[0] == ARG, org
    for org in [(0, 0), (31, 25), (31, 0), (0, 25), (5, 3), (7, 1)]:      # odd origins are legal
        assert rc(origins=(org,))[0] == 0, org
    assert rc(row_pitch=131 * 4 + 6)[0] == ARG                            # pixel_stride 4: pitches in whole dwords
    assert rc(frame_pitch=tight + 2)[0] == ARG
    assert rc(channels=3, row_pitch=131 * 4 + 6)[0] == ARG                # ... whatever the channel count
    assert rc(channels=3, pixel_stride=3, row_pitch=131 * 3 + 5, frame_pitch=76 * (131 * 3 + 5) + 131 * 3 + 1)[0] == 0
    assert rc(origins=((32, 3),)) == (ARG, 0)                             # a refusal leaves *bytes at 0
    with pytest.raises(himg_amd.HimgError) as e:
        himg_amd.dst_extent(himg_amd.dst_desc(8, 8, 4), 4, [(1, 0)], 8, 8)
    assert e.value.code == ARG
    n = C.c_size_t()
    org = np.zeros(2, np.int32)
    d = himg_amd.dst_desc(8, 8, 4)
    L = himg_amd.lib()
    assert L.himg_hip_dst_extent(C.byref(d), 4, 0, org.ctypes.data, 8, 8, C.byref(n)) == ARG   # batch
    assert L.himg_hip_dst_extent(C.byref(d), 4, 1, None, 8, 8, C.byref(n)) == ARG
    assert L.himg_hip_dst_extent(C.byref(d), 4, 1, org.ctypes.data, 8, 8, None) == ARG


def test_device_entries_refuse_without_a_context():
    """The NULL-argument refusals of the device and host-picture entries need no GPU."""
    L = himg_amd.lib()
    d = himg_amd.dst_desc(8, 8, 4)
    org = np.zeros(2, np.int32)
    w = C.c_int()
    assert L.himg_hip_decode_into_device(None, None, 0, None, 1, 8, 8, 4, None, C.byref(d), org.ctypes.data, None, None) == ARG
    assert L.himg_hip_decode_regions_into_device(None, None, 0, None, 1, 8, 8, 4, org.ctypes.data, 8, 8, None, C.byref(d),
                                                 org.ctypes.data, None, None) == ARG
    assert L.himg_hip_decode_into_to(None, None, 0, None, C.byref(d), 0, 0, C.byref(w), C.byref(w), C.byref(w)) == ARG
