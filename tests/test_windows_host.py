"""Host (no GPU): the source descriptor and window rules of the window encode through
himg_hip_windows_extent -- against a three-line numpy model over seeded descriptors, and every
refusal of include/himg_hip.h with its code -- and the marshalling of himg_amd.src_desc /
himg_amd.windows_extent."""
import ctypes as C

import numpy as np
import pytest

import himg_amd


def _extent_rc(src, channels, origins, w, h):
    org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(-1, 2))
    n = C.c_size_t(12345)
    rc = himg_amd.lib().himg_hip_windows_extent(C.byref(src) if src is not None else None, channels, len(org),
                                                org.ctypes.data, w, h, C.byref(n))
    return rc, n.value


def model_extent(src, origins, w, h):
    """The largest f * frame_pitch + (y_f + h - 1) * row_pitch + (x_f + w) * pixel_stride."""
    org = np.asarray(origins, np.int64).reshape(-1, 2)
    f = np.arange(len(org), dtype=np.int64)
    return int((f * src.frame_pitch + (org[:, 1] + h - 1) * src.row_pitch + (org[:, 0] + w) * src.pixel_stride).max())


def test_symbols_exported():
    L = himg_amd.lib()
    for name in ("himg_hip_windows_extent", "himg_hip_encode_windows_device", "himg_hip_encode_window_to"):
        assert hasattr(L, name), name
    assert C.sizeof(himg_amd.SrcDesc) == 32
    assert [f for f, _ in himg_amd.SrcDesc._fields_] == ["width", "height", "pixel_stride", "row_pitch", "frame_pitch"]


def _random_case(rng):
    channels = int(rng.integers(1, 5))
    ps = channels + int(rng.integers(0, 3)) if rng.random() < 0.5 else channels
    sw, sh = int(rng.integers(1, 300)), int(rng.integers(1, 200))
    w, h = int(rng.integers(1, sw + 1)), int(rng.integers(1, sh + 1))
    unit = 4 if ps == 4 else 1
    row_pitch = sw * ps + unit * int(rng.integers(0, 9))
    if ps == 4:
        row_pitch = (row_pitch + 3) // 4 * 4
    tight = (sh - 1) * row_pitch + sw * ps
    kind = int(rng.integers(0, 3))
    frame_pitch = 0 if kind == 0 else (tight + unit - 1) // unit * unit + (0 if kind == 1 else unit * int(rng.integers(0, 40)))
    batch = int(rng.integers(1, 9))
    org = np.stack([rng.integers(0, sw - w + 1, batch), rng.integers(0, sh - h + 1, batch)], axis=1)
    # windows at the last column and the last row
    org[rng.integers(0, batch)] = (sw - w, sh - h)
    return himg_amd.src_desc(sw, sh, ps, row_pitch, frame_pitch), channels, org, w, h


def test_extent_matches_model():
    rng = np.random.default_rng(20261019)
    seen = set()
    for _ in range(400):
        src, channels, org, w, h = _random_case(rng)
        want = model_extent(src, org, w, h)
        assert _extent_rc(src, channels, org, w, h) == (0, want), (src.width, src.height, src.pixel_stride, org, w, h)
        assert himg_amd.windows_extent(src, channels, org, w, h) == want
        seen.add((src.frame_pitch == 0, src.pixel_stride > channels))
    assert len(seen) == 4   # one picture / a picture per frame, packed pixels / pixel_stride > channels


def test_extent_corners():
    # one picture: the window in the bottom right corner ends at the picture's last byte
    s = himg_amd.src_desc(131, 77, 4, 131 * 4 + 12, 0)
    assert himg_amd.windows_extent(s, 4, [(0, 0), (31, 25)], 100, 52) == 76 * s.row_pitch + 131 * 4
    # the default pitches are the packed ones
    t = himg_amd.src_desc(64, 32, 3)
    assert (t.row_pitch, t.frame_pitch) == (192, 192 * 32)
    assert himg_amd.windows_extent(t, 3, [(0, 0), (0, 0), (63, 31)], 1, 1) == 2 * t.frame_pitch + 31 * 192 + 64 * 3
    # an odd origin is legal, pixel_stride > channels counts whole pixels
    u = himg_amd.src_desc(40, 24, 4, 160, 0)
    assert himg_amd.windows_extent(u, 3, [(5, 3)], 16, 8) == 10 * 160 + 21 * 4


def test_refusals():
    ARG = himg_amd.HIMG_ERR_ARG
    ok = dict(width=131, height=77, pixel_stride=4, row_pitch=131 * 4 + 12, frame_pitch=0)

    def rc(channels=4, origins=((5, 3),), w=100, h=52, src=True, **over):
        s = himg_amd.src_desc(**{**ok, **over}) if src else None
        return _extent_rc(s, channels, origins, w, h)

    assert rc() == (0, 54 * (131 * 4 + 12) + 105 * 4)
    assert rc(src=False)[0] == ARG                                        # NULL src
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(height=-1)):
        assert rc(**bad)[0] == ARG, bad                                   # source size not positive
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
    for org in [(0, 0), (31, 25), (31, 0), (0, 25)]:
        assert rc(origins=(org,))[0] == 0, org
    assert rc(row_pitch=131 * 4 + 6)[0] == ARG                            # pixel_stride 4: pitches in whole dwords
    assert rc(frame_pitch=tight + 2)[0] == ARG
    assert rc(channels=3, pixel_stride=3, row_pitch=131 * 3 + 5, frame_pitch=76 * (131 * 3 + 5) + 131 * 3 + 1)[0] == 0
    # a refusal leaves *bytes at 0
    assert rc(origins=((32, 3),)) == (ARG, 0)
    with pytest.raises(himg_amd.HimgError) as e:
        himg_amd.windows_extent(himg_amd.src_desc(8, 8, 4), 4, [(1, 0)], 8, 8)
    assert e.value.code == ARG
    n = C.c_size_t()
    org = np.zeros(2, np.int32)
    s = himg_amd.src_desc(8, 8, 4)
    L = himg_amd.lib()
    assert L.himg_hip_windows_extent(C.byref(s), 4, 0, org.ctypes.data, 8, 8, C.byref(n)) == ARG   # batch
    assert L.himg_hip_windows_extent(C.byref(s), 4, 1, None, 8, 8, C.byref(n)) == ARG
    assert L.himg_hip_windows_extent(C.byref(s), 4, 1, org.ctypes.data, 8, 8, None) == ARG
