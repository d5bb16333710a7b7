"""GPU (-m gpu): the window encode (encode_windows_device, Engine.encode_window, chimg -r) against the
CPU oracle's stream of the numpy crop.  Bar: status 0, exact sizes, bit-exact streams, nothing written
behind the last out_stride; the bytes outside the windows decide nothing; every refusal leaves the
output buffers as they were."""

import numpy as np
import pytest

import himg_amd
from himg_amd import build as hb

import oracle_lib as ol
import test_gpu_budget as tb   # its ten geometries, pictures and (cached) oracle streams

pytestmark = pytest.mark.gpu

CASES, IDS, THREE = tb.CASES, tb.IDS, tb.THREE
BY_NAME = {c[0]: c for c in CASES}


def _src_for(w, h, ps):
    """The issue's source for a w x h window: (w + 24) x (h + 16), padded rows, frame_pitch the exact
    extent of a picture rounded up to 16."""
    sw, sh = w + 24, h + 16
    row_pitch = sw * ps + (12 if ps == 4 else 5)
    tight = (sh - 1) * row_pitch + sw * ps
    return himg_amd.src_desc(sw, sh, ps, row_pitch, (tight + 15) // 16 * 16)


def _place(buf, src, f, x, y, pic):
    """Picture `pic` (h, w, ps) as window f at (x, y) of the source buffer."""
    h, w, ps = pic.shape
    for i in range(h):
        at = f * src.frame_pitch + (y + i) * src.row_pitch + x * ps
        buf[at: at + w * ps] = pic[i].ravel()


def _background(n, fill, seed=7):
    if fill is None:
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return np.full(n, fill, np.uint8)


def _encode_windows(torch, eng, buf, src, ch, origins, w, h, quals, ycc):
    B = len(origins)
    cap = himg_amd.max_packed_size(w, h, ch)
    d_src = torch.from_numpy(buf).cuda()
    d_out, d_sizes, d_st = tb._buffers(torch, B, cap)
    eng.encode_windows_device(d_src, src, B, ch, origins, w, h, quals, ycc, d_out, cap, d_sizes, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_sizes.cpu().numpy(), d_out.cpu().numpy(), cap


def _check_streams(tag, st, sizes, out, cap, wants):
    assert not st.any(), (tag, st)
    for f, want in enumerate(wants):
        assert int(sizes[f]) == want.size, (tag, f, int(sizes[f]), want.size)
        assert np.array_equal(out[f * cap: f * cap + want.size], want), (tag, f)
    assert not out[len(wants) * cap:].any(), (tag, "bytes behind the last frame's out_stride")


@pytest.mark.parametrize("name,w,h,ch,opts,ycc", CASES, ids=IDS)
def test_windows_match_the_oracle(name, w, h, ch, opts, ycc):
    import torch
    eng = tb._engine(opts)
    src = _src_for(w, h, ch)
    corners = [(0, 0), (5, 3), (src.width - w, src.height - h)]
    for origins, quals in ((corners, (10, 50, 90)), ([corners[2], corners[0], corners[1]], (100, 0, 37))):
        buf = _background(himg_amd.windows_extent(src, ch, origins, w, h), None)
        for f, ((k, s), (x, y)) in enumerate(zip(THREE, origins)):
            _place(buf, src, f, x, y, tb._picture(k, s, w, h, ch))
        st, sizes, out, cap = _encode_windows(torch, eng, buf, src, ch, origins, w, h, quals, ycc)
        wants = [tb._oracle(k, s, w, h, ch, q, ycc) for (k, s), q in zip(THREE, quals)]
        _check_streams((name, quals), st, sizes, out, cap, wants)
    eng.close()


@pytest.mark.parametrize("W,H,tw,th,opts", [(128, 128, 64, 64, {}), (1024, 128, 512, 64, {"front": 1, "row_tokens": 1})],
                         ids=["pix-tiles", "front-tiles"])
def test_tiles_of_one_picture(W, H, tw, th, opts):
    """frame_pitch = 0: four windows on the tile grid of ONE picture, each the oracle's stream of its tile."""
    import torch
    eng = tb._engine(opts)
    img = himg_amd.synth("randtile", 5, W, H)
    src = himg_amd.src_desc(W, H, 4, W * 4 + 16, 0)
    origins = [(x, y) for y in range(0, H, th) for x in range(0, W, tw)]
    assert len(origins) == 4
    buf = _background(himg_amd.windows_extent(src, 4, origins, tw, th), None)
    _place(buf, src, 0, 0, 0, img)
    quals = (50, 20, 80, 50)
    st, sizes, out, cap = _encode_windows(torch, eng, buf, src, 4, origins, tw, th, quals, True)
    wants = [ol.oracle_encode(img[y: y + th, x: x + tw], q, True) for (x, y), q in zip(origins, quals)]
    _check_streams((W, H), st, sizes, out, cap, wants)
    eng.close()


@pytest.mark.parametrize("name", ["pix-one-wavefront", "front-tokens", "three-channels", "not-multiples-of-8"])
def test_only_the_windows_bytes_are_used(name):
    """The source twice, identical inside the windows, 0x00 and 0xff everywhere else (row padding and the
    gap between the pictures included), in a device buffer of exactly windows_extent bytes that the last
    window ends: the same streams, the oracle's."""
    import torch
    _, w, h, ch, opts, ycc = BY_NAME[name]
    eng = tb._engine(opts)
    src = _src_for(w, h, ch)
    origins = [(5, 3), (0, 0), (src.width - w, src.height - h)]
    quals = (10, 50, 90)
    n = himg_amd.windows_extent(src, ch, origins, w, h)
    assert n == 2 * src.frame_pitch + (src.height - 1) * src.row_pitch + src.width * ch
    results = []
    for fill in (0x00, 0xff):
        buf = _background(n, fill)
        for f, ((k, s), (x, y)) in enumerate(zip(THREE, origins)):
            _place(buf, src, f, x, y, tb._picture(k, s, w, h, ch))
        results.append(_encode_windows(torch, eng, buf, src, ch, origins, w, h, quals, ycc))
    wants = [tb._oracle(k, s, w, h, ch, q, ycc) for (k, s), q in zip(THREE, quals)]
    for st, sizes, out, cap in results:
        _check_streams(name, st, sizes, out, cap, wants)
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][2], results[1][2])
    eng.close()


@pytest.mark.parametrize("name", ["pix-one-wavefront", "front-tokens"])
def test_tight_windows_equal_encode_device_q(name):
    """row_pitch = w * ps, tight frame_pitch, origins 0: the bytes of encode_device_q on the same buffer."""
    import torch
    _, w, h, ch, opts, ycc = BY_NAME[name]
    eng = tb._engine(opts)
    frames = np.stack([tb._picture(k, s, w, h, ch) for k, s in THREE])
    d_frames = torch.from_numpy(frames).cuda()
    cap = himg_amd.max_packed_size(w, h, ch)
    quals = (10, 50, 90)
    a_out, a_sizes, a_st = tb._buffers(torch, 3, cap)
    eng.encode_device_q(d_frames, 3, w, h, ch, ch, quals, ycc, a_out, cap, a_sizes, a_st)
    b_out, b_sizes, b_st = tb._buffers(torch, 3, cap)
    eng.encode_windows_device(d_frames, himg_amd.src_desc(w, h, ch), 3, ch, [(0, 0)] * 3, w, h, quals, ycc, b_out, cap,
                              b_sizes, b_st)
    torch.cuda.synchronize()
    assert not a_st.cpu().numpy().any() and not b_st.cpu().numpy().any()
    assert np.array_equal(a_sizes.cpu().numpy(), b_sizes.cpu().numpy()) and a_sizes.cpu().numpy().all()
    assert np.array_equal(a_out.cpu().numpy(), b_out.cpu().numpy())
    eng.close()


def test_refusals_write_nothing():
    import torch
    w, h, ch = 64, 64, 4
    eng = himg_amd.Engine(0)
    ok = _src_for(w, h, ch)
    sw, sh = ok.width, ok.height
    good = [(0, 0), (5, 3), (sw - w, sh - h)]
    d_src = torch.zeros(3 * ok.frame_pitch + 64, dtype=torch.uint8, device="cuda")
    cap = himg_amd.max_packed_size(w, h, ch)
    d_out, d_sizes, d_st = tb._buffers(torch, 3, cap, fill=0xa5)

    def refused(src=ok, origins=good, quals=(10, 50, 90), ptr=None, ww=w, hh=h):
        with pytest.raises(himg_amd.HimgError) as ei:
            eng.encode_windows_device(d_src if ptr is None else ptr, src, 3, ch, origins, ww, hh, quals, True, d_out, cap,
                                      d_sizes, d_st)
        assert ei.value.code == himg_amd.HIMG_ERR_ARG, ei.value

    for bad in [(-1, 0), (0, -1), (sw - w + 1, 3), (5, sh - h + 1)]:       # one pixel outside, each direction
        for slot in range(3):
            refused(origins=good[:slot] + [bad] + good[slot + 1:])
    refused(src=himg_amd.src_desc(sw, sh, ch, sw * ch - 4, ok.frame_pitch))             # row_pitch too small
    refused(src=himg_amd.src_desc(sw, sh, ch, ok.row_pitch + 2, ok.frame_pitch + 1024))  # ps = 4: whole dwords
    refused(src=himg_amd.src_desc(sw, sh, ch, ok.row_pitch, ok.frame_pitch + 2))
    refused(src=himg_amd.src_desc(sw, sh, ch, ok.row_pitch, (sh - 1) * ok.row_pitch + sw * ch - 4))   # bad frame_pitch
    refused(src=himg_amd.src_desc(sw, sh, ch, ok.row_pitch, 16))
    refused(quals=(10, 101, 90))
    refused(quals=(10, 50, -1))
    refused(src=himg_amd.src_desc(sw, sh, 3, ok.row_pitch, ok.frame_pitch))              # pixel_stride < channels
    refused(ptr=d_src.data_ptr() + 4)                                                   # d_src not 16-byte aligned
    refused(ww=0)
    refused(hh=-1)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xa5).all()
    assert (d_sizes.cpu().numpy() == 0x5a5a5a5a).all() and (d_st.cpu().numpy() == 0x5a5a5a5a).all()
    eng.close()


def test_ordinary_encode_around_a_window_call():
    """encode_device on the same context before and after a window call of another geometry."""
    import torch
    eng = himg_amd.Engine(0)
    (k, s), W, H = THREE[0], 200, 72
    img = tb._picture(k, s, W, H, 4)
    want = tb._oracle(k, s, W, H, 4, 50, True)
    d_img = torch.from_numpy(img).cuda()
    cap = himg_amd.max_packed_size(W, H, 4)

    def plain():
        d_out, d_sizes, d_st = tb._buffers(torch, 1, cap)
        eng.encode_device(d_img, 1, W, H, 4, 4, 50, True, d_out, cap, d_sizes, d_st)
        torch.cuda.synchronize()
        _check_streams("plain", d_st.cpu().numpy(), d_sizes.cpu().numpy(), d_out.cpu().numpy(), cap, [want])

    plain()
    w, h = 100, 52
    src = himg_amd.src_desc(W, H, 4, frame_pitch=0)
    st, sizes, out, wcap = _encode_windows(torch, eng, img.ravel(), src, 4, [(5, 3), (100, 20)], w, h, (50, 37), True)
    wants = [ol.oracle_encode(img[3: 3 + h, 5: 5 + w], 50, True), ol.oracle_encode(img[20: 20 + h, 100: 100 + w], 37, True)]
    _check_streams("windows", st, sizes, out, wcap, wants)
    plain()
    eng.close()


def test_host_window_and_capacity_protocol():
    import ctypes as C
    eng = himg_amd.Engine(0)
    W, H, w, h, x, y = 131, 77, 100, 52, 5, 3
    img = himg_amd.synth("randtile", 9, W, H)
    src = himg_amd.src_desc(W, H, 4, W * 4 + 12, 0)
    buf = _background((H - 1) * src.row_pitch + W * 4, None)
    _place(buf, src, 0, 0, 0, img)
    for (xx, yy), q in (((x, y), 50), ((W - w, H - h), 90), ((0, 0), 0)):
        want = ol.oracle_encode(img[yy: yy + h, xx: xx + w], q, True)
        assert np.array_equal(eng.encode_window(buf, src, xx, yy, w, h, q), want), (xx, yy, q)
    # frame_pitch is ignored: there is one picture
    junk = himg_amd.src_desc(W, H, 4, src.row_pitch, 2)
    assert np.array_equal(eng.encode_window(buf, junk, x, y, w, h, 50), ol.oracle_encode(img[y: y + h, x: x + w], 50, True))
    # three channels of four-byte pixels, RGB
    want = ol.oracle_encode(img[y: y + h, x: x + w], 50, False, channels=3, stride=4)
    assert np.array_equal(eng.encode_window(buf, src, x, y, w, h, 50, use_ycbcr=False, channels=3), want)
    # the capacity protocol: too small a buffer reports the size, himg_hip_fetch_last delivers the stream
    want = ol.oracle_encode(img[y: y + h, x: x + w], 50, True)
    L, n = himg_amd.lib(), C.c_size_t()
    small = np.full(want.size - 1, 0xa5, np.uint8)
    rc = L.himg_hip_encode_window_to(eng._ctx, buf.ctypes.data, C.byref(src), 4, x, y, w, h, 50, 1, small.ctypes.data,
                                     small.nbytes, C.byref(n))
    assert (rc, n.value) == (himg_amd.HIMG_ERR_CAPACITY, want.size) and (small == 0xa5).all()
    got = np.empty(want.size, np.uint8)
    assert L.himg_hip_fetch_last(eng._ctx, got.ctypes.data, got.nbytes, C.byref(n)) == 0 and np.array_equal(got, want)
    exact = np.empty(want.size, np.uint8)
    rc = L.himg_hip_encode_window_to(eng._ctx, buf.ctypes.data, C.byref(src), 4, x, y, w, h, 50, 1, exact.ctypes.data,
                                     exact.nbytes, C.byref(n))
    assert (rc, n.value) == (0, want.size) and np.array_equal(exact, want)
    # a window outside: HIMG_ERR_ARG, no size
    rc = L.himg_hip_encode_window_to(eng._ctx, buf.ctypes.data, C.byref(src), 4, W - w + 1, y, w, h, 50, 1, exact.ctypes.data,
                                     exact.nbytes, C.byref(n))
    assert (rc, n.value) == (himg_amd.HIMG_ERR_ARG, 0)
    eng.close()


def test_chimg_rectangle(tmp_path):
    """chimg -r x,y,w,h writes the file chimg writes for the cropped picture.  The rectangle is in the codec's
    coordinates (row 0 = the first coded row = the picture's bottom scanline), as dhimg -r's."""
    import test_cli as tc
    chimg = hb.build_cli()[0]
    W, H, w, h, x, y = 131, 77, 100, 52, 5, 3
    img = himg_amd.synth("randtile", 9, W, H)
    full, crop = str(tmp_path / "full.pam"), str(tmp_path / "crop.pam")
    tc._write_pnm(full, img)
    tc._write_pnm(crop, img[H - y - h: H - y, x: x + w])
    a, b = str(tmp_path / "a.himg"), str(tmp_path / "b.himg")
    for q in ("50", "90"):
        r = tc._run(chimg, "-q", q, "-r", "%d,%d,%d,%d" % (x, y, w, h), full, a)
        assert r.returncode == 0, r.stderr
        assert tc._run(chimg, "-q", q, crop, b).returncode == 0
        got = open(a, "rb").read()
        assert got == open(b, "rb").read() and r.stdout == "Compressed size: %d\n" % len(got)
    r = tc._run(chimg, "-r", "5,3,100", full, a)
    assert r.returncode == 0 and r.stdout.startswith("Invalid rectangle: 5,3,100\nUsage:")
    r = tc._run(chimg, "-r", "32,3,100,52", full, a)
    assert r.returncode == 255 and "does not lie inside" in r.stderr
