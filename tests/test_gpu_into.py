"""GPU: the decodes into windows of pitched destination pictures -- decode_into_device,
decode_regions_into_device and Engine.decode_into.  Expected bytes: the CPU oracle's decode of the
same stream, pasted with numpy into a copy of the destination's initial (random) contents; the WHOLE
destination buffer and a 64-byte sentinel tail are compared, so every byte that must stay -- the bytes
of a pixel past its channels, row padding, pixels outside a window, the gap between pictures, the
bytes behind the last window -- is checked.  Every store form (the fused row kernel's <512>, <-1>
and <0> forms, both k_tile_inv forms, the region kernel; 16-byte, dword and byte stores), the
profiler's stage names say which kernel ran; the tiles of one picture (frame_pitch = 0); a damaged
frame in a batch; refusals that leave the outputs alone."""
import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol
from test_gpu_region import _crop, _full, _stream
from test_gpu_regions import _upload
from test_gpu_tensor import SHAPES, _pictures

pytestmark = pytest.mark.gpu

TAIL = 64
OTHER_STORE_STAGES = {"k_dec_row_fused", "k_tile_inv<true>", "k_tile_inv<false>", "k_dec_region",
                      "k_dec_row_fused_t<512>", "k_dec_row_fused_t<-1>", "k_dec_row_fused_t<0>",
                      "k_tile_inv_t<true>", "k_tile_inv_t<false>", "k_dec_region_t"}


@pytest.fixture
def eng(engine):
    """The session's engine; HIMG_OPT_FIX_T2 back to the default behind every test."""
    yield engine
    engine.set_option("fix_t2", 0)


def _padded(Wd, Hd, ps, one_picture=False):
    """A descriptor of padded pictures: a row pitch that is no multiple of 16 (4-byte pixels: + 12 bytes,
    whole dwords; otherwise an odd padding) and a gap between the pictures."""
    rp = Wd * ps + (12 if ps == 4 else 5)
    if rp % 16 == 0:
        rp += 4 if ps == 4 else 2
    tight = (Hd - 1) * rp + Wd * ps
    fp = 0 if one_picture else ((tight + 3) // 4 * 4 + 8 if ps == 4 else tight + 3)
    return himg_amd.dst_desc(Wd, Hd, ps, rp, fp)


def _background(dst, n, seed):
    """n pictures' bytes of random background (the last picture ends with its last pixel) and the tail."""
    nbytes = (n - 1) * dst.frame_pitch + (dst.height - 1) * dst.row_pitch + dst.width * dst.pixel_stride
    return np.random.default_rng(seed).integers(0, 256, nbytes + TAIL, dtype=np.uint8)


def _paste(buf, dst, f, x, y, pic):
    """pic (h, w, C) at (x, y) of picture f: the definition of include/himg_hip.h."""
    h, w, Cn = pic.shape
    base = f * dst.frame_pitch + y * dst.row_pitch + x * dst.pixel_stride
    v = np.lib.stride_tricks.as_strided(buf[base:], shape=(h, w, Cn), strides=(dst.row_pitch, dst.pixel_stride, 1))
    v[...] = pic


def _same(d_got, want, what):
    d_want = torch.from_numpy(want).cuda()
    if not torch.equal(d_got, d_want):
        bad = (d_got != d_want).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError("%s: %d of %d bytes differ, first at %d: got %#x, expected %#x"
                             % (what, bad.numel(), want.size, i, int(d_got[i]), int(d_want[i])))


def _status(n):
    return torch.full((n,), -99, dtype=torch.int32, device="cuda")


def _profiled(eng, call):
    eng.profile(True)
    eng.profile_reset()
    call()
    torch.cuda.synchronize()
    stages = eng.profile_read()
    eng.profile(False)
    return set(stages)


# ---- 1. every store form, padded pictures -------------------------------------------------------

@pytest.mark.parametrize("W,H,Cn,quals,batch,stage,also_rgb", SHAPES)
def test_every_store_form_padded(eng, W, H, Cn, quals, batch, stage, also_rgb):
    stage = stage.replace("_t<", "_p<")
    nsrc = min(batch, 3)
    Wd, Hd = W + 24, H + 16
    for ycbcr in ([True, False] if also_rgb else [True]):
        streams = [_stream("randtile", W, H, Cn, quals[0], ycbcr, seed=s) for s in range(nsrc)]
        pics = _pictures(eng, streams, H, W, Cn)
        pick = [f % nsrc for f in range(batch)]
        d_in, stride = _upload([streams[k] for k in pick])
        sizes = [len(streams[k]) for k in pick]
        # aligned, dword-aligned, neither, and the bottom right corner (the last frame's: the buffer ends
        # with its last pixel)
        cycle = [(0, 0), (5, 3), (4, 8), (Wd - W, Hd - H)]
        org = [cycle[f % 4] for f in range(batch)]
        org[-1] = cycle[3]
        for ps in sorted({Cn, 4}):
            dst = _padded(Wd, Hd, ps)
            assert dst.row_pitch % 16 != 0
            bg = _background(dst, batch, seed=W + ps)
            assert himg_amd.dst_extent(dst, Cn, org, W, H) == bg.size - TAIL
            want = bg.copy()
            for f in range(batch):
                _paste(want, dst, f, org[f][0], org[f][1], pics[pick[f]])
            d_dst = torch.from_numpy(bg).cuda()
            d_st = _status(batch)
            stages = _profiled(eng, lambda: eng.decode_into_device(d_in, stride, sizes, batch, W, H, Cn, d_dst, dst,
                                                                   org, d_st))
            what = "%dx%dx%d ycbcr=%d pixel_stride=%d" % (W, H, Cn, ycbcr, ps)
            assert (d_st.cpu().numpy() == 0).all(), what
            assert stage in stages and not (OTHER_STORE_STAGES & stages), (what, stage, sorted(stages))
            _same(d_dst, want, what)


# ---- 2. the tiles of one picture (frame_pitch = 0) -----------------------------------------------

def _tiles_case(eng, picture, tiles, quals, row_pad):
    """tiles: (x, y, w, h) of each tile stream; tiles of one size go through one call."""
    PH, PW, Cn = picture.shape
    ps = Cn
    dst = himg_amd.dst_desc(PW, PH, ps, PW * ps + row_pad, 0)
    bg = _background(dst, 1, seed=PW)
    want = bg.copy()
    d_dst = torch.from_numpy(bg).cuda()
    for size in sorted({t[2:] for t in tiles}):
        group = [(t, q) for t, q in zip(tiles, quals) if t[2:] == size]
        w, h = size
        streams = [np.frombuffer(ol.oracle_encode(np.ascontiguousarray(_crop(picture, t)), q, True), np.uint8).copy()
                   for t, q in group]
        pics = _pictures(eng, streams, h, w, Cn)
        for (t, _), p in zip(group, pics):
            _paste(want, dst, 0, t[0], t[1], p)
        d_in, stride = _upload(streams)
        d_st = _status(len(streams))
        eng.decode_into_device(d_in, stride, [len(s) for s in streams], len(streams), w, h, Cn, d_dst, dst,
                               [t[:2] for t, _ in group], d_st)
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == 0).all(), size
    _same(d_dst, want, "tiles of %dx%dx%d" % (PW, PH, Cn))


def test_tiles_of_one_picture_rgba(eng):
    pic = himg_amd.synth("randtile", 7, 128, 128)
    _tiles_case(eng, pic, [(0, 0, 64, 64), (64, 0, 64, 64), (0, 64, 64, 64), (64, 64, 64, 64)], (50, 20, 80, 50), 16)


def test_tiles_of_one_picture_wide(eng):
    pic = himg_amd.synth("randtile", 8, 1024, 128)
    _tiles_case(eng, pic, [(0, 0, 512, 64), (512, 0, 512, 64), (0, 64, 512, 64), (512, 64, 512, 64)], (50, 20, 80, 50), 16)


def test_tiles_of_one_picture_ragged_rgb(eng):
    pic = np.ascontiguousarray(himg_amd.synth("randtile", 9, 100, 37)[:, :, :3])
    _tiles_case(eng, pic, [(0, 0, 50, 19), (50, 0, 50, 19), (0, 19, 50, 18), (50, 19, 50, 18)], (50, 20, 80, 50), 7)


# ---- 3. a tight destination is the existing decode ----------------------------------------------

@pytest.mark.parametrize("W,H,Cn,batch", [(4096, 24, 4, 2), (203, 21, 4, 3)])
def test_tight_destination_is_decode_device(eng, W, H, Cn, batch):
    streams = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(batch)]
    _pictures(eng, streams, H, W, Cn)   # (the decode mode these streams need)
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    n = batch * H * W * Cn
    d_ref = torch.full((n + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = _status(batch)
    eng.decode_device(d_in, stride, sizes, batch, W, H, Cn, d_ref, d_st)
    d_dst = torch.full((n + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st2 = _status(batch)
    eng.decode_into_device(d_in, stride, sizes, batch, W, H, Cn, d_dst, himg_amd.dst_desc(W, H, Cn),
                           [(0, 0)] * batch, d_st2)
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == 0).all() and (d_st2.cpu().numpy() == 0).all()
    assert torch.equal(d_dst, d_ref)


REGION_ORIGINS = {(264, 40): [(3, 5), (224, 23), (8, 8)], (100, 37): [(3, 5), (60, 20), (8, 8)]}   # inside, the corner, aligned
WIN = (40, 17)


def test_tight_destination_is_decode_regions_device(eng):
    W, H, Cn = 264, 40, 4
    w, h = WIN
    org = REGION_ORIGINS[(W, H)]
    streams = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(3)]
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    n = 3 * h * w * Cn
    d_ref = torch.full((n + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = _status(3)
    eng.decode_regions_device(d_in, stride, sizes, 3, W, H, Cn, org, w, h, d_ref, d_st)
    d_dst = torch.full((n + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st2 = _status(3)
    stages = _profiled(eng, lambda: eng.decode_regions_into_device(d_in, stride, sizes, 3, W, H, Cn, org, w, h, d_dst,
                                                                   himg_amd.dst_desc(w, h, Cn), [(0, 0)] * 3, d_st2))
    assert (d_st.cpu().numpy() == 0).all() and (d_st2.cpu().numpy() == 0).all()
    assert "k_dec_region_p" in stages and not (OTHER_STORE_STAGES & stages), sorted(stages)
    assert torch.equal(d_dst, d_ref)


# ---- 4. regions into windows ---------------------------------------------------------------------

@pytest.mark.parametrize("W,H,Cn,ps", [(264, 40, 4, 4), (100, 37, 3, 3), (100, 37, 3, 4)])
def test_regions_into_windows(eng, W, H, Cn, ps):
    w, h = WIN
    src_org = REGION_ORIGINS[(W, H)]
    dst_org = [(1, 1), (96 - w - 1, 64 - h), (7, 3)]   # odd origins; the second window ends in the last row
    streams = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(3)]
    pics = _pictures(eng, streams, H, W, Cn)
    dst = _padded(96, 64, ps)
    bg = _background(dst, 3, seed=W + ps)
    want = bg.copy()
    for f in range(3):
        _paste(want, dst, f, dst_org[f][0], dst_org[f][1], _crop(pics[f], src_org[f] + WIN))
    d_in, stride = _upload(streams)
    d_dst = torch.from_numpy(bg).cuda()
    d_st = _status(3)
    stages = _profiled(eng, lambda: eng.decode_regions_into_device(d_in, stride, [len(s) for s in streams], 3, W, H, Cn,
                                                                   src_org, w, h, d_dst, dst, dst_org, d_st))
    assert (d_st.cpu().numpy() == 0).all()
    assert "k_dec_region_p" in stages and not (OTHER_STORE_STAGES & stages), sorted(stages)
    _same(d_dst, want, "%dx%dx%d pixel_stride=%d" % (W, H, Cn, ps))


# ---- 5. a damaged frame in a batch ---------------------------------------------------------------

def test_damaged_frame_in_a_batch(eng):
    W, H, Cn = 264, 40, 4
    good = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(3)]
    pics = _pictures(eng, good, H, W, Cn)
    offs, lens = himg_amd.index_host(good[1])[3:5]
    cut = good[1][:int(offs[1]) + int(lens[1]) // 2].copy()   # truncated inside its second block row
    streams = [good[0], cut, good[2]]
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    d_pix = torch.empty((3, H, W, Cn), dtype=torch.uint8, device="cuda")
    d_st = _status(3)
    eng.decode_device(d_in, stride, sizes, 3, W, H, Cn, d_pix, d_st)
    torch.cuda.synchronize()
    st_ref = d_st.cpu().numpy()
    assert st_ref[0] == 0 and st_ref[1] != 0 and st_ref[2] == 0, st_ref
    dst = _padded(W + 24, H + 16, 4)
    org = [(5, 3), (4, 8), (24, 16)]
    bg = _background(dst, 3, seed=5)
    d_dst = torch.from_numpy(bg).cuda()
    d_st2 = _status(3)
    eng.decode_into_device(d_in, stride, sizes, 3, W, H, Cn, d_dst, dst, org, d_st2)
    torch.cuda.synchronize()
    assert np.array_equal(d_st2.cpu().numpy(), st_ref)
    want = bg.copy()
    _paste(want, dst, 0, org[0][0], org[0][1], pics[0])
    _paste(want, dst, 2, org[2][0], org[2][1], pics[2])
    got = d_dst.cpu().numpy()
    # frame 1's window holds unspecified bytes: it is taken from the result; everything else is checked
    _paste(want, dst, 1, org[1][0], org[1][1], np.lib.stride_tricks.as_strided(
        got[dst.frame_pitch + org[1][1] * dst.row_pitch + org[1][0] * 4:], shape=(H, W, Cn),
        strides=(dst.row_pitch, 4, 1)).copy())
    assert np.array_equal(got, want)


# ---- 6. refusals leave everything as it was ------------------------------------------------------

def test_refusals_leave_everything_alone(eng):
    W, H, Cn = 96, 48, 4
    b = _stream("randtile", W, H, Cn, 50, True)
    d_in, stride = _upload([b, b])
    sizes = [len(b)] * 2
    good = _padded(W + 24, H + 16, 4)
    bg = _background(good, 2, seed=6)
    d_dst = torch.from_numpy(bg).cuda()
    d_st = _status(2)
    org = [(5, 3), (24, 16)]
    three = himg_amd.dst_desc(W + 24, H + 16, 3)
    odd = himg_amd.dst_desc(W + 24, H + 16, 4, (W + 24) * 4 + 6)
    cases = [("a window one pixel outside", good, [(5, 3), (25, 16)], d_dst),
             ("a window one pixel below", good, [(5, 17), (24, 16)], d_dst),
             ("pixel_stride < C", three, org, d_dst),
             ("d_dst not 16-byte aligned", good, org, d_dst[4:]),
             ("row_pitch no multiple of 4 with 4-byte pixels", odd, org, d_dst)]
    for what, dst, o, d in cases:
        with pytest.raises(himg_amd.HimgError) as e:
            eng.decode_into_device(d_in, stride, sizes, 2, W, H, Cn, d, dst, o, d_st)
        assert e.value.code == himg_amd.HIMG_ERR_ARG, what
        with pytest.raises(himg_amd.HimgError) as e:
            eng.decode_regions_into_device(d_in, stride, sizes, 2, W, H, Cn, [(0, 0), (0, 0)], W, H, d, dst, o, d_st)
        assert e.value.code == himg_amd.HIMG_ERR_ARG, what
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == -99).all()
    assert np.array_equal(d_dst.cpu().numpy(), bg)
    # ... and the same arguments, put right, decode
    eng.decode_into_device(d_in, stride, sizes, 2, W, H, Cn, d_dst, good, org, d_st)
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == 0).all()


# ---- 7. Engine.decode_into: a host stream into a host picture -----------------------------------

@pytest.mark.parametrize("W,H,Cn,ps", [(203, 21, 4, 4), (100, 37, 3, 4)])
def test_engine_decode_into(eng, W, H, Cn, ps):
    b = _stream("randtile", W, H, Cn, 50, True, seed=2)
    pic = _pictures(eng, [b], H, W, Cn)[0]
    dst = _padded(W + 24, H + 16, ps, one_picture=True)
    data = _background(dst, 1, seed=7)
    want = data.copy()
    _paste(want, dst, 0, 5, 3, pic)
    assert eng.decode_into(b, data, dst, 5, 3) == (W, H, Cn)
    assert np.array_equal(data, want)
    # a picture that does not fit at (x, y) is refused and nothing is written
    with pytest.raises(himg_amd.HimgError) as e:
        eng.decode_into(b, data, dst, 25, 3)
    assert e.value.code == himg_amd.HIMG_ERR_ARG
    assert np.array_equal(data, want)
