"""GPU: the tensor decode -- decode_tensor_device and decode_regions_tensor_device against the numpy
model (tests/tensor_model.py) applied to the oracle's decode of the same stream, bit for bit on the
integer view of the output; every store form (the fused row kernel's <512>, <-1> and <0> forms, both
k_tile_inv forms, the region kernel), every dtype and channel count, both colour branches; the
profiler's stage names say which kernel ran; sentinels behind the output; damaged frames in a
batch; argument errors that leave the outputs alone."""
import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol
import tensor_model as tm
from test_gpu_region import _full, _stream
from test_gpu_regions import _upload

pytestmark = pytest.mark.gpu

IVIEW = {tm.F32: torch.int32, tm.F16: torch.int16, tm.BF16: torch.int16}
NPI = {tm.F32: np.int32, tm.F16: np.int16, tm.BF16: np.int16}
U8_STORE_STAGES = {"k_dec_row_fused", "k_tile_inv<true>", "k_tile_inv<false>", "k_dec_region"}
TAIL = 64


@pytest.fixture
def eng(engine):
    """The session's engine; HIMG_OPT_FIX_T2 back to the default behind every test."""
    yield engine
    engine.set_option("fix_t2", 0)


def _pictures(eng, streams, H, W, Cn):
    """The oracle's decode of every stream.  Streams of few block rows are among those the reference
    decoder rejects although its own encoder wrote them (HIMG_OPT_FIX_T2): then both the oracle and
    the engine decode in the fixed mode -- streams the reference accepts decode identically either way."""
    fix = any(ol.oracle_decode(s)[0] != 0 for s in streams)
    eng.set_option("fix_t2", int(fix))
    return [_full(s, fix).reshape(H, W, Cn) for s in streams]


def _out(nbytes):
    return torch.full((nbytes + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")


def _view(d_out, nbytes, dtype, shape):
    assert (d_out[nbytes:] == 0x5A).all().item(), "the sentinel behind the last element was overwritten"
    return d_out[:nbytes].view(IVIEW[dtype]).view(*shape)


def _tensor(eng, d_in, stride, sizes, W, H, Cn, desc):
    n = len(sizes)
    nbytes = n * himg_amd.tensor_bytes(desc, Cn, W, H)
    d_out = _out(nbytes)
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_tensor_device(d_in, stride, sizes, n, W, H, Cn, desc, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), _view(d_out, nbytes, desc.dtype, (n, desc.out_channels, H, W))


def _regions_tensor(eng, d_in, stride, sizes, W, H, Cn, org, w, h, desc):
    n = len(sizes)
    nbytes = n * himg_amd.tensor_bytes(desc, Cn, w, h)
    d_out = _out(nbytes)
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_regions_tensor_device(d_in, stride, sizes, n, W, H, Cn, org, w, h, desc, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), _view(d_out, nbytes, desc.dtype, (n, desc.out_channels, h, w))


def _expected(pics, name, dtype, Cn):
    """[stream][C][H][W] integer views on the GPU of the model's tensor for Co = C; fewer output
    channels are its first planes (a channel's table does not depend on Co)."""
    desc = tm.DESCS[name](dtype, Cn)
    return torch.from_numpy(np.stack([tm.expected(p, desc).view(NPI[dtype]) for p in pics])).cuda()


def _same(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d elements differ, first at %s: got %#x, expected %#x"
                             % (what, bad.shape[0], i, int(got[i]) & 0xFFFFFFFF, int(want[i]) & 0xFFFFFFFF))


# W, H, C, qualities, batch, the stage that must have run, colour lift also off
SHAPES = [
    (4096, 24, 4, (50, 90), 3, "k_dec_row_fused_t<512>", True),     # 16-byte stores, three block rows
    (2048, 16, 4, (50,), 2, "k_dec_row_fused_t<-1>", False),         # the other BASELINE widths
    (1920, 16, 4, (50,), 2, "k_dec_row_fused_t<-1>", False),
    # 33 tile columns (across the 32-tile wavefront boundary), several rows per workgroup, more grid
    # elements than CUs: the persistent loop and its per_row * nr < 1024 tail
    (264, 40, 4, (50,), 300, "k_dec_row_fused_t<-1>", False),
    (203, 21, 4, (50,), 2, "k_dec_row_fused_t<0>", True),            # RGBA, ragged right and bottom tiles
    (100, 37, 3, (90,), 2, "k_dec_row_fused_t<0>", True),            # 1-3 channels
    (67, 19, 1, (50,), 2, "k_dec_row_fused_t<0>", False),
    (1000, 16, 2, (50,), 2, "k_dec_row_fused_t<0>", False),
    (8192, 16, 4, (50,), 2, "k_tile_inv_t<true>", True),             # rows through HBM
    (6001, 9, 3, (50,), 1, "k_tile_inv_t<false>", False),            # ... ragged
]


@pytest.mark.parametrize("W,H,Cn,quals,batch,stage,also_rgb", SHAPES)
def test_full_decode_bit_exact(eng, W, H, Cn, quals, batch, stage, also_rgb):
    engine = eng
    nsrc = min(batch, 3)
    for q in quals:
        for ycbcr in ([True, False] if also_rgb else [True]):
            streams = [_stream("randtile", W, H, Cn, q, ycbcr, seed=s) for s in range(nsrc)]
            pics = _pictures(engine, streams, H, W, Cn)
            pick = [f % nsrc for f in range(batch)]
            d_in, stride = _upload([streams[k] for k in pick])
            sizes = [len(streams[k]) for k in pick]
            d_pick = torch.tensor(pick, device="cuda")
            for dtype in tm.DTYPES:
                for name in ("imagenet", "mix"):
                    want = _expected(pics, name, dtype, Cn)[d_pick]
                    for co in range(1, Cn + 1):
                        if name == "mix" and co != Cn:
                            continue
                        desc = tm.DESCS[name](dtype, co)
                        engine.profile(True)
                        engine.profile_reset()
                        st, got = _tensor(engine, d_in, stride, sizes, W, H, Cn, desc)
                        stages = engine.profile_read()
                        engine.profile(False)
                        assert (st == 0).all(), (q, ycbcr, dtype, co, st)
                        assert stage in stages and not (U8_STORE_STAGES & set(stages)), (stage, sorted(stages))
                        _same(got, want[:, :co], "%dx%dx%d q%d ycbcr=%d dtype=%d %s Co=%d" % (W, H, Cn, q, ycbcr, dtype, name, co))


@pytest.mark.parametrize("W,H,Cn,q,batch", [(4096, 24, 4, 50, 2), (264, 40, 4, 50, 3), (203, 21, 4, 50, 2),
                                            (100, 37, 3, 90, 2), (8192, 16, 4, 50, 2), (6001, 9, 3, 50, 1)])
def test_identity_is_the_engines_own_decode(eng, W, H, Cn, q, batch):
    engine = eng
    streams = [_stream("randtile", W, H, Cn, q, True, seed=s) for s in range(batch)]
    _pictures(engine, streams, H, W, Cn)   # (the decode mode these streams need)
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    d_pix = torch.full((batch, H, W, Cn), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((batch,), -99, dtype=torch.int32, device="cuda")
    engine.decode_device(d_in, stride, sizes, batch, W, H, Cn, d_pix, d_st)
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == 0).all()
    want = np.ascontiguousarray(d_pix.cpu().numpy().transpose(0, 3, 1, 2)).astype(np.float32).view(np.int32)
    st, got = _tensor(engine, d_in, stride, sizes, W, H, Cn, tm.identity(tm.F32, Cn))
    assert (st == 0).all()
    assert np.array_equal(got.cpu().numpy(), want)


def test_damaged_frames(engine):
    W, H, Cn = 264, 40, 4
    good = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(4)]
    first, width = good[1].copy(), good[2].copy()
    first[0] ^= 0x01          # the first byte: no RIFF file
    width[21] ^= 0x10         # FRMT's width field: 264 -> 280
    # the reference rejects both in its container stages (the oracle returns -stage, 1..6)
    for bad in (first, width):
        assert -6 <= ol.oracle_decode(bad)[0] <= -1
    streams = [good[0], first, width, good[3]]
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    d_pix = torch.empty((4, H, W, Cn), dtype=torch.uint8, device="cuda")
    d_st = torch.full((4,), -99, dtype=torch.int32, device="cuda")
    engine.decode_device(d_in, stride, sizes, 4, W, H, Cn, d_pix, d_st)
    torch.cuda.synchronize()
    st_u8 = d_st.cpu().numpy()
    assert st_u8[0] == 0 and st_u8[3] == 0 and st_u8[1] != 0 and st_u8[2] != 0, st_u8
    pics = [_full(good[0]).reshape(H, W, Cn), _full(good[3]).reshape(H, W, Cn)]
    for dtype in tm.DTYPES:
        want = _expected(pics, "imagenet", dtype, Cn)
        for co in (3, 4):
            desc = tm.imagenet(dtype, co)
            for rnd in range(2):   # the same call twice on one engine
                st, got = _tensor(engine, d_in, stride, sizes, W, H, Cn, desc)
                assert np.array_equal(st, st_u8), (dtype, co, rnd, st, st_u8)
                _same(got[0], want[0, :co], "frame 0 dtype=%d Co=%d round %d" % (dtype, co, rnd))
                _same(got[3], want[1, :co], "frame 3 dtype=%d Co=%d round %d" % (dtype, co, rnd))


def test_argument_errors(engine):
    W, H, Cn = 96, 48, 4
    b = _stream("randtile", W, H, Cn, 50, True)
    d_in, stride = _upload([b, b])
    sizes = [len(b)] * 2

    def broken(what, field, value, slot=None):
        d = tm.imagenet(tm.F16, 3)
        if slot is None:
            setattr(d, field, value)
        else:
            getattr(d, field)[slot] = value
        return what, d

    def descs():
        yield broken("dtype 3", "dtype", 3)
        yield broken("dtype -1", "dtype", -1)
        yield broken("Co = 0", "out_channels", 0)
        yield broken("Co = C + 1", "out_channels", Cn + 1)
        yield broken("inf scale", "scale", float("inf"), 1)
        yield broken("nan bias", "bias", float("nan"), 2)

    good = tm.imagenet(tm.F16, 3)
    org_ok, org_bad = np.array([(0, 0), (8, 8)], np.int32), np.array([(0, 0), (57, 0)], np.int32)
    w, h = 40, 8
    cases = [(what, d, 0, org_ok) for what, d in descs()] + [("d_out + 2", good, 2, org_ok)]
    for what, desc, shift, org in cases + [("origin", good, 0, org_bad)]:
        for regions in (False, True):
            if what == "origin" and not regions:
                continue
            d_out = torch.full((2 * 4 * H * W * 4 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            d_st = torch.full((2,), -99, dtype=torch.int32, device="cuda")
            with pytest.raises(himg_amd.HimgError) as e:
                if regions:
                    engine.decode_regions_tensor_device(d_in, stride, sizes, 2, W, H, Cn, org, w, h, desc, d_out[shift:], d_st)
                else:
                    engine.decode_tensor_device(d_in, stride, sizes, 2, W, H, Cn, desc, d_out[shift:], d_st)
            assert e.value.code == himg_amd.HIMG_ERR_ARG, (what, regions)
            torch.cuda.synchronize()
            assert (d_out == 0x5A).all().item() and (d_st.cpu().numpy() == -99).all(), (what, regions)
    # ... and the same arguments with nothing wrong go through
    st, _ = _regions_tensor(engine, d_in, stride, sizes, W, H, Cn, org_ok, w, h, good)
    assert (st == 0).all()


def _origins(W, H, w, h):
    """The four corners, (7, 7), (8, 7), (7, 8), (16, 15), each within the frame."""
    X, Y = W - w, H - h
    o = [(0, 0), (X, 0), (0, Y), (X, Y)] + [(min(a, X), min(b, Y)) for a, b in [(7, 7), (8, 7), (7, 8), (16, 15)]]
    return np.array(list(dict.fromkeys(o)), np.int32)


REGION_SHAPES = [(4096, 24, 4, 50), (264, 40, 4, 50), (203, 21, 4, 50), (100, 37, 3, 90), (8192, 16, 4, 50)]


@pytest.mark.parametrize("W,H,Cn,q", REGION_SHAPES)
def test_regions_bit_exact(eng, W, H, Cn, q):
    engine = eng
    streams = [_stream("randtile", W, H, Cn, q, True, seed=s) for s in range(2)]
    pics = _pictures(engine, streams, H, W, Cn)
    full = {dtype: _expected(pics, "imagenet", dtype, Cn) for dtype in tm.DTYPES}
    # 1 x 1, the whole picture, one that holds the last (ragged) tile from the corner origin, 129 x 13,
    # and at 8192 pixels one across two column strips
    wins = [(1, 1), (W, H), (min(W, 13), min(H, 7)), (min(W, 129), 13)] + ([(5000, 9)] if W == 8192 else [])
    for w, h in wins:
        org = _origins(W, H, w, h)
        n = len(org)
        pick = [f % 2 for f in range(n)]
        d_in, stride = _upload([streams[k] for k in pick])
        sizes = [len(streams[k]) for k in pick]
        d_u8 = torch.full((n * h * w * Cn + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        engine.decode_regions_device(d_in, stride, sizes, n, W, H, Cn, org, w, h, d_u8, d_st)
        torch.cuda.synchronize()
        st_u8 = d_st.cpu().numpy()
        assert (st_u8 == 0).all()
        for dtype in tm.DTYPES:
            want = torch.stack([full[dtype][pick[f], :, y:y + h, x:x + w] for f, (x, y) in enumerate(org.tolist())])
            for co in sorted({1, min(3, Cn), Cn}):
                desc = tm.imagenet(dtype, co)
                engine.profile(True)
                engine.profile_reset()
                st, got = _regions_tensor(engine, d_in, stride, sizes, W, H, Cn, org, w, h, desc)
                stages = engine.profile_read()
                engine.profile(False)
                assert np.array_equal(st, st_u8), (w, h, dtype, co, st)
                assert "k_dec_region_t" in stages and not (U8_STORE_STAGES & set(stages)), sorted(stages)
                _same(got, want[:, :co], "%dx%dx%d window %dx%d dtype=%d Co=%d" % (W, H, Cn, w, h, dtype, co))
                if (w, h) == (W, H):   # the whole picture: decode_tensor_device's output
                    st2, got2 = _tensor(engine, d_in, stride, sizes, W, H, Cn, desc)
                    assert (st2 == 0).all()
                    _same(got, got2, "whole-picture window against the full decode, dtype=%d Co=%d" % (dtype, co))


def test_region_verdicts_per_frame(engine):
    """A damaged frame among good ones: the statuses are decode_regions_device's, the good frames' crops exact."""
    W, H, Cn, w, h = 264, 40, 4, 50, 20
    good = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(2)]
    bad = good[1].copy()
    bad[0] ^= 0x01
    streams = [good[0], bad, good[1]]
    org = np.array([(7, 7), (0, 0), (W - w, H - h)], np.int32)
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    d_u8 = torch.empty((3 * h * w * Cn,), dtype=torch.uint8, device="cuda")
    d_st = torch.full((3,), -99, dtype=torch.int32, device="cuda")
    engine.decode_regions_device(d_in, stride, sizes, 3, W, H, Cn, org, w, h, d_u8, d_st)
    torch.cuda.synchronize()
    st_u8 = d_st.cpu().numpy()
    assert st_u8[0] == 0 and st_u8[1] != 0 and st_u8[2] == 0
    pics = [_full(s).reshape(H, W, Cn) for s in good]
    for dtype in tm.DTYPES:
        full = _expected(pics, "imagenet", dtype, Cn)
        st, got = _regions_tensor(engine, d_in, stride, sizes, W, H, Cn, org, w, h, tm.imagenet(dtype, 3))
        assert np.array_equal(st, st_u8)
        _same(got[0], full[0, :3, 7:7 + h, 7:7 + w], "frame 0 dtype=%d" % dtype)
        _same(got[2], full[1, :3, H - h:, W - w:], "frame 2 dtype=%d" % dtype)
