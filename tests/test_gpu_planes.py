"""GPU: the planes decode -- decode_planes_device and decode_planes against the model
(tests/planes_model.py: the oracle's decode of the stream rewritten to colour space 0 with one shift
table), byte for byte; every store form (the fused row kernel's <512>, <-1> and <0> forms, both
k_tile_inv forms), every mask of 1-3 channel streams and luma / alpha / chroma / YCbCr / all of RGBA,
both colour branches; the profiler's stage names say which kernel ran; a sentinel behind the output,
the buffer refilled between masks; the planes recombined through the colour inverse in numpy against
decode_device; damaged frames in a batch; the host form and its capacity report; argument errors that
leave the outputs alone; a caller's stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import damage_model as dm
import himg_amd
import oracle_lib as ol
import planes_model as pm
from test_gpu_region import _stream
from test_gpu_regions import _upload

pytestmark = pytest.mark.gpu

U8_STORE_STAGES = {"k_dec_row_fused", "k_tile_inv<true>", "k_tile_inv<false>", "k_dec_region"}
TAIL = 64


@pytest.fixture
def eng(engine):
    """The session's engine; HIMG_OPT_FIX_T2 back to the default behind every test."""
    yield engine
    engine.set_option("fix_t2", 0)


def _models(eng, streams):
    """The model's [C][H][W] planes of every stream.  Where the oracle rejects one under the T2 rule both
    the engine and the oracle run in the fixed mode -- streams the reference accepts decode identically
    either way (test_gpu_tensor._pictures)."""
    fix = any(ol.oracle_decode(s)[0] != 0 for s in streams)
    eng.set_option("fix_t2", int(fix))
    out = []
    for s in streams:
        rc, pl = pm.planes(s, fix_t2=fix)
        assert rc == 0
        out.append(pl)
    return out


def _masks(Cn):
    return [0x1, 0x8, 0x6, 0x7, 0xF] if Cn == 4 else list(range(1, 1 << Cn))


def _planes(eng, d_in, stride, sizes, W, H, Cn, mask, stream=0):
    """One call into a freshly filled buffer: (status words, [n][P][H][W] on the GPU), the sentinel checked."""
    n, P = len(sizes), bin(mask).count("1")
    nbytes = n * himg_amd.planes_bytes(Cn, mask, W, H)
    assert nbytes == n * P * H * W
    d_out = torch.full((nbytes + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.decode_planes_device(d_in, stride, sizes, n, W, H, Cn, mask, d_out, d_st, stream=stream)
    torch.cuda.synchronize()
    assert (d_out[nbytes:] == 0x5A).all().item(), "the sentinel behind the last plane was overwritten"
    return d_st.cpu().numpy(), d_out[:nbytes].view(n, P, H, W)


def _same(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d bytes differ, first at %s: got %d, expected %d"
                             % (what, bad.shape[0], i, int(got[i]), int(want[i])))


def _decode_device(eng, d_in, stride, sizes, W, H, Cn):
    n = len(sizes)
    d_pix = torch.full((n, H, W, Cn), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_device(d_in, stride, sizes, n, W, H, Cn, d_pix, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_pix


# W, H, C, qualities, batch, the stage that must have run, colour lift also off
SHAPES = [
    (4096, 24, 4, (50, 90), 3, "k_dec_row_fused_c<512>", True),     # 8-byte stores, three block rows
    (2048, 16, 4, (50,), 2, "k_dec_row_fused_c<-1>", False),
    # 33 tile columns (across the 32-tile wavefront boundary), several rows per workgroup, more grid
    # elements than CUs: the persistent loop and its per_row * nr < 1024 tail
    (264, 40, 4, (50,), 300, "k_dec_row_fused_c<-1>", False),
    (203, 21, 4, (50,), 2, "k_dec_row_fused_c<0>", True),            # RGBA, ragged right and bottom tiles
    (100, 37, 3, (90,), 2, "k_dec_row_fused_c<0>", True),            # 1-3 channels
    (67, 19, 1, (50,), 2, "k_dec_row_fused_c<0>", False),
    (1000, 16, 2, (50,), 2, "k_dec_row_fused_c<0>", False),
    (8192, 16, 4, (50,), 2, "k_tile_inv_c<true>", True),             # rows through HBM
    (6001, 9, 3, (50,), 1, "k_tile_inv_c<false>", False),            # ... ragged
]


@pytest.mark.parametrize("W,H,Cn,quals,batch,stage,also_rgb", SHAPES)
def test_planes_byte_exact(eng, W, H, Cn, quals, batch, stage, also_rgb):
    nsrc = min(batch, 3)
    for q in quals:
        for ycbcr in ([True, False] if also_rgb else [True]):
            streams = [_stream("randtile", W, H, Cn, q, ycbcr, seed=s) for s in range(nsrc)]
            cs = pm.header(streams[0])[3]
            assert cs == (1 if ycbcr and Cn >= 3 else 0)
            models = torch.from_numpy(np.stack(_models(eng, streams))).cuda()
            pick = [f % nsrc for f in range(batch)]
            d_in, stride = _upload([streams[k] for k in pick])
            sizes = [len(streams[k]) for k in pick]
            want_all = models[torch.tensor(pick, device="cuda")]
            st_u8, d_pix = _decode_device(eng, d_in, stride, sizes, W, H, Cn)
            assert (st_u8 == 0).all()
            for mask in _masks(Cn):
                sel = [c for c in range(Cn) if (mask >> c) & 1]
                eng.profile(True)
                eng.profile_reset()
                st, got = _planes(eng, d_in, stride, sizes, W, H, Cn, mask)
                stages = eng.profile_read()
                eng.profile(False)
                what = "%dx%dx%d q%d ycbcr=%d mask %#x" % (W, H, Cn, q, ycbcr, mask)
                assert np.array_equal(st, st_u8), (what, st)
                assert stage in stages and not (U8_STORE_STAGES & set(stages)), (what, sorted(stages))
                _same(got, want_all[:, sel], what)
                if len(sel) == Cn or (Cn == 4 and mask == 0x7):
                    # the planes through the colour inverse in numpy: decode_device's picture (mask 0x7: its RGB)
                    g = got.cpu().numpy()
                    pic = d_pix.cpu().numpy()
                    for f in sorted(set(range(min(batch, 4))) | {batch - 1}):
                        assert np.array_equal(pm.to_picture(g[f], cs), pic[f][:, :, :len(sel)]), (what, f)


def test_damaged_frames(eng):
    """Damaged frames among sound ones: a head failure (no RIFF file; FRMT's width), a block row the row
    kernel rejects, and a stream the T2 rule rejects -- without the fix, then with it.  The status words
    are decode_device's, word for word; sound neighbours are exact."""
    W, H, Cn = 264, 40, 4
    good = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(4)]
    first, width = good[1].copy(), good[2].copy()
    first[0] ^= 0x01          # the first byte: no RIFF file
    width[21] ^= 0x10         # FRMT's width field: 264 -> 280
    for bad in (first, width):
        assert -6 <= ol.oracle_decode(bad)[0] <= -1
    # one block row's payload damaged until the oracle rejects the stream in its FRES rows
    _, ranges = dm.rows_of(good[3])
    off, length = ranges[2]
    row = None
    for k in range(64):
        cand = good[3].copy()
        cand[off + (7 * k + 3) % length] ^= 1 << (k % 8)
        if ol.oracle_decode(cand)[0] == -7:
            row = cand
            break
    assert row is not None
    flat = np.frombuffer(ol.oracle_encode(np.full((H, W, Cn), 90, np.uint8), 50, True), np.uint8).copy()
    assert ol.oracle_decode(flat)[0] != 0 and ol.oracle_decode(flat, fix_t2=True)[0] == 0   # the T2 rule
    streams = [good[0], first, flat, width, good[1], row, good[3]]
    sound = [0, 4, 6]
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    n = len(streams)
    for fix in (0, 1):
        eng.set_option("fix_t2", fix)
        st_u8, _ = _decode_device(eng, d_in, stride, sizes, W, H, Cn)
        ok = sound + ([2] if fix else [])
        assert all((st_u8[f] == 0) == (f in ok) for f in range(n)), (fix, st_u8)
        want = {f: torch.from_numpy(pm.planes(streams[f], fix_t2=bool(fix))[1]).cuda() for f in ok}
        for mask in (0x1, 0x8, 0x6, 0xF):
            sel = [c for c in range(Cn) if (mask >> c) & 1]
            for rnd in range(2):   # the same call twice on one engine
                st, got = _planes(eng, d_in, stride, sizes, W, H, Cn, mask)
                assert np.array_equal(st, st_u8), (fix, mask, rnd, st, st_u8)
                for f in ok:
                    _same(got[f], want[f][sel], "fix %d frame %d mask %#x round %d" % (fix, f, mask, rnd))


def test_host_form_and_capacity(eng):
    L = himg_amd.lib()
    for W, H, Cn, q in [(203, 21, 4, 50), (100, 37, 3, 90), (67, 19, 1, 50), (4096, 24, 4, 50)]:
        s = _stream("randtile", W, H, Cn, q, True)
        model = _models(eng, [s])[0]
        d_in, stride = _upload([s])
        for mask in _masks(Cn):
            P = bin(mask).count("1")
            st, dev = _planes(eng, d_in, stride, [len(s)], W, H, Cn, mask)
            assert (st == 0).all()
            got = eng.decode_planes(s, mask)
            assert got.shape == (P, H, W) and got.dtype == np.uint8
            assert np.array_equal(got, dev[0].cpu().numpy()) and np.array_equal(got, pm.select(model, mask))
            # the capacity report: the geometry with HIMG_ERR_CAPACITY, nothing written
            w, h, c = C.c_int(), C.c_int(), C.c_int()
            assert L.himg_hip_decode_planes_to(eng._ctx, s.ctypes.data, s.nbytes, mask, None, 0,
                                               C.byref(w), C.byref(h), C.byref(c)) == himg_amd.HIMG_ERR_CAPACITY
            assert (w.value, h.value, c.value) == (W, H, Cn)
            short = np.full(P * H * W - 1, 0x5A, np.uint8)
            assert L.himg_hip_decode_planes_to(eng._ctx, s.ctypes.data, s.nbytes, mask, short.ctypes.data, short.nbytes,
                                               C.byref(w), C.byref(h), C.byref(c)) == himg_amd.HIMG_ERR_CAPACITY
            assert (short == 0x5A).all()
            # `out` is reused when it fits
            buf = np.empty(P * H * W, np.uint8)
            again = eng.decode_planes(s, mask, out=buf)
            assert np.shares_memory(again, buf) and np.array_equal(again, got)
        for mask in (0, 1 << Cn, 0x10, 0x80000001):
            with pytest.raises(himg_amd.HimgError) as e:
                eng.decode_planes(s, mask)
            assert e.value.code == himg_amd.HIMG_ERR_ARG, (Cn, mask)
    bad = s.copy()
    bad[0] ^= 1
    with pytest.raises(himg_amd.HimgError) as e:
        eng.decode_planes(bad, 1)
    assert e.value.code == himg_amd.HIMG_ERR_FORMAT


def test_argument_errors(engine):
    W, H, Cn = 96, 48, 3
    b = _stream("randtile", W, H, Cn, 50, True)
    d_in, stride = _upload([b, b])
    sizes = [len(b)] * 2
    L = himg_amd.lib()
    hs = np.ascontiguousarray(sizes, np.uint32)

    def call(ctx, packed, hsz, mask, out, status, batch=2, shift=0):
        d_out = torch.full((2 * Cn * H * W + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.full((2,), -99, dtype=torch.int32, device="cuda")
        rc = L.himg_hip_decode_planes_device(ctx, d_in.data_ptr() if packed else None, stride,
                                             hs.ctypes.data if hsz else None, batch, W, H, Cn, mask,
                                             d_out.data_ptr() + shift if out else None,
                                             d_st.data_ptr() if status else None, None)
        torch.cuda.synchronize()
        assert (d_out == 0x5A).all().item() and (d_st.cpu().numpy() == -99).all()
        return rc

    ctx = engine._ctx
    cases = {"mask 0": (ctx, 1, 1, 0, 1, 1), "bit C": (ctx, 1, 1, 1 << Cn, 1, 1), "bit 3 of RGB": (ctx, 1, 1, 0x9, 1, 1),
             "bit 31": (ctx, 1, 1, 0x80000001, 1, 1), "no context": (None, 1, 1, 1, 1, 1), "no input": (ctx, 0, 1, 1, 1, 1),
             "no sizes": (ctx, 1, 0, 1, 1, 1), "no output": (ctx, 1, 1, 1, 0, 1), "no status": (ctx, 1, 1, 1, 1, 0)}
    for what, args in cases.items():
        assert call(*args) == himg_amd.HIMG_ERR_ARG, what
    assert call(ctx, 1, 1, 1, 1, 1, batch=0) == himg_amd.HIMG_ERR_ARG
    assert call(ctx, 1, 1, 1, 1, 1, shift=2) == himg_amd.HIMG_ERR_ARG   # d_out's base: 16-byte aligned
    # ... and the same arguments with nothing wrong go through
    st, _ = _planes(engine, d_in, stride, sizes, W, H, Cn, 0x5)
    assert (st == 0).all()


def test_on_a_callers_stream(eng):
    W, H, Cn, mask = 264, 40, 4, 0x9
    streams = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(3)]
    models = _models(eng, streams)
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    side = torch.cuda.Stream()
    n, P = len(streams), 2
    d_out = torch.full((n * P * H * W + TAIL,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.decode_planes_device(d_in, stride, sizes, n, W, H, Cn, mask, d_out, d_st, stream=side.cuda_stream)
    side.synchronize()
    assert (d_st.cpu().numpy() == 0).all() and (d_out[n * P * H * W:] == 0x5A).all().item()
    got = d_out[:n * P * H * W].view(n, P, H, W).cpu().numpy()
    for f in range(n):
        assert np.array_equal(got[f], pm.select(models[f], mask)), f
