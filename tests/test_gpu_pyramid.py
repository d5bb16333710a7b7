"""GPU: the pyramid decode -- decode_pyramid_device's four levels against two judges each, the CPU
models (the oracle's decode, tests/scaled_model.py, the preview model of test_gpu_preview) and the
existing device entry points run on the same upload, byte for byte; every store form (the fused row
kernel's <512>, <-1> and <0> pyramid forms, both k_tile_inv_m forms) with the profiler's stage names
saying which one ran; every subset of the levels, with sentinels behind each level and nothing written
for a level that is not wanted; damaged frames in a batch (one verdict per frame, the full decode's);
argument errors that leave everything alone; Engine.decode_pyramid and its capacity rule."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol
import scaled_model as sm
from test_gpu_preview import expected as preview_expected
from test_gpu_region import _full, _stream
from test_gpu_regions import _upload

pytestmark = pytest.mark.gpu

TAIL = 64
POISON = 0x5A
# the stages that store a level's pixels in the entry points of their own
OTHER_STORE_STAGES = {"k_dec_row_fused", "k_tile_inv<true>", "k_tile_inv<false>", "k_dec_scaled"}


@pytest.fixture
def eng(engine):
    """The session's engine; HIMG_OPT_FIX_T2 back to the default behind every test."""
    yield engine
    engine.set_option("fix_t2", 0)


def _fix_mode(eng, streams):
    """test_gpu_tensor._pictures' rule: streams of few block rows are among those the reference decoder
    rejects although its own encoder wrote them -- then the oracle and the engine both decode in the
    fixed mode (streams the reference accepts decode identically either way)."""
    fix = any(ol.oracle_decode(s)[0] != 0 for s in streams)
    eng.set_option("fix_t2", int(fix))
    return fix


def _dims(W, H, k):
    f = 1 << k
    return (H + f - 1) // f, (W + f - 1) // f


def _models(s, fix, H, W, Cn):
    """The four levels of one stream by the CPU models."""
    out = {0: _full(s, fix).reshape(H, W, Cn)}
    for k in (1, 2):
        rc, pic = sm.expected(s, k, fix)
        assert rc == 0
        out[k] = pic
    rc, low = preview_expected(s, fix)
    assert rc == 0
    out[3] = low
    for k in range(4):
        assert out[k].shape == _dims(W, H, k) + (Cn,), (k, out[k].shape)
    return out


def _buffers(n, W, H, Cn):
    """A poisoned buffer per level with a sentinel tail: {level: (tensor, bytes)}."""
    bufs = {}
    for k in range(4):
        oh, ow = _dims(W, H, k)
        nb = n * oh * ow * Cn
        bufs[k] = (torch.full((nb + TAIL,), POISON, dtype=torch.uint8, device="cuda"), nb)
    return bufs


def _pyramid(eng, d_in, stride, sizes, W, H, Cn, levels=(0, 1, 2, 3), bufs=None):
    """decode_pyramid_device of `levels`: (statuses, {level: [n][oh][ow][C] array}, the buffers).  The
    sentinels behind the wanted levels are checked, and every byte of the buffers of the others."""
    n = len(sizes)
    bufs = bufs or _buffers(n, W, H, Cn)
    desc = himg_amd.pyramid_desc(*[bufs[k][0] if k in levels else None for k in range(4)])
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_pyramid_device(d_in, stride, sizes, n, W, H, Cn, desc, d_st)
    torch.cuda.synchronize()
    got = {}
    for k in range(4):
        t, nb = bufs[k]
        if k in levels:
            assert (t[nb:] == POISON).all().item(), "level %d: the sentinel behind the last byte was overwritten" % k
            got[k] = t[:nb].cpu().numpy().reshape((n,) + _dims(W, H, k) + (Cn,))
        else:
            assert (t == POISON).all().item(), "level %d is not wanted and was written" % k
    return d_st.cpu().numpy(), got, bufs


def _entry_points(eng, d_in, stride, sizes, W, H, Cn):
    """The four levels by the entry points of their own, on the same upload: (statuses of the full decode, levels)."""
    n = len(sizes)
    out, st0 = {}, None
    for k in range(4):
        oh, ow = _dims(W, H, k)
        d_out = torch.full((n, oh, ow, Cn), POISON, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        if k == 0:
            eng.decode_device(d_in, stride, sizes, n, W, H, Cn, d_out, d_st)
        elif k == 3:
            eng.preview_device(d_in, stride, sizes, n, W, H, Cn, d_out, d_st)
        else:
            eng.decode_scaled_device(d_in, stride, sizes, n, W, H, Cn, k, d_out, d_st)
        torch.cuda.synchronize()
        out[k] = d_out.cpu().numpy()
        if k == 0:
            st0 = d_st.cpu().numpy()
    return st0, out


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d bytes differ, first at %s: got %d, expected %d" % (what, len(bad), i, got[i], want[i]))


# W, H, C, qualities, batch, the stage that must have run, colour lift also off
SHAPES = [
    (4096, 24, 4, (50, 90), 3, "k_dec_row_fused_m<512>", True),     # three block rows
    (2048, 16, 4, (50,), 2, "k_dec_row_fused_m<-1>", False),
    (1920, 16, 4, (50,), 2, "k_dec_row_fused_m<-1>", False),
    # 33 tile columns, several rows per workgroup, more grid elements than CUs: the persistent loop and its tail
    (264, 40, 4, (50,), 300, "k_dec_row_fused_m<-1>", False),
    (203, 21, 4, (50,), 2, "k_dec_row_fused_m<0>", True),
    (100, 37, 3, (50,), 2, "k_dec_row_fused_m<0>", True),
    (67, 19, 1, (50,), 2, "k_dec_row_fused_m<0>", False),
    (1000, 16, 2, (50,), 2, "k_dec_row_fused_m<0>", False),
    (8192, 16, 4, (50,), 2, "k_tile_inv_m<true>", True),             # rows through HBM
    (6001, 9, 3, (50,), 1, "k_tile_inv_m<false>", False),            # ... ragged
    (8, 8, 4, (50,), 2, "k_dec_row_fused_m<-1>", False),             # one tile
    (1, 1, 1, (50,), 2, "k_dec_row_fused_m<0>", False),              # every level one sample
    (7, 5, 3, (50,), 2, "k_dec_row_fused_m<0>", True),               # ragged single tile: ceil differs from floor at every level
    (9, 17, 4, (50,), 2, "k_dec_row_fused_m<0>", True),              # ragged right and bottom
]


@pytest.mark.parametrize("W,H,Cn,quals,batch,stage,also_rgb", SHAPES)
def test_levels_bit_exact(eng, W, H, Cn, quals, batch, stage, also_rgb):
    nsrc = min(batch, 3)
    for q in quals:
        for ycbcr in ([True, False] if also_rgb else [True]):
            what = "%dx%dx%d q%d ycbcr=%d" % (W, H, Cn, q, ycbcr)
            streams = [_stream("randtile", W, H, Cn, q, ycbcr, seed=s) for s in range(nsrc)]
            fix = _fix_mode(eng, streams)
            models = [_models(s, fix, H, W, Cn) for s in streams]
            pick = [f % nsrc for f in range(batch)]
            d_in, stride = _upload([streams[k] for k in pick])
            sizes = [len(streams[k]) for k in pick]
            eng.profile(True)
            eng.profile_reset()
            st, got, _ = _pyramid(eng, d_in, stride, sizes, W, H, Cn)
            stages = eng.profile_read()
            eng.profile(False)
            assert (st == 0).all(), (what, st)
            assert stage in stages and "k_lres_preview" in stages and not (OTHER_STORE_STAGES & set(stages)), \
                (stage, sorted(stages))
            st0, ref = _entry_points(eng, d_in, stride, sizes, W, H, Cn)
            assert (st0 == 0).all()
            for k in range(4):
                _same(got[k], np.stack([models[p][k] for p in pick]), "%s level %d against the CPU model" % (what, k))
                _same(got[k], ref[k], "%s level %d against its own entry point" % (what, k))


SUBSETS = [c for r in range(1, 5) for c in itertools.combinations(range(4), r)]


@pytest.mark.parametrize("W,H,Cn", [(203, 21, 4), (4096, 16, 4)])
def test_every_level_subset(eng, W, H, Cn):
    assert len(SUBSETS) == 15
    streams = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(2)]
    fix = _fix_mode(eng, streams)
    models = [_models(s, fix, H, W, Cn) for s in streams]
    want = {k: np.stack([m[k] for m in models]) for k in range(4)}
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    for levels in SUBSETS:
        # (_pyramid: the wanted levels' sentinels, and the poisoned buffers of the others untouched)
        st, got, bufs = _pyramid(eng, d_in, stride, sizes, W, H, Cn, levels)
        assert (st == 0).all(), (levels, st)
        assert sorted(got) == list(levels)
        for k in levels:
            _same(got[k], want[k], "%dx%d levels %s: level %d" % (W, H, levels, k))
        # A second run into the same buffers with each wanted level in turn left out (NULL): that level's
        # bytes stay what the first run wrote, the others are written again.
        for drop in levels:
            rest = tuple(k for k in levels if k != drop)
            if not rest:
                continue
            before = bufs[drop][0].clone()
            for k in rest:
                bufs[k][0].fill_(POISON)
            desc = himg_amd.pyramid_desc(*[bufs[k][0] if k in rest else None for k in range(4)])
            d_st = torch.full((2,), -99, dtype=torch.int32, device="cuda")
            eng.decode_pyramid_device(d_in, stride, sizes, 2, W, H, Cn, desc, d_st)
            torch.cuda.synchronize()
            assert (d_st.cpu().numpy() == 0).all()
            assert torch.equal(bufs[drop][0], before), "levels %s without %d: level %d was written" % (levels, drop, drop)
            for k in rest:
                t, nb = bufs[k]
                assert (t[nb:] == POISON).all().item()
                _same(t[:nb].cpu().numpy().reshape(want[k].shape), want[k], "levels %s without %d: level %d" % (levels, drop, k))


def _damage_header(b, r, fix):
    """b with the size header of block row r made to overrun the chunk (test_gpu_regions' damage)."""
    offs = himg_amd.index_host(b, fix)[3]
    d = b.copy()
    hdr = int(offs[r]) - 2
    d[hdr], d[hdr + 1] = 0xFF, 0x7F
    return d


def _damage_tree(b):
    """b with the first bytes of the FRES chunk -- its Huffman tree -- overwritten."""
    off, _ = sm.find_chunks(b)["FRES"]
    d = b.copy()
    d[off:off + 8] = 0xFF
    return d


def test_verdicts_per_frame(eng):
    """Good frames around damaged ones: every frame's status is decode_device's, the good frames are
    exact at all four levels, twice on one engine."""
    W, H, Cn = 264, 40, 4
    good = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(4)]
    fix = _fix_mode(eng, good)
    offs, lens = himg_amd.index_host(good[1], fix)[3:5]
    cut = good[1][:int(offs[1]) + int(lens[1]) // 2].copy()   # cut short inside its second block row
    header = _damage_header(good[2], 3, fix)                      # block row 3's size header overruns the chunk
    tree = _damage_tree(good[1])
    first = good[2].copy()
    first[0] ^= 0x01                                          # no RIFF file
    streams = [good[0], cut, header, good[3], tree, first, good[1]]
    n = len(streams)
    ok = [0, 3, 6]
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    st0, _ = _entry_points(eng, d_in, stride, sizes, W, H, Cn)
    assert all(st0[f] == 0 for f in ok) and all(st0[f] != 0 for f in range(n) if f not in ok), st0
    models = {f: _models(streams[f], fix, H, W, Cn) for f in ok}
    for levels in [(0, 1, 2, 3), (3,), (1, 2)]:   # (level 3 alone: still the full decode's verdict)
        for rnd in range(2):
            st, got, _ = _pyramid(eng, d_in, stride, sizes, W, H, Cn, levels)
            assert np.array_equal(st, st0), (levels, rnd, st, st0)
            for f in ok:
                for k in levels:
                    _same(got[k][f], models[f][k], "levels %s round %d frame %d level %d" % (levels, rnd, f, k))


def test_argument_errors(engine):
    W, H, Cn = 96, 48, 4
    b = _stream("randtile", W, H, Cn, 50, True)
    d_in, stride = _upload([b, b])
    sizes = [len(b)] * 2
    bufs = _buffers(2, W, H, Cn)
    full = [bufs[k][0] for k in range(4)]

    def untouched(d_st):
        torch.cuda.synchronize()
        return all((t == POISON).all().item() for t in full) and (d_st.cpu().numpy() == -99).all()

    cases = [
        ("empty subset", himg_amd.pyramid_desc(), 2, W, H),
        ("NULL out", None, 2, W, H),
        ("width 0", himg_amd.pyramid_desc(*full), 2, 0, H),
        ("height -8", himg_amd.pyramid_desc(*full), 2, W, -8),
        ("batch 0", himg_amd.pyramid_desc(*full), 0, W, H),
        ("level 2 + 4 bytes", himg_amd.pyramid_desc(full[0], full[1], full[2][4:], full[3]), 2, W, H),
    ]
    for what, desc, n, w, h in cases:
        d_st = torch.full((2,), -99, dtype=torch.int32, device="cuda")
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_pyramid_device(d_in, stride, sizes, n, w, h, Cn, desc, d_st)
        assert e.value.code == himg_amd.HIMG_ERR_ARG, what
        assert untouched(d_st), what
    # ... and the same arguments with nothing wrong go through
    st, _, _ = _pyramid(engine, d_in, stride, sizes, W, H, Cn, bufs=bufs)
    assert (st == 0).all()


def test_engine_decode_pyramid(eng):
    W, H, Cn = 100, 37, 3
    s = _stream("randtile", W, H, Cn, 50, True, seed=1)
    fix = _fix_mode(eng, [s])
    models = _models(s, fix, H, W, Cn)
    got = eng.decode_pyramid(s)
    assert sorted(got) == [0, 1, 2, 3]
    for k in range(4):
        _same(got[k], models[k], "decode_pyramid level %d" % k)
    got = eng.decode_pyramid(s, levels=(3, 1))
    assert sorted(got) == [1, 3]
    for k in (1, 3):
        _same(got[k], models[k], "decode_pyramid levels (1, 3): level %d" % k)
    # Nothing stays resident behind it: there is no fetch_last protocol.
    size = C.c_size_t()
    assert himg_amd.lib().himg_hip_fetch_last(eng._ctx, None, 0, C.byref(size)) == himg_amd.HIMG_ERR_ARG and size.value == 0
    # A wanted level whose buffer is too small, or NULL with a capacity: HIMG_ERR_CAPACITY, the geometry set, nothing written.
    outs = {k: np.full(models[k].size, POISON, np.uint8) for k in range(4)}
    for what, k_bad, null in [("too small", 2, False), ("NULL with a capacity", 1, True), ("too small", 0, False)]:
        dst, cap = (C.c_void_p * 4)(), (C.c_size_t * 4)()
        for k in range(4):
            dst[k], cap[k] = outs[k].ctypes.data, outs[k].nbytes
        if null:
            dst[k_bad] = None
        else:
            cap[k_bad] = outs[k_bad].nbytes - 1
        w, h, c = C.c_int(), C.c_int(), C.c_int()
        rc = himg_amd.lib().himg_hip_decode_pyramid_to(eng._ctx, s.ctypes.data, s.nbytes, dst, cap, C.byref(w), C.byref(h), C.byref(c))
        assert rc == himg_amd.HIMG_ERR_CAPACITY, (what, k_bad, rc)
        assert (w.value, h.value, c.value) == (W, H, Cn)
        assert all((outs[k] == POISON).all() for k in range(4))
    # no level wanted
    dst, cap = (C.c_void_p * 4)(), (C.c_size_t * 4)()
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    rc = himg_amd.lib().himg_hip_decode_pyramid_to(eng._ctx, s.ctypes.data, s.nbytes, dst, cap, C.byref(w), C.byref(h), C.byref(c))
    assert rc == himg_amd.HIMG_ERR_ARG
    # a damaged stream: the full decode's verdict and wording
    bad = s.copy()
    bad[0] ^= 0x01
    with pytest.raises(himg_amd.HimgError) as e:
        eng.decode_pyramid(bad)
    assert e.value.code == himg_amd.HIMG_ERR_FORMAT
