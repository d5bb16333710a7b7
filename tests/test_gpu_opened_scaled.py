"""GPU: scaled windows (1/2, 1/4, 1/8) on an opened-streams handle -- scaled_regions_device / scaled_regions --
against the scaled decode's model (tests/scaled_model.py) and the oracle's low-res plane, cropped, byte for
byte; against decode_scaled_regions_device over one stream copy per window and preview_device, status word for
status word: the head is kept (poisoned after open), the counts are shared with the full-resolution entry (the
stage timer's launch counts), independence across calls and scales with the kept frame left clean, every damaged
stream of the corpus, two column strips, the host form, argument errors, a caller's stream, far addresses.
Every test checks the sentinels behind d_out and d_status and that d_packed is byte for byte what it was."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import himg_amd
import damage_model as dm
import opened_scaled_cases as oc
import scaled_model as sm
import stream_region_cases as sc
import test_gpu_preview as tp
from scaled_region_rects import rects
from test_gpu_opened_streams import Opened, _counted_call, _poisoned, _shape_case
from test_gpu_region import _crop
from test_gpu_stream_regions import MAP12, SENT_OUT, SENT_ST, SHAPES, _corpus_windows, _run, _upload

pytestmark = pytest.mark.gpu

ARG = himg_amd.HIMG_ERR_ARG


@pytest.fixture(scope="module", params=[0, 1], ids=["count", "count_w"])
def eng_wave(request):
    e = himg_amd.Engine(0)
    e.set_option("count_wave", request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_own():
    """An engine whose options a test may change as it goes."""
    e = himg_amd.Engine(0)
    yield e
    e.close()


class OpenedS(Opened):
    """test_gpu_opened_streams.Opened with scall(): scaled_regions_device behind sentinels."""

    def scall(self, s, so, org, w, h, **kw):
        n = len(so)
        nb = n * h * w * self.Cn
        d_out = torch.full((nb + 64,), SENT_OUT, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n + 4,), SENT_ST, dtype=torch.int32, device="cuda")
        self.h.scaled_regions_device(s, so, org, w, h, d_out, d_st, **kw)
        torch.cuda.synchronize()
        out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
        assert (out[nb:] == SENT_OUT).all() and (st[n:] == SENT_ST).all()
        return st[:n], out[:nb].reshape(n, h, w, self.Cn)


def _model(stream, s, fix):
    """The picture of a sound stream at scale 2^-s: scaled_model at 1 and 2, the oracle's interleaved low-res
    trace (as test_gpu_preview builds it) at 3."""
    rc, img = sm.expected(stream, s, fix) if s < 3 else tp.expected(stream, fix)
    assert rc == 0
    return img


def _stateless(eng, streams, W, H, Cn, s, so, org, w, h):
    """The stateless answer, window by window: decode_scaled_regions_device over a batch with a stream copied per
    window (s = 1, 2); preview_device over the streams, cropped, with its status words (s = 3)."""
    n = len(so)
    if s == 3:
        st, pv = tp._preview_device(eng, streams, W, H, Cn)
        return st[so], np.stack([_crop(pv[k], (x, y, w, h)) for k, (x, y) in zip(so, org)])
    batch = [streams[k] for k in so]
    d_in, stride = _upload(batch)
    d_out = torch.full((n * h * w * Cn + 16,), SENT_OUT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), SENT_ST, dtype=torch.int32, device="cuda")
    eng.decode_scaled_regions_device(d_in, stride, [len(b) for b in batch], n, W, H, Cn, s, org, w, h, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy()[:n * h * w * Cn].reshape(n, h, w, Cn)


def _four_calls(ow, oh):
    """Test 1's calls: (w, h, origins) x 4 -- 12 x 9, 1 x 1, ow x oh, and the first again."""
    rng = np.random.default_rng(19)
    sizes = [(min(12, ow), min(9, oh)), (1, 1), (ow, oh)]
    calls = [(w, h, sc.origins12(ow, oh, w, h, rng)) for w, h in sizes]
    return calls + [calls[0]]


def _parity_calls(eng, o, streams, models, W, H, Cn, s):
    outs = []
    for w, h, org in _four_calls(*oc.size(W, H, s)):
        st, out = o.scall(s, MAP12, org, w, h)
        st0, out0 = _stateless(eng, streams, W, H, Cn, s, MAP12, org, w, h)
        assert np.array_equal(st, st0) and (st == 0).all(), (s, w, h, st, st0)
        for k in range(12):
            assert np.array_equal(out[k], _crop(models[MAP12[k]], (org[k][0], org[k][1], w, h))), (s, w, h, k)
        assert np.array_equal(out, out0)
        outs.append(out)
    assert np.array_equal(outs[0], outs[3])


# ---- 1. parity ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", oc.SCALES)
@pytest.mark.parametrize("kind,W,H,Cn,q", SHAPES)
def test_parity(eng_wave, kind, W, H, Cn, q, s):
    streams, _, fix = _shape_case(eng_wave, kind, W, H, Cn, q)
    try:
        models = [_model(b, s, fix) for b in streams]
        ow, oh = oc.size(W, H, s)
        assert models[0].shape == (oh, ow, Cn)
        o = OpenedS(eng_wave, streams, W, H, Cn)
        _parity_calls(eng_wave, o, streams, models, W, H, Cn, s)
        # (the ow x oh windows touched every row of both streams; at 1/8 scale no row is touched)
        assert o.h.info()["rows_counted"] == (0 if s == 3 else 2 * ((H + 7) // 8))
        o.done()
    finally:
        eng_wave.set_option("fix_t2", 0)


@pytest.mark.parametrize("s", (1, 2))
def test_every_rectangle_one_per_call(engine, s):
    """Every rectangle of scaled_region_rects on the 50 x 41 x 3 shape -- every x mod S and y mod S, single
    samples, the ragged last tile --, one per call on one handle."""
    kind, W, H, Cn, q = SHAPES[1]
    streams, _, fix = _shape_case(engine, kind, W, H, Cn, q)
    try:
        models = [_model(b, s, fix) for b in streams]
        o = OpenedS(engine, streams, W, H, Cn)
        for i, rect in enumerate(rects(W, H, s)):
            k = i % 2
            st, out = o.scall(s, [k], [rect[:2]], rect[2], rect[3])
            assert st[0] == 0 and np.array_equal(out[0], _crop(models[k], rect)), (s, rect)
        o.done()
    finally:
        engine.set_option("fix_t2", 0)


# ---- 2. the head is kept ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,W,H,Cn,q", SHAPES)
def test_head_is_kept(eng_wave, kind, W, H, Cn, q):
    streams, _, fix = _shape_case(eng_wave, kind, W, H, Cn, q)
    try:
        o = OpenedS(eng_wave, streams, W, H, Cn)
        torch.cuda.synchronize()
        poison = _poisoned(o.d_in, o.stride, streams, fix)
        assert not torch.equal(poison, o.d_in)
        o.d_in.copy_(poison)
        torch.cuda.synchronize()
        for s in oc.SCALES:
            # (the stateless calls, which read the head, get the streams as they were)
            _parity_calls(eng_wave, o, streams, [_model(b, s, fix) for b in streams], W, H, Cn, s)
        o.done(expect=poison)
        # the stages of a scaled call: on a fresh handle, so that the counts run too
        for s in oc.SCALES:
            o = OpenedS(eng_wave, streams, W, H, Cn)
            torch.cuda.synchronize()
            o.d_in.copy_(poison)
            eng_wave.profile(True)
            eng_wave.profile_reset()
            try:
                w, h, org = _four_calls(*oc.size(W, H, s))[0]
                o.scall(s, MAP12, org, w, h)
                names = sorted(eng_wave.profile_read())
            finally:
                eng_wave.profile(False)
                eng_wave.profile_reset()
            if s == 3:
                assert names == ["k_opened_preview_region"], names
                assert not [n for n in names if "count" in n], names
            else:
                assert "k_dec_opened_scaled_region" in names and "k_opened_gate" in names, names
                assert [n for n in names if "count" in n], names
            assert not [n for n in names if "parse" in n or ("lres_" in n and n != "k_opened_preview_region") or "walk" in n
                        or "set_index" in n or "memset" in n], names
            o.done(expect=poison)
    finally:
        eng_wave.set_option("fix_t2", 0)


# ---- 3. the counts are shared across entry points ------------------------------------------------------

def _counted_scall(eng, o, s, so, org, w, h):
    """_counted_call for a scaled call."""
    eng.profile(True)
    eng.profile_reset()
    try:
        st, out = o.scall(s, so, org, w, h)
        prof = eng.profile_read()
    finally:
        eng.profile(False)
        eng.profile_reset()
    return st, out, {k: v[1] for k, v in prof.items() if "count" in k}


@pytest.mark.parametrize("wave", [0, 1])
def test_counts_are_shared_across_entry_points(eng_own, wave):
    eng = eng_own
    streams = [sc.stream(seed=0), sc.stream(seed=1)]
    one = np.array([1], np.int32)
    kernel = "k_stream_count_w" if wave else "k_stream_count"
    try:
        eng.set_option("count_wave", wave)
        o = OpenedS(eng, streams, sc.W, sc.H, sc.C)
        for s, xy, (w, h), rows, launches, total in oc.COUNT_STEPS:
            org = np.array([xy], np.int32)
            if s:
                st, out, cnt = _counted_scall(eng, o, s, one, org, w, h)
                want = _crop(_model(streams[1], s, False), xy + (w, h))
            else:
                st, out, cnt = _counted_call(eng, o, one, org, w, h)
                want = _crop(sc.full(seed=1), xy + (w, h))
            assert cnt == ({kernel: 1} if launches else {}), (s, xy, cnt)
            assert o.h.info()["rows_counted"] == total, (s, xy)
            assert st[0] == 0 and np.array_equal(out[0], want), (s, xy)
        o.done()
        # a fresh handle: the 1/8 level touches no row
        o = OpenedS(eng, streams, sc.W, sc.H, sc.C)
        cols, rows = oc.size(sc.W, sc.H, 3)
        st, out, cnt = _counted_scall(eng, o, 3, np.array([0, 1], np.int32), np.zeros((2, 2), np.int32), cols, rows)
        assert (st == 0).all() and cnt == {} and o.h.info()["rows_counted"] == 0
        o.done()
    finally:
        eng.set_option("count_wave", -1)


# ---- 4. independence, and the kept frame stays clean ----------------------------------------------------

@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("name", ["payload", "header", "cut", "surplus", "head"])
def test_independence_across_calls_and_the_frame_stays_clean(eng_wave, name, s):
    good, bad, clean = sc.independence_cases()[name]
    streams = [bad, clean]
    so, org = oc.windows(s)
    w, h = oc.WIN[s]
    exp = oc.expected(name, s)
    fails = np.array([code != dm.OK for code, _ in exp])
    assert fails.any() and (not fails.all())
    st0, out0 = _stateless(eng_wave, streams, sc.W, sc.H, sc.C, s, so, org, w, h)
    assert np.array_equal(st0 != 0, fails), (name, s, st0)
    # the full-resolution answer the handle must still give afterwards
    so_f, org_f = sc.windows()
    stf, outf = _run(eng_wave, streams, sc.W, sc.H, sc.C, so_f, org_f, *sc.WIN)
    rc, clean_model = sm.expected(good, s)
    assert rc == 0

    def judge(st, out, idx, how):
        assert np.array_equal(st, st0[idx]), (name, s, how, st, st0[idx])
        for j, k in enumerate(idx):
            if not fails[k]:
                assert np.array_equal(out[j], exp[k][1]), (name, s, how, k)
                assert np.array_equal(out[j], out0[k]), (name, s, how, k)
                if so[k] == 0:   # (the damage lies outside the window's rows: the clean picture's samples)
                    assert np.array_equal(out[j], _crop(clean_model, (org[k][0], org[k][1], w, h))), (name, s, how, k)

    every = np.arange(len(so))
    for order, how in [((fails, ~fails), "the failing windows first"), ((~fails, fails), "the passing windows first")]:
        o = OpenedS(eng_wave, streams, sc.W, sc.H, sc.C)
        for part in order:
            idx = every[part]
            judge(*o.scall(s, so[idx], org[idx], w, h), idx, how)
        # the scaled kernel raised its rejected rows into the windows' words, not into the handle's DecFrame
        st, out = o.call(so_f, org_f, *sc.WIN)
        assert np.array_equal(st, stf), (name, s, how, st, stf)
        assert np.array_equal(out[st == 0], outf[st == 0])
        # and the scaled windows again, all in one call, after the full-resolution one
        judge(*o.scall(s, so, org, w, h), every, how + ", then all")
        o.done()


@pytest.mark.parametrize("name", ["payload", "header", "cut", "surplus", "head"])
def test_scale_3_sees_the_head_alone(engine, name):
    """At 1/8 scale damage behind the head fails no window: every window is the crop of the damaged stream's
    preview.  A damaged head gives every window of its stream the word open wrote to d_head_status."""
    good, bad, clean = sc.independence_cases()[name]
    streams = [bad, clean]
    so, org = oc.windows(3)
    w, h = oc.WIN[3]
    d_in, stride = _upload(streams)
    ref = d_in.clone()
    d_hs = torch.full((2 + 4,), SENT_ST, dtype=torch.int32, device="cuda")
    n, nb = len(so), len(so) * h * w * sc.C
    d_out = torch.full((nb + 64,), SENT_OUT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n + 4,), SENT_ST, dtype=torch.int32, device="cuda")
    with engine.open_streams_device(d_in, stride, [len(b) for b in streams], 2, sc.W, sc.H, sc.C, d_head_status=d_hs) as o:
        o.scaled_regions_device(3, so, org, w, h, d_out, d_st)
        torch.cuda.synchronize()
        assert o.info()["rows_counted"] == 0
    hs, st, out = d_hs.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy()
    assert (out[nb:] == SENT_OUT).all() and (st[n:] == SENT_ST).all() and (hs[2:] == SENT_ST).all()
    assert torch.equal(d_in, ref)
    assert np.array_equal(st[:n], hs[so]) and hs[1] == 0
    px = out[:nb].reshape(n, h, w, sc.C)
    if name == "head":
        assert hs[0] != 0 and (px[so == 0] == SENT_OUT).all()   # (no pixel of a window with a verdict is written)
        streams = [clean, clean]
    else:
        assert hs[0] == 0
    st_p, pv = tp._preview_device(engine, streams, sc.W, sc.H, sc.C)
    assert (st_p == 0).all()
    for k in range(n):
        if st[k] == 0:
            assert np.array_equal(px[k], _crop(pv[so[k]], (org[k][0], org[k][1], w, h))), (name, k)


# ---- 5. the corpus -----------------------------------------------------------------------------------

@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("cls", "PHC")
@pytest.mark.parametrize("name", [b.name for b in dm.BASES])
def test_equals_scaled_regions_on_the_corpus(engine, name, cls, s):
    """Every damaged stream of the corpus's class: a handle over [good, bad], the class's windows scaled to the
    level (x // F, y // F, size max(1, w // F) x max(1, h // F)) in two calls, against
    decode_scaled_regions_device over a batch with a stream copied per window."""
    b, m = dm.BASE[name], dm.good_model(name)
    ss = dm.streams(name, cls)
    if not ss:
        return   # (a frame of one block row has no size header to damage)
    engine.set_option("fix_t2", int(b.fix))
    F = 1 << s
    w, h = max(1, b.win[0] // F), max(1, b.win[1] // F)
    so, org = _corpus_windows(name, cls)
    org = (org >> s).astype(np.int32)
    ow, oh = himg_amd.scaled_size(b.W, b.H, s)
    assert (org[:, 0] + w <= ow).all() and (org[:, 1] + h <= oh).all()
    n, wb = len(so), h * w * b.C
    half = n // 32 * 16 + 16   # (a little past the middle, and the second call's slots 16-byte aligned)
    assert 0 < half < n
    d_so = torch.from_numpy(so.astype(np.int64)).cuda()
    tail = (n * wb + 64 + 255) // 256 * 256
    d_out = torch.empty((2, tail), dtype=torch.uint8, device="cuda")
    d_st = torch.empty((2, n + 4), dtype=torch.int32, device="cuda")
    try:
        n_fail = n_ok = 0
        for i, bad in enumerate(ss):
            streams = [m.packed, bad.bad]
            d_in, stride = _upload(streams)
            ref = d_in.clone()
            sizes = [len(x) for x in streams]
            d_out.fill_(SENT_OUT)
            d_st.fill_(SENT_ST)
            with engine.open_streams_device(d_in, stride, sizes, 2, b.W, b.H, b.C) as o:
                # (the second call's slots lie behind the first's: window k at k * wb, its word at k)
                o.scaled_regions_device(s, so[:half], org[:half], w, h, d_out[0], d_st[0])
                o.scaled_regions_device(s, so[half:], org[half:], w, h, d_out[0][half * wb:], d_st[0][half:])
                engine.decode_scaled_regions_device(d_in[d_so].contiguous(), stride, [sizes[k] for k in so], n, b.W, b.H, b.C,
                                                    s, org, w, h, d_out[1], d_st[1])
                torch.cuda.synchronize()
            st = d_st.cpu().numpy()
            assert bool((d_out[:, n * wb:] == SENT_OUT).all()) and (st[:, n:] == SENT_ST).all()
            assert torch.equal(d_in, ref)
            assert np.array_equal(st[0, :n], st[1, :n]), (name, cls, s, i, np.flatnonzero(st[0, :n] != st[1, :n])[:8])
            ok = st[0, :n] == 0
            px = d_out[:, :n * wb].view(2, n, wb)
            d_ok = torch.from_numpy(ok).cuda()
            assert torch.equal(px[0][d_ok], px[1][d_ok]), (name, cls, s, i)
            assert ok[so == 0].all(), (name, cls, s, i)
            n_fail += int((~ok[so == 1]).sum())
            n_ok += int(ok[so == 1].sum())
        assert n_fail > 0 and (n_ok > 0 or b.H <= 8), (n_fail, n_ok)
    finally:
        engine.set_option("fix_t2", 0)


# ---- 6. two column strips ------------------------------------------------------------------------------

def _strip_tiles(Cn, s):
    """scaled_strip_tiles (kernels_dec.hip), as test_gpu_scaled_region.py restates it."""
    nseg = (16 if s == 1 else 4) * Cn
    return ((160 * 1024 - 1024 - 27600) // nseg & ~3) - 8


def _strip_case(engine, kind, W, H, w, h, xs):
    s, Cn = 1, 4
    b = sc.stream(kind, W, H, Cn)
    fix = sc.needs_fix(kind, W, H, Cn)
    engine.set_option("fix_t2", int(fix))
    try:
        want = _model(b, s, fix)
        ow, oh = himg_amd.scaled_size(W, H, s)
        org = np.array([(xs[0], 0), (xs[1], 3), (ow - w, oh - h), (xs[1] + 2, 1)], np.int32)
        o = OpenedS(engine, [b], W, H, Cn)
        for part in (slice(0, 2), slice(2, 4)):
            st, out = o.scall(s, np.zeros(2, np.int32), org[part], w, h)
            assert (st == 0).all(), st
            for k, (x, y) in enumerate(org[part]):
                assert np.array_equal(out[k], _crop(want, (x, y, w, h))), (part, k)
        o.done()
    finally:
        engine.set_option("fix_t2", 0)


def test_wide_windows_of_an_8192_wide_stream(engine):
    """1/2-scale windows 2081 samples wide of an 8192 x 64 x 4 stream: from 0, from an odd origin, at the right
    edge; two windows per call, two calls.  (521 tiles: one strip -- at this scale a strip holds 2104 tiles of
    RGBA, more than any 8192-wide picture has; the next test takes two.)"""
    _strip_case(engine, "randtile", 8192, 64, 2081, 10, (0, 1001))


def test_two_column_strips(engine):
    """A stream wider than one strip of the scaled kernel's LDS layout holds (the shape of
    test_gpu_scaled_region.test_window_of_two_strips): windows of more tiles than scaled_strip_tiles, from 0, from
    an odd origin and at the right edge."""
    tiles = _strip_tiles(4, 1)
    W, H = 8 * (tiles + 37) + 3, 21
    w = 4 * tiles + 9
    assert (1 + w + 3) // 4 > tiles and himg_amd.scaled_size(W, H, 1)[0] >= w + 7
    _strip_case(engine, "rand", W, H, w, 7, (0, 5))


# ---- 7. the host form ------------------------------------------------------------------------------------

def test_host_form(engine):
    cases = sc.independence_cases()
    n_fail = 0
    for what, b in [("clean", sc.stream()), ("payload", cases["payload"][1]), ("header", cases["header"][1])]:
        if what == "header":
            with pytest.raises(himg_amd.HimgError):
                himg_amd.index_host(b)   # (the host cannot index it: the device walk runs)
        with engine.open_stream(b) as o:
            for s in (1, 2):
                so, org = oc.windows(s)
                org0 = np.ascontiguousarray(org[so == 0])
                ow, oh = himg_amd.scaled_size(sc.W, sc.H, s)
                for w, h, oo in [oc.WIN[s] + (org0,), oc.WIN[s] + (org0[::-1],), (ow, oh, np.array([(0, 0)], np.int32))]:
                    got, st = o.scaled_regions(s, oo, w, h)
                    assert got.shape == (len(oo), h, w, sc.C)
                    for k, (x, y) in enumerate(oo):
                        try:
                            want, code = engine.decode_scaled_region(b, s, int(x), int(y), w, h), 0
                        except himg_amd.HimgError as e:
                            want, code = None, e.code
                        assert st[k] == code, (what, s, w, h, k, st[k], code)
                        if code == 0:
                            assert np.array_equal(got[k], want), (what, s, w, h, k)
                    n_fail += int((st != 0).sum())
            assert o.info()["rows_counted"] == sc.ROWS
            if what == "clean":   # the 1/8 level: the crops of preview()
                so, org = oc.windows(3)
                got, st = o.scaled_regions(3, org, *oc.WIN[3])
                pv = engine.preview(b)
                assert (st == 0).all() and o.info()["rows_counted"] == sc.ROWS
                for k, (x, y) in enumerate(org):
                    assert np.array_equal(got[k], _crop(pv, (x, y) + oc.WIN[3])), k
    assert n_fail > 0
    # a short or missing dst: HIMG_ERR_CAPACITY, the geometry set, dst and statuses untouched, nothing counted
    L, b = himg_amd.lib(), sc.stream()
    for s in oc.SCALES:
        so, org = oc.windows(s)
        org0 = np.ascontiguousarray(org[so == 0])
        n, (w, h) = len(org0), oc.WIN[s]
        want = np.stack([_crop(_model(b, s, False), (x, y, w, h)) for x, y in org0])
        with engine.open_stream(b) as o:
            wo, ho, co = C.c_int(), C.c_int(), C.c_int()
            for dst_len in (n * h * w * sc.C - 1, 16, 0):
                dst = np.full(max(dst_len, 1) + 32, 0x77, np.uint8)
                st = np.full(n, 7, np.int32)
                rc = L.himg_hip_opened_scaled_regions_to(engine._ctx, o._h, s, n, None, org0.ctypes.data, w, h,
                                                         dst.ctypes.data if dst_len else None, dst_len, st.ctypes.data,
                                                         C.byref(wo), C.byref(ho), C.byref(co))
                assert rc == himg_amd.HIMG_ERR_CAPACITY and (wo.value, ho.value, co.value) == (w, h, sc.C)
                assert (dst == 0x77).all() and (st == 7).all() and o.info()["rows_counted"] == 0
            # and with room: the bytes, and nothing behind them
            dst = np.full(n * h * w * sc.C + 32, 0x77, np.uint8)
            st = np.full(n + 2, 7, np.int32)
            rc = L.himg_hip_opened_scaled_regions_to(engine._ctx, o._h, s, n, None, org0.ctypes.data, w, h, dst.ctypes.data,
                                                     n * h * w * sc.C, st.ctypes.data, C.byref(wo), C.byref(ho), C.byref(co))
            assert rc == 0 and (dst[-32:] == 0x77).all() and (st[:n] == 0).all() and (st[n:] == 7).all()
            assert np.array_equal(dst[:-32].reshape(want.shape), want)
            ow, oh = oc.size(sc.W, sc.H, s)
            with pytest.raises(himg_amd.HimgError) as e:
                o.scaled_regions(s, [(0, 0), (ow - w + 1, 0)], w, h)
            assert e.value.code == ARG
            with pytest.raises(himg_amd.HimgError) as e:
                o.scaled_regions(s, [(0, 0)], w, h, stream_of=[1])
            assert e.value.code == ARG
            with pytest.raises(himg_amd.HimgError) as e:
                o.scaled_regions(4, [(0, 0)], 1, 1)
            assert e.value.code == ARG


# ---- 8. arguments -----------------------------------------------------------------------------------

def test_argument_errors(engine):
    b = sc.stream()
    o = OpenedS(engine, [b, b], sc.W, sc.H, sc.C)
    L = himg_amd.lib()
    w, h = oc.WIN[1]
    ok_so, ok_org = np.array([0, 1], np.int32), np.array([(0, 0), (5, 5)], np.int32)
    d_out = torch.full((4 * sc.W * sc.H * sc.C + 16,), SENT_OUT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((70000,), SENT_ST, dtype=torch.int32, device="cuda")

    def untouched(what):
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENT_OUT).all() and (d_st.cpu().numpy() == SENT_ST).all(), what
        assert o.h.info()["rows_counted"] == 0, what

    def raw(ctx, handle, s=1, so=ok_so, org=ok_org, n=2, ww=w, hh=h, out=d_out, st=d_st):
        return L.himg_hip_opened_scaled_regions_device(ctx, handle, s, so.ctypes.data if so is not None else None,
                                                       org.ctypes.data if org is not None else None, n, ww, hh,
                                                       out.data_ptr() if out is not None else None,
                                                       st.data_ptr() if st is not None else None, None)

    def refused(s, so, org, ww, hh):
        with pytest.raises(himg_amd.HimgError) as e:
            o.h.scaled_regions_device(s, so, org, ww, hh, d_out, d_st)
        assert e.value.code == ARG, (s, list(so)[:4], list(org)[:4], ww, hh)
        untouched((s, list(so)[:4], list(org)[:4], ww, hh))

    other = himg_amd.Engine(0)
    try:
        assert raw(engine._ctx, None) == ARG                 # a NULL handle
        assert raw(None, o.h._h) == ARG                      # no context
        assert raw(other._ctx, o.h._h) == ARG                # another context's handle
        with pytest.raises(himg_amd.HimgError) as e:
            o.h.scaled_regions_device(1, ok_so, ok_org, w, h, d_out, d_st, engine=other)
        assert e.value.code == ARG
        untouched("handle and context")
        for s in (0, 4, -1):
            refused(s, ok_so, ok_org, 1, 1)
        for s in oc.SCALES:
            ow, oh = oc.size(sc.W, sc.H, s)
            ww, hh = oc.WIN[s]
            # inside W x H, outside ow x oh
            refused(s, ok_so, [(0, 0), (ow - ww + 1, 0)], ww, hh)
            refused(s, ok_so, [(0, oh - hh + 1), (0, 0)], ww, hh)
            refused(s, ok_so, [(0, 0), (0, 0)], ow + 1, 1)
            refused(s, ok_so, [(0, 0), (0, 0)], 1, oh + 1)
            refused(s, ok_so, [(0, 0), (-1, 0)], ww, hh)
            refused(s, ok_so, [(0, -1), (0, 0)], ww, hh)
            refused(s, ok_so, ok_org, 0, hh)
            refused(s, ok_so, ok_org, ww, 0)
            refused(s, [0, 2], ok_org, ww, hh)
            refused(s, [-1, 0], ok_org, ww, hh)
            refused(s, [], [], ww, hh)
            refused(s, [0] * 65536, [(0, 0)] * 65536, 1, 1)
            for kw in [dict(so=None), dict(org=None), dict(out=None), dict(st=None), dict(n=0), dict(n=-1)]:
                assert raw(engine._ctx, o.h._h, s=s, ww=ww, hh=hh, **kw) == ARG, (s, kw)
            untouched("NULLs")
        # the handle still works at every scale, and a closed handle is refused
        for s in oc.SCALES:
            st, out = o.scall(s, ok_so, ok_org, *oc.WIN[s])
            assert (st == 0).all()
            for k in range(2):
                assert np.array_equal(out[k], _crop(_model(b, s, False), tuple(ok_org[k]) + oc.WIN[s])), (s, k)
        touched = {(k, r) for s in (1, 2) for k in range(2) for r in range(*oc.rows_of(s, int(ok_org[k][1]), oc.WIN[s][1]))}
        assert o.h.info()["rows_counted"] == len(touched)
        stale = C.c_void_p(o.h._h.value)
        o.done()
        d_out.fill_(SENT_OUT)
        d_st.fill_(SENT_ST)
        for s in oc.SCALES:
            assert raw(engine._ctx, stale, s=s) == ARG
            with pytest.raises(himg_amd.HimgError) as e:
                o.h.scaled_regions_device(s, ok_so, ok_org, 1, 1, d_out, d_st)
            assert e.value.code == ARG
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENT_OUT).all() and (d_st.cpu().numpy() == SENT_ST).all()
    finally:
        other.close()


# ---- 9. a caller's stream ------------------------------------------------------------------------------

def test_callers_stream_gated(engine):
    """Open, one full-resolution call and one scaled call at each scale on the caller's non-blocking stream behind
    tests/stream_gate.py's gate, no host wait between them; a decoy decode on the same context goes in front (six
    calls: fewer than the context's eight pinned slots, so none waits for a copy behind the gate)."""
    import stream_gate as sg
    streams = [sc.stream(seed=0), sc.stream(seed=1)]
    models = {s: [_model(b, s, False) for b in streams] for s in oc.SCALES}
    models[0] = [sc.full(seed=0), sc.full(seed=1)]
    calls = [(0, sc.WIN) + sc.windows()] + [(s, oc.WIN[s]) + oc.windows(s) for s in oc.SCALES]
    stride = (max(len(b) for b in streams) + 3 + 255) // 256 * 256
    real, decoy = np.zeros((2, stride), np.uint8), np.zeros((2, stride), np.uint8)
    for i, b in enumerate(streams):
        real[i, :len(b)] = b
        decoy[1 - i, :len(b)] = b
    sizes = [len(b) for b in streams]
    w0, h0 = sc.WIN
    d_org = sc.origins12(sc.W, sc.H, w0, h0, np.random.default_rng(23))
    outs = {"decoy_pix": (12 * h0 * w0 * sc.C, SENT_OUT), "decoy_st": (4 * 12, 0x9D)}
    for j, (s, (w, h), so, _) in enumerate(calls):
        outs["pix%d" % j] = (len(so) * h * w * sc.C, SENT_OUT)
        outs["st%d" % j] = (4 * len(so), 0x9D)
    gate = sg.Gate(log=lambda *a: None)
    S = gate.self_check()
    assert S is not None, "inconclusive: no torch stream ran independently of the null stream"
    buf = sg.Buffers(torch, real, decoy, outs)
    handles = []

    def issue():
        engine.decode_stream_regions_device(buf.d_in, stride, sizes, 2, sc.W, sc.H, sc.C, MAP12, d_org, w0, h0,
                                            buf.outs["decoy_pix"][0], buf.outs["decoy_st"][0], stream=S.cuda_stream)
        o = engine.open_streams_device(buf.d_in, stride, sizes, 2, sc.W, sc.H, sc.C, stream=S.cuda_stream)
        handles.append(o)
        for j, (s, (w, h), so, org) in enumerate(calls):
            pix, st = buf.outs["pix%d" % j][0], buf.outs["st%d" % j][0]
            if s:
                o.scaled_regions_device(s, so, org, w, h, pix, st, stream=S.cuda_stream)
            else:
                o.regions_device(so, org, w, h, pix, st, stream=S.cuda_stream)

    def check(what):
        for j, (s, (w, h), so, org) in enumerate(calls):
            st = buf.result("st%d" % j).view(np.int32)
            assert (st == 0).all(), (what, j, st)
            px = buf.result("pix%d" % j).reshape(len(so), h, w, sc.C)
            for k in range(len(so)):
                assert np.array_equal(px[k], _crop(models[s][so[k]], (org[k][0], org[k][1], w, h))), (what, j, k)
        assert (buf.result("decoy_st").view(np.int32) == 0).all(), what

    def close_all():
        while handles:
            handles.pop().close()

    # warm-up on S, ungated: the first pass reserves (and may wait for the device), the second is timed on the host
    buf.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        buf.queue_input()
    issue()
    S.synchronize()
    close_all()
    host_s = sg.timed_call(issue)
    with torch.cuda.stream(S):
        buf.queue_collect()
    S.synchronize()
    check("warm-up")
    close_all()
    # gated: from here to the wait no device-wide synchronise, no .cpu(), nothing on the default stream
    buf.reset()
    torch.cuda.synchronize()
    opened = gate.shut(S, sg.gate_ms(host_s))
    with torch.cuda.stream(S):
        buf.queue_input()
    issue()
    returned_while_shut = not opened.query()
    with torch.cuda.stream(S):
        done = torch.cuda.Event()
        buf.queue_collect()
        done.record(S)
    done.synchronize()
    assert returned_while_shut, "the calls waited for the device (or the host was slower than the gate is long)"
    check("gated")
    close_all()


# ---- 10. far addresses -----------------------------------------------------------------------------------

def test_far_addresses():
    """Five streams at an in_stride of 2^30: stream 4 starts at 2^32, stream 3 beyond 2^31.  Stream f holds picture
    f % 3, so an offset that wraps lands on another valid stream and shows as wrong samples.  Scaled windows of
    streams 3 and 4 at 1/2 and 1/4 scale, each scale's second call on rows the first has not counted.  Need:
    4 GiB + 1 MiB for the input and 1 GiB of allowance; skips with less free device memory."""
    GIB = 1 << 30
    n_bytes = 4 * GIB + (1 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < n_bytes + GIB:
        pytest.skip("needs %d bytes of device memory, %d are free" % (n_bytes + GIB, free))
    eng = himg_amd.Engine(0)
    try:
        streams = [sc.stream(seed=f % 3) for f in range(5)]
        far = torch.full((n_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        for f, b in enumerate(streams):
            far[f * GIB:f * GIB + len(b)] = torch.from_numpy(b.copy()).cuda()
            far[f * GIB + len(b):f * GIB + len(b) + 64] = 0   # (the bit readers' look-ahead: as _upload leaves it)

        def digest():
            torch.cuda.synchronize()
            return [int(far[a:a + (256 << 20)].view(torch.int64).sum().item()) for a in range(0, 4 * GIB, 256 << 20)] + \
                   [far[f * GIB:f * GIB + len(b)].clone() for f, b in enumerate(streams)]

        before = digest()
        d_hs = torch.full((5,), SENT_ST, dtype=torch.int32, device="cuda")
        with eng.open_streams_device(far, GIB, [len(b) for b in streams], 5, sc.W, sc.H, sc.C, d_head_status=d_hs) as o:
            for s in (1, 2, 3):
                models = [_model(streams[f], s, False) for f in range(3)]
                w, h = oc.WIN[s]
                org = oc.windows(s)[1]
                calls = [(np.array([3, 4, 3, 0], np.int32), org[[0, 2, 9, 4]]), (np.array([4, 3, 4, 4], np.int32), org[[8, 6, 1, 5]])]
                for so, og in calls:
                    n = len(so)
                    nb = n * h * w * sc.C
                    d_out = torch.full((nb + 64,), SENT_OUT, dtype=torch.uint8, device="cuda")
                    d_st = torch.full((n + 4,), SENT_ST, dtype=torch.int32, device="cuda")
                    o.scaled_regions_device(s, so, og, w, h, d_out, d_st)
                    torch.cuda.synchronize()
                    out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
                    assert (out[nb:] == SENT_OUT).all() and (st[n:] == SENT_ST).all() and (st[:n] == 0).all(), (s, st)
                    px = out[:nb].reshape(n, h, w, sc.C)
                    for k in range(n):
                        assert np.array_equal(px[k], _crop(models[so[k] % 3], (og[k][0], og[k][1], w, h))), (s, so[k], og[k])
            assert (d_hs.cpu().numpy() == 0).all()
        after = digest()
        assert before[:16] == after[:16] and all(torch.equal(a, b) for a, b in zip(before[16:], after[16:]))
        del far
    finally:
        eng.close()
        gc.collect()
        torch.cuda.empty_cache()
