"""GPU: the opened-streams handle -- open_streams_device / open_stream, then windows in many calls -- against
the oracle's crops and, status word for status word, against decode_stream_regions_device of the same streams,
map, origins and window size: the head is kept (poisoned after open), the counts are kept (the stage timer's
launch counts), independence within and across calls, every damaged stream of the corpus, two column strips,
the host form, argument errors, a caller's stream, far addresses.  Every test checks the sentinels behind d_out
and d_status and that d_packed is byte for byte what it was."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import himg_amd
import damage_model as dm
import stream_region_cases as sc
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


class Opened:
    """Streams on the device with a handle over them; call(): regions_device behind sentinels; done(): the
    input is byte for byte what it was (or what `expect` says), and the handle is closed."""

    def __init__(self, eng, streams, W, H, Cn):
        self.eng, self.Cn = eng, Cn
        self.d_in, self.stride = _upload(streams)
        self.ref = self.d_in.clone()
        self.sizes = [len(s) for s in streams]
        self.h = eng.open_streams_device(self.d_in, self.stride, self.sizes, len(streams), W, H, Cn)

    def call(self, so, org, w, h, **kw):
        n = len(so)
        nb = n * h * w * self.Cn
        d_out = torch.full((nb + 64,), SENT_OUT, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n + 4,), SENT_ST, dtype=torch.int32, device="cuda")
        self.h.regions_device(so, org, w, h, d_out, d_st, **kw)
        torch.cuda.synchronize()
        out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
        assert (out[nb:] == SENT_OUT).all() and (st[n:] == SENT_ST).all()
        return st[:n], out[:nb].reshape(n, h, w, self.Cn)

    def done(self, expect=None):
        torch.cuda.synchronize()
        assert torch.equal(self.d_in, self.ref if expect is None else expect)
        self.h.close()


def _four_calls(W, H):
    """Test 1's calls: (w, h, origins) x 4 -- 24 x 17, 1 x 1, W x H, and the first again."""
    rng = np.random.default_rng(17)
    sizes = [(min(24, W), min(17, H)), (1, 1), (W, H)]
    calls = [(w, h, sc.origins12(W, H, w, h, rng)) for w, h in sizes]
    return calls + [calls[0]]


def _parity_calls(eng, o, streams, fulls, W, H, Cn, stateless_streams=None):
    """Every call of _four_calls on handle o: the oracle's crops, decode_stream_regions_device's status words,
    and the repeat of the first call byte for byte."""
    outs = []
    for w, h, org in _four_calls(W, H):
        st, out = o.call(MAP12, org, w, h)
        st0, out0 = _run(eng, stateless_streams or streams, W, H, Cn, MAP12, org, w, h)
        assert np.array_equal(st, st0) and (st == 0).all(), (w, h, st, st0)
        for k in range(12):
            assert np.array_equal(out[k], _crop(fulls[MAP12[k]], (org[k][0], org[k][1], w, h))), (w, h, k)
        assert np.array_equal(out, out0)
        outs.append(out)
    assert np.array_equal(outs[0], outs[3])


def _shape_case(eng, kind, W, H, Cn, q):
    streams = [sc.stream(kind, W, H, Cn, q, seed) for seed in (0, 1)]
    fulls = [sc.full(kind, W, H, Cn, q, seed) for seed in (0, 1)]
    fix = sc.needs_fix(kind, W, H, Cn, q, 0)
    assert fix == sc.needs_fix(kind, W, H, Cn, q, 1)
    eng.set_option("fix_t2", int(fix))
    return streams, fulls, fix


# ---- 1. parity ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,W,H,Cn,q", SHAPES)
def test_parity(eng_wave, kind, W, H, Cn, q):
    streams, fulls, _ = _shape_case(eng_wave, kind, W, H, Cn, q)
    try:
        o = Opened(eng_wave, streams, W, H, Cn)
        info = o.h.info()
        assert (info["n_streams"], info["width"], info["height"], info["channels"]) == (2, W, H, Cn)
        assert info["device_bytes"] == himg_amd.opened_bytes(W, H, Cn, 2) and info["rows_counted"] == 0
        _parity_calls(eng_wave, o, streams, fulls, W, H, Cn)
        assert o.h.info()["rows_counted"] == 2 * ((H + 7) // 8)   # (the W x H windows touched every row of both)
        o.done()
    finally:
        eng_wave.set_option("fix_t2", 0)


def test_head_status_and_context_manager(engine):
    """d_head_status: 0 for a sound stream, the head verdict for head_damaged; the handle as a context manager."""
    good, bad, clean = sc.independence_cases()["head"]
    d_in, stride = _upload([bad, clean])
    ref = d_in.clone()
    d_hs = torch.full((2 + 4,), SENT_ST, dtype=torch.int32, device="cuda")
    with engine.open_streams_device(d_in, stride, [len(bad), len(clean)], 2, sc.W, sc.H, sc.C, d_head_status=d_hs) as h:
        torch.cuda.synchronize()
        hs = d_hs.cpu().numpy()
        assert hs[0] != 0 and hs[1] == 0 and (hs[2:] == SENT_ST).all()
        assert h.info()["n_streams"] == 2
    with pytest.raises(himg_amd.HimgError):
        h.info()
    assert torch.equal(d_in, ref)


# ---- 2. the head is kept ------------------------------------------------------------------------------

def _poisoned(d_in, stride, streams, fix):
    """d_in with [0, head_bytes) and every size header of every stream overwritten with 0xA5."""
    buf = d_in.cpu().numpy().reshape(len(streams), stride).copy()
    for i, s in enumerate(streams):
        offs, lens = himg_amd.index_host(s, fix_t2=fix)[3:5]
        buf[i, :int(offs[0])] = 0xA5
        for r in range(1, len(offs)):
            a, e = int(offs[r - 1]) + int(lens[r - 1]), int(offs[r])
            assert 2 <= e - a <= 4
            buf[i, a:e] = 0xA5
    return torch.from_numpy(buf).cuda()


@pytest.mark.parametrize("kind,W,H,Cn,q", SHAPES)
def test_head_is_kept(eng_wave, kind, W, H, Cn, q):
    streams, fulls, fix = _shape_case(eng_wave, kind, W, H, Cn, q)
    try:
        o = Opened(eng_wave, streams, W, H, Cn)
        torch.cuda.synchronize()
        poison = _poisoned(o.d_in, o.stride, streams, fix)
        assert not torch.equal(poison, o.d_in)
        o.d_in.copy_(poison)
        torch.cuda.synchronize()
        # (the stateless call, which reads the head, gets the streams as they were)
        _parity_calls(eng_wave, o, streams, fulls, W, H, Cn)
        # the stages of a call on the handle
        eng_wave.profile(True)
        eng_wave.profile_reset()
        try:
            w, h, org = _four_calls(W, H)[0]
            o.call(MAP12, org, w, h)
            names = sorted(eng_wave.profile_read())
        finally:
            eng_wave.profile(False)
            eng_wave.profile_reset()
        assert "k_dec_stream_region" in names and "k_opened_gate" in names, names
        assert not [n for n in names if "parse" in n or "lres" in n or "walk" in n or "set_index" in n or "memset" in n], names
        o.done(expect=poison)
    finally:
        eng_wave.set_option("fix_t2", 0)


# ---- 3. the counts are kept ---------------------------------------------------------------------------

def _counted_call(eng, o, so, org, w, h):
    """(statuses, pixels, launches of a count kernel by name) of one call under the stage timer."""
    eng.profile(True)
    eng.profile_reset()
    try:
        st, out = o.call(so, org, w, h)
        prof = eng.profile_read()
    finally:
        eng.profile(False)
        eng.profile_reset()
    return st, out, {k: v[1] for k, v in prof.items() if "count" in k}


def test_counts_are_kept(eng_own):
    eng = eng_own
    streams, fulls = [sc.stream(seed=0), sc.stream(seed=1)], [sc.full(seed=0), sc.full(seed=1)]
    so = np.array([1, 0, 1], np.int32)

    def check(st, out, org, w, h):
        st0, out0 = _run(eng, streams, sc.W, sc.H, sc.C, so, org, w, h)
        assert (st == 0).all() and np.array_equal(st, st0) and np.array_equal(out, out0)
        for k in range(len(so)):
            assert np.array_equal(out[k], _crop(fulls[so[k]], (org[k][0], org[k][1], w, h))), k

    try:
        eng.set_option("count_wave", 0)
        o = Opened(eng, streams, sc.W, sc.H, sc.C)
        one = np.array([1], np.int32)
        # rows [2, 5) of stream 1: y = 20, h = 17
        org_a = np.array([(33, 20)], np.int32)
        st, out, cnt = _counted_call(eng, o, one, org_a, 24, 17)
        assert cnt == {"k_stream_count": 1}, cnt
        assert o.h.info()["rows_counted"] == 3 and (st == 0).all()
        first = out.copy()
        st, out, cnt = _counted_call(eng, o, one, org_a, 24, 17)
        assert cnt == {}, cnt
        assert o.h.info()["rows_counted"] == 3 and np.array_equal(out, first)
        # rows [3, 7) of the same stream, counted by the other form: rows 5 and 6 are new
        eng.set_option("count_wave", 1)
        st, out, cnt = _counted_call(eng, o, one, np.array([(7, 24)], np.int32), 40, 30)
        assert cnt == {"k_stream_count_w": 1}, cnt
        assert o.h.info()["rows_counted"] == 5 and (st == 0).all()
        assert np.array_equal(out[0], _crop(fulls[1], (7, 24, 40, 30)))
        # windows over rows [2, 7) of stream 1 read records of both forms; stream 0's rows are new
        eng.set_option("count_wave", 0)
        org = np.array([(0, 16), (50, 16), (56, 17)], np.int32)
        st, out, cnt = _counted_call(eng, o, so, org, 40, 39)
        assert cnt == {"k_stream_count": 1} and o.h.info()["rows_counted"] == 10
        check(st, out, org, 40, 39)
        st, out, cnt = _counted_call(eng, o, so, org, 40, 39)
        assert cnt == {} and o.h.info()["rows_counted"] == 10
        check(st, out, org, 40, 39)
        o.done()
    finally:
        eng.set_option("count_wave", -1)


# ---- 4. independence within and across calls -----------------------------------------------------------

@pytest.mark.parametrize("name", ["payload", "header", "cut", "surplus", "head"])
def test_independence_within_and_across_calls(eng_wave, name):
    good, bad, clean = sc.independence_cases()[name]
    so, org = sc.windows()
    exp = sc.expected(name)
    fails = np.array([code != dm.OK for code, _ in exp])
    assert fails.any() and not fails.all()
    streams = [bad, clean]
    st0, out0 = _run(eng_wave, streams, sc.W, sc.H, sc.C, so, org, *sc.WIN)
    assert np.array_equal(st0 != 0, fails)

    def judge(st, out, idx, how):
        assert np.array_equal(st, st0[idx]), (name, how, st, st0[idx])
        for j, k in enumerate(idx):
            if not fails[k]:
                assert np.array_equal(out[j], exp[k][1]), (name, how, k)

    every = np.arange(len(so))
    o = Opened(eng_wave, streams, sc.W, sc.H, sc.C)
    judge(*o.call(so, org, *sc.WIN), every, "one call")
    o.done()
    for order, how in [((fails, ~fails), "the failing windows first"), ((~fails, fails), "the passing windows first")]:
        o = Opened(eng_wave, streams, sc.W, sc.H, sc.C)
        for part in order:
            idx = every[part]
            judge(*o.call(so[idx], org[idx], *sc.WIN), idx, how)
        o.done()


# ---- 5. the corpus -----------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", "PHC")
@pytest.mark.parametrize("name", [b.name for b in dm.BASES])
def test_equals_stream_regions_on_the_corpus(engine, name, cls):
    """Every damaged stream of the corpus's class: a handle over [good, bad], the class's windows in two calls,
    against decode_stream_regions_device in one."""
    b, m = dm.BASE[name], dm.good_model(name)
    ss = dm.streams(name, cls)
    if not ss:
        return   # (a frame of one block row has no size header to damage)
    engine.set_option("fix_t2", int(b.fix))
    w, h = b.win
    so, org = _corpus_windows(name, cls)
    n, wb = len(so), h * w * b.C
    half = n // 32 * 16 + 16   # (a little past the middle, and the second call's slots 16-byte aligned)
    assert 0 < half < n
    tail = (n * wb + 64 + 255) // 256 * 256
    d_out = torch.empty((2, tail), dtype=torch.uint8, device="cuda")
    d_st = torch.empty((2, n + 4), dtype=torch.int32, device="cuda")
    try:
        n_fail = n_ok = 0
        for i, s in enumerate(ss):
            streams = [m.packed, s.bad]
            d_in, stride = _upload(streams)
            ref = d_in.clone()
            sizes = [len(x) for x in streams]
            d_out.fill_(SENT_OUT)
            d_st.fill_(SENT_ST)
            with engine.open_streams_device(d_in, stride, sizes, 2, b.W, b.H, b.C) as o:
                # (the second call's slots lie behind the first's: window k at k * wb, its word at k)
                o.regions_device(so[:half], org[:half], w, h, d_out[0], d_st[0])
                o.regions_device(so[half:], org[half:], w, h, d_out[0][half * wb:], d_st[0][half:])
                engine.decode_stream_regions_device(d_in, stride, sizes, 2, b.W, b.H, b.C, so, org, w, h, d_out[1], d_st[1])
                torch.cuda.synchronize()
            st = d_st.cpu().numpy()
            assert bool((d_out[:, n * wb:] == SENT_OUT).all()) and (st[:, n:] == SENT_ST).all()
            assert torch.equal(d_in, ref)
            assert np.array_equal(st[0, :n], st[1, :n]), (name, cls, i, np.flatnonzero(st[0, :n] != st[1, :n])[:8])
            ok = st[0, :n] == 0
            px = d_out[:, :n * wb].view(2, n, wb)   # (compared on the device: the wide bases' windows are 37 MB a call)
            d_ok = torch.from_numpy(ok).cuda()
            assert torch.equal(px[0][d_ok], px[1][d_ok]), (name, cls, i)
            assert ok[so == 0].all(), (name, cls, i)
            n_fail += int((~ok[so == 1]).sum())
            n_ok += int(ok[so == 1].sum())
        assert n_fail > 0 and (n_ok > 0 or b.H <= 8), (n_fail, n_ok)
    finally:
        engine.set_option("fix_t2", 0)


# ---- 6. two column strips ------------------------------------------------------------------------------

def test_two_column_strips(engine):
    W, H, Cn, w, h = 8192, 64, 4, 4161, 20
    s, full = sc.stream("randtile", W, H, Cn), sc.full("randtile", W, H, Cn)
    org = np.array([(0, 0), (W - w, 10), (2000, 5), (17, 44)], np.int32)
    o = Opened(engine, [s], W, H, Cn)
    for part in (slice(0, 2), slice(2, 4)):
        st, out = o.call(np.zeros(2, np.int32), org[part], w, h)
        assert (st == 0).all(), st
        for k, (x, y) in enumerate(org[part]):
            assert np.array_equal(out[k], _crop(full, (x, y, w, h))), (part, k)
    o.done()


# ---- 7. the host form ------------------------------------------------------------------------------------

def test_host_form(engine):
    so, org = sc.windows()
    org0 = np.ascontiguousarray(org[so == 0])
    cases = sc.independence_cases()
    n_fail = 0
    for what, s in [("clean", sc.stream()), ("payload", cases["payload"][1]), ("header", cases["header"][1])]:
        if what == "header":
            with pytest.raises(himg_amd.HimgError):
                himg_amd.index_host(s)   # (the host cannot index it: the device walk runs)
        with engine.open_stream(s) as o:
            assert o.info()["n_streams"] == 1 and o.info()["device_bytes"] >= himg_amd.opened_bytes(sc.W, sc.H, sc.C) + len(s)
            for w, h, oo in [sc.WIN + (org0,), sc.WIN + (org0[::-1],), (sc.W, sc.H, np.array([(0, 0)], np.int32))]:
                got, st = o.regions(oo, w, h)
                want, st0 = engine.decode_stream_regions(s, oo, w, h)
                assert np.array_equal(st, st0), (what, w, h, st, st0)
                assert got.shape == (len(oo), h, w, sc.C)
                for k in range(len(oo)):
                    if st[k] == 0:
                        assert np.array_equal(got[k], want[k]), (what, w, h, k)
                n_fail += int((st != 0).sum())
            assert o.info()["rows_counted"] == sc.ROWS
    assert n_fail > 0
    # a short or missing dst: HIMG_ERR_CAPACITY, the geometry set, dst untouched, nothing decoded
    L, s = himg_amd.lib(), sc.stream()
    n, (w, h) = len(org0), sc.WIN
    with engine.open_stream(s) as o:
        for dst_len in (n * h * w * sc.C - 1, 16, 0):
            dst = np.full(max(dst_len, 1) + 32, 0x77, np.uint8)
            st = np.full(n, 7, np.int32)
            wo, ho, co = C.c_int(), C.c_int(), C.c_int()
            rc = L.himg_hip_opened_regions_to(engine._ctx, o._h, n, None, org0.ctypes.data, w, h,
                                              dst.ctypes.data if dst_len else None, dst_len, st.ctypes.data, C.byref(wo),
                                              C.byref(ho), C.byref(co))
            assert rc == himg_amd.HIMG_ERR_CAPACITY and (wo.value, ho.value, co.value) == (w, h, sc.C)
            assert (dst == 0x77).all() and (st == 7).all() and o.info()["rows_counted"] == 0
        # and with room: the bytes, and nothing behind them
        dst = np.full(n * h * w * sc.C + 32, 0x77, np.uint8)
        st = np.full(n + 2, 7, np.int32)
        rc = L.himg_hip_opened_regions_to(engine._ctx, o._h, n, None, org0.ctypes.data, w, h, dst.ctypes.data,
                                          n * h * w * sc.C, st.ctypes.data, C.byref(wo), C.byref(ho), C.byref(co))
        assert rc == 0 and (dst[-32:] == 0x77).all() and (st[:n] == 0).all() and (st[n:] == 7).all()
        want, _ = engine.decode_stream_regions(s, org0, w, h)
        assert np.array_equal(dst[:-32].reshape(want.shape), want)
        with pytest.raises(himg_amd.HimgError) as e:
            o.regions([(0, 0), (sc.W, 0)], w, h)
        assert e.value.code == ARG
        with pytest.raises(himg_amd.HimgError) as e:
            o.regions([(0, 0)], w, h, stream_of=[1])
        assert e.value.code == ARG
    with pytest.raises(himg_amd.HimgError) as e:
        engine.open_stream(np.zeros(64, np.uint8))
    assert e.value.code == himg_amd.HIMG_ERR_FORMAT


# ---- 8. arguments -----------------------------------------------------------------------------------

def test_argument_errors(engine):
    s = sc.stream()
    w, h = sc.WIN
    o = Opened(engine, [s, s], sc.W, sc.H, sc.C)
    L = himg_amd.lib()
    ok_so, ok_org = np.array([0, 1], np.int32), np.array([(0, 0), (5, 5)], np.int32)
    d_out = torch.full((4 * w * h * sc.C + 16,), SENT_OUT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((70000,), SENT_ST, dtype=torch.int32, device="cuda")

    def untouched(what):
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENT_OUT).all() and (d_st.cpu().numpy() == SENT_ST).all(), what
        assert o.h.info()["rows_counted"] == 0, what

    def raw(ctx, handle, so=ok_so, org=ok_org, n=2, ww=w, hh=h, out=d_out, st=d_st):
        return L.himg_hip_opened_regions_device(ctx, handle, so.ctypes.data if so is not None else None,
                                                org.ctypes.data if org is not None else None, n, ww, hh,
                                                out.data_ptr() if out is not None else None,
                                                st.data_ptr() if st is not None else None, None)

    other = himg_amd.Engine(0)
    try:
        assert raw(engine._ctx, None) == ARG                 # a NULL handle
        assert raw(None, o.h._h) == ARG                      # no context
        assert raw(other._ctx, o.h._h) == ARG                # another context's handle
        with pytest.raises(himg_amd.HimgError) as e:
            o.h.regions_device(ok_so, ok_org, w, h, d_out, d_st, engine=other)
        assert e.value.code == ARG
        untouched("handle and context")
        cases = [([0, 2], ok_org, w, h), ([-1, 0], ok_org, w, h), (ok_so, [(0, 0), (sc.W - w + 1, 0)], w, h),
                 (ok_so, [(0, sc.H - h + 1), (0, 0)], w, h), (ok_so, [(0, 0), (-1, 0)], w, h), (ok_so, ok_org, 0, h),
                 (ok_so, ok_org, w, 0), ([], [], w, h), ([0] * 65536, [(0, 0)] * 65536, 1, 1)]
        for so, org, ww, hh in cases:
            with pytest.raises(himg_amd.HimgError) as e:
                o.h.regions_device(so, org, ww, hh, d_out, d_st)
            assert e.value.code == ARG, (list(so)[:4], list(org)[:4])
            untouched((list(so)[:4], list(org)[:4], ww, hh))
        for kw in [dict(so=None), dict(org=None), dict(out=None), dict(st=None), dict(n=0), dict(n=-1)]:
            assert raw(engine._ctx, o.h._h, **kw) == ARG, kw
        untouched("NULLs")
        # open's own: NULLs, stream counts, a stride that does not cover a stream, a bad geometry
        good = dict(d_packed=o.d_in, in_stride=o.stride, h_sizes=o.sizes, n_streams=2, width=sc.W, height=sc.H, channels=sc.C)
        for key, val in [("d_packed", None), ("h_sizes", None), ("n_streams", 0), ("n_streams", 65536), ("in_stride", 8),
                         ("width", 0), ("channels", 5)]:
            with pytest.raises(himg_amd.HimgError) as e:
                engine.open_streams_device(**dict(good, **{key: val}))
            assert e.value.code == ARG, key
        # the handle still works, and a closed handle is refused
        st, out = o.call(ok_so, ok_org, w, h)
        assert (st == 0).all() and o.h.info()["rows_counted"] == 6
        stale = C.c_void_p(o.h._h.value)
        o.done()
        d_out.fill_(SENT_OUT)
        d_st.fill_(SENT_ST)
        assert raw(engine._ctx, stale) == ARG
        with pytest.raises(himg_amd.HimgError) as e:
            o.h.regions_device(ok_so, ok_org, w, h, d_out, d_st)
        assert e.value.code == ARG
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENT_OUT).all() and (d_st.cpu().numpy() == SENT_ST).all()
    finally:
        other.close()


def test_destroy_closes_the_handles_that_are_left():
    e = himg_amd.Engine(0)
    s = sc.stream()
    d_in, stride = _upload([s])
    h1 = e.open_streams_device(d_in, stride, [len(s)], 1, sc.W, sc.H, sc.C)
    h2 = e.open_stream(s)
    got, st = h2.regions([(0, 0)], *sc.WIN)
    assert (st == 0).all() and np.array_equal(got[0], _crop(sc.full(), (0, 0) + sc.WIN))
    e.close()
    h1.close()   # (the context took the handles with it: nothing left to free)
    h2.close()


# ---- 9. a caller's stream ------------------------------------------------------------------------------

def test_callers_stream_gated(engine):
    """Open and two calls on the handle on the caller's non-blocking stream behind tests/stream_gate.py's gate,
    no host wait between them; a decoy decode on the same context goes in front (four calls: one for each of
    the context's pinned slots, so none waits for a copy behind the gate)."""
    import stream_gate as sg
    streams = [sc.stream(seed=0), sc.stream(seed=1)]
    fulls = [sc.full(seed=0), sc.full(seed=1)]
    w, h = sc.WIN
    maps = [sc.windows(), (MAP12, sc.origins12(sc.W, sc.H, w, h, np.random.default_rng(23)))]
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    real, decoy = np.zeros((2, stride), np.uint8), np.zeros((2, stride), np.uint8)
    for i, s in enumerate(streams):
        real[i, :len(s)] = s
        decoy[1 - i, :len(s)] = s
    sizes = [len(s) for s in streams]
    outs = {"decoy_pix": (12 * h * w * sc.C, SENT_OUT), "decoy_st": (4 * 12, 0x9D)}
    for j, (so, _) in enumerate(maps):
        outs["pix%d" % j] = (len(so) * h * w * sc.C, SENT_OUT)
        outs["st%d" % j] = (4 * len(so), 0x9D)
    gate = sg.Gate(log=lambda *a: None)
    S = gate.self_check()
    assert S is not None, "inconclusive: no torch stream ran independently of the null stream"
    buf = sg.Buffers(torch, real, decoy, outs)
    handles = []

    def decoy_decode():
        engine.decode_stream_regions_device(buf.d_in, stride, sizes, 2, sc.W, sc.H, sc.C, MAP12, maps[1][1], w, h,
                                            buf.outs["decoy_pix"][0], buf.outs["decoy_st"][0], stream=S.cuda_stream)

    def issue():
        decoy_decode()
        o = engine.open_streams_device(buf.d_in, stride, sizes, 2, sc.W, sc.H, sc.C, stream=S.cuda_stream)
        handles.append(o)
        for j, (so, org) in enumerate(maps):
            o.regions_device(so, org, w, h, buf.outs["pix%d" % j][0], buf.outs["st%d" % j][0], stream=S.cuda_stream)

    def check(what):
        for j, (so, org) in enumerate(maps):
            st = buf.result("st%d" % j).view(np.int32)
            assert (st == 0).all(), (what, j, st)
            px = buf.result("pix%d" % j).reshape(len(so), h, w, sc.C)
            for k in range(len(so)):
                assert np.array_equal(px[k], _crop(fulls[so[k]], (org[k][0], org[k][1], w, h))), (what, j, k)
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
    """Five streams at an in_stride of 2^30: stream 4 starts at 2^32, streams 2 and 3 beyond 2^31.  Stream f holds
    picture f % 3, so an offset that wraps lands on another valid stream and shows as wrong pixels.  Windows of
    stream 4 come in a second call, on rows the first call has not counted.  Need: 4 GiB + 1 MiB for the input
    and 1 GiB of allowance; skips with less free device memory."""
    GIB = 1 << 30
    n_bytes = 4 * GIB + (1 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < n_bytes + GIB:
        pytest.skip("needs %d bytes of device memory, %d are free" % (n_bytes + GIB, free))
    eng = himg_amd.Engine(0)
    try:
        streams = [sc.stream(seed=f % 3) for f in range(5)]
        fulls = [sc.full(seed=f % 3) for f in range(5)]
        far = torch.full((n_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        for f, s in enumerate(streams):
            far[f * GIB:f * GIB + len(s)] = torch.from_numpy(s.copy()).cuda()
            far[f * GIB + len(s):f * GIB + len(s) + 64] = 0   # (the bit readers' look-ahead: as _upload leaves it)

        def digest():
            torch.cuda.synchronize()
            return [int(far[a:a + (256 << 20)].view(torch.int64).sum().item()) for a in range(0, 4 * GIB, 256 << 20)] + \
                   [far[f * GIB:f * GIB + len(s)].clone() for f, s in enumerate(streams)]

        before = digest()
        w, h = sc.WIN
        d_hs = torch.full((5,), SENT_ST, dtype=torch.int32, device="cuda")
        with eng.open_streams_device(far, GIB, [len(s) for s in streams], 5, sc.W, sc.H, sc.C, d_head_status=d_hs) as o:
            calls = [(np.array([0, 3, 2, 1, 3], np.int32), np.array([(0, 0), (72, 55), (33, 30), (7, 20), (5, 3)], np.int32)),
                     (np.array([4, 2, 4, 4], np.int32), np.array([(72, 55), (0, 0), (5, 3), (33, 30)], np.int32))]
            for so, org in calls:
                n = len(so)
                nb = n * h * w * sc.C
                d_out = torch.full((nb + 64,), SENT_OUT, dtype=torch.uint8, device="cuda")
                d_st = torch.full((n + 4,), SENT_ST, dtype=torch.int32, device="cuda")
                o.regions_device(so, org, w, h, d_out, d_st)
                torch.cuda.synchronize()
                out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
                assert (out[nb:] == SENT_OUT).all() and (st[n:] == SENT_ST).all() and (st[:n] == 0).all(), st
                px = out[:nb].reshape(n, h, w, sc.C)
                for k in range(n):
                    assert np.array_equal(px[k], _crop(fulls[so[k]], (org[k][0], org[k][1], w, h))), (so[k], org[k])
            assert (d_hs.cpu().numpy() == 0).all()
        after = digest()
        assert before[:16] == after[:16] and all(torch.equal(a, b) for a, b in zip(before[16:], after[16:]))
        del far
    finally:
        eng.close()
        gc.collect()
        torch.cuda.empty_cache()
