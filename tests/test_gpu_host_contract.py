"""GPU: the contract of the host decodes of one stream, entry point by entry point, as DESIGN.md tables it
("The host decodes' contract"): what himg_hip_fetch_last serves behind a call, what a too-small buffer
gets, what a damaged stream gets, and that a stream staged behind a longer one decodes bit-exactly (the
zeroed tail).  Two pictures: one block row (the device walks it) and three (the host indexes them).  The
pictures come from the oracle's decode and the models the entry points' own tests use.  (Streams this
small are ones the reference rejects as they stand, trap T2: the context and the models run with the fix.)

The fallback messages "device decode reported an error" and "device preview reported an error" belong to
status words that blame neither the format nor an argument; no stream reaches one through a host form
(the host checks the geometry first), so only the prefix forms' fallback is exercised here."""
import ctypes as C

import numpy as np
import pytest

import himg_amd
import oracle_lib as ol
import planes_model as pm
import scaled_model as sm
import stream_region_cases as sc
import test_gpu_preview as tp

pytestmark = pytest.mark.gpu

OK, ARG, FORMAT, CAPACITY = 0, himg_amd.HIMG_ERR_ARG, himg_amd.HIMG_ERR_FORMAT, himg_amd.HIMG_ERR_CAPACITY
PICTURES = {"one_row": (24, 8), "three_rows": (24, 24)}   # RGBA
MASK = 0b0101
SMALL, QCFG = "output buffer too small", "Error decoding quantization configuration.\n"
SHORT = "the prefix ends before the first block row"


def _rects(W, H):
    """A window across every block row, the same in the half-scale picture, and two origins of it."""
    full = (5, 1, 13, H - 3)
    half = (2, 1, 7, H // 2 - 2)
    return full, half


class Pic:
    """A picture's stream, its damaged form and the outputs the entry points owe for it."""

    def __init__(self, W, H):
        s = sc.stream("randtile", W, H, 4, 50, 3)
        rc, pic = ol.oracle_decode(s, fix_t2=True)
        assert rc == 0
        self.s, self.bad, self.W, self.H = s, sc.head_damaged(s), W, H
        assert -6 <= ol.oracle_decode(self.bad, fix_t2=True)[0] <= -1
        self.pic = pic.reshape(H, W, 4)
        rc1, self.half = sm.expected(s, 1, True)
        rc3, self.eighth = tp.expected(s, True)
        rcp, planes = pm.planes(s, fix_t2=True)
        assert rc1 == 0 and rc3 == 0 and rcp == 0
        self.planes = pm.select(planes, MASK)
        self.full_rect, self.half_rect = _rects(W, H)
        x, y, w, h = self.full_rect
        self.org = np.array([[x, y], [0, 0]], np.int32)
        self.crops = np.stack([self.pic[b:b + h, a:a + w] for a, b in self.org])
        x, y, w, h = self.half_rect
        self.horg = np.array([[x, y], [0, 0]], np.int32)
        self.hcrops = np.stack([self.half[b:b + h, a:a + w] for a, b in self.horg])


@pytest.fixture(scope="module")
def pics():
    return {k: Pic(*wh) for k, wh in PICTURES.items()}


@pytest.fixture(scope="module")
def engine():
    """A context of this module's own, with HIMG_OPT_FIX_T2."""
    e = himg_amd.Engine(0)
    e.set_option("fix_t2", 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def long_stream():
    """A stream far longer than the pictures': decoded first, it leaves its bytes in the staging."""
    return sc.stream("rand", 96, 72, 4, 90, 1)


def _p(a):
    return a.ctypes.data if a is not None else None


class Call:
    """One entry point: run(L, ctx, stream, dst, cap) -> (rc, (w, h, c)); want(pic) -> the bytes owed; dims(pic);
    resident: himg_hip_fetch_last serves the result; early: the capacity rule comes before the launch;
    bad: (code, message) for the stream with a spoilt head chunk, None where the call does not read it."""

    def __init__(self, name, run, want, dims, resident, early=False, bad=(FORMAT, QCFG)):
        self.name, self.run, self.want, self.dims, self.resident, self.early, self.bad = name, run, want, dims, resident, early, bad


def _dims3():
    return C.c_int(-7), C.c_int(-7), C.c_int(-7)


def _decode_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    return L.himg_hip_decode_to(ctx, _p(s), s.nbytes, dst, cap, w, h, c), (w.value, h.value, c.value)


def _prefix_to(L, ctx, p, s, dst, cap, avail=None):
    w, h, c = _dims3()
    k = C.c_int(-7)
    rc = L.himg_hip_decode_prefix_to(ctx, _p(s), s.nbytes if avail is None else avail, dst, cap, w, h, c, k)
    assert rc != OK or k.value == (p.H + 7) // 8
    return rc, (w.value, h.value, c.value)


def _prefix_more_to(L, ctx, p, s, dst, cap, avail=None):
    w, h, c = _dims3()
    k = C.c_int(-7)
    state = himg_amd.PrefixState()
    rc = L.himg_hip_decode_prefix_more_to(ctx, _p(s), s.nbytes if avail is None else avail, C.byref(state), dst, cap,
                                          w, h, c, k)
    assert rc != OK or k.value == (p.H + 7) // 8
    return rc, (w.value, h.value, c.value)


def _conceal_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    n = C.c_int(-7)
    rc = L.himg_hip_decode_conceal_to(ctx, _p(s), s.nbytes, dst, cap, w, h, c, None, 0, n)
    assert rc == FORMAT or n.value == 0
    return rc, (w.value, h.value, c.value)


def _pyramid_to(L, ctx, p, s, dst, cap):
    """Levels 0 and 1, one behind the other in dst; cap counts for level 1 alone (level 0 always fits)."""
    w, h, c = _dims3()
    n0 = p.pic.size
    dsts = (C.c_void_p * 4)(dst, dst + n0 if dst else None, None, None)
    caps = (C.c_size_t * 4)(n0 if dst else 1, max(cap - n0, 1), 0, 0)
    return L.himg_hip_decode_pyramid_to(ctx, _p(s), s.nbytes, dsts, caps, w, h, c), (w.value, h.value, c.value)


def _planes_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    return L.himg_hip_decode_planes_to(ctx, _p(s), s.nbytes, MASK, dst, cap, w, h, c), (w.value, h.value, c.value)


def _preview_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    return L.himg_hip_preview_to(ctx, _p(s), s.nbytes, dst, cap, w, h, c), (w.value, h.value, c.value)


def _region_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    return L.himg_hip_decode_region_to(ctx, _p(s), s.nbytes, *p.full_rect, dst, cap, w, h, c), (w.value, h.value, c.value)


def _scaled_region_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    rc = L.himg_hip_decode_scaled_region_to(ctx, _p(s), s.nbytes, 1, *p.half_rect, dst, cap, w, h, c)
    return rc, (w.value, h.value, c.value)


def _scaled_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    return L.himg_hip_decode_scaled_to(ctx, _p(s), s.nbytes, 1, dst, cap, w, h, c), (w.value, h.value, c.value)


def _windows_verdict(rc, st):
    """A windows call returns its first failing window's code; every window of these streams fares alike."""
    assert rc in (OK, CAPACITY) and (st == 0).all() or (st == rc).all(), (rc, st)


def _stream_regions_to(L, ctx, p, s, dst, cap):
    w, h, c = _dims3()
    st = np.full(2, -77, np.int32)
    rc = L.himg_hip_decode_stream_regions_to(ctx, _p(s), s.nbytes, 2, _p(p.org), p.full_rect[2], p.full_rect[3], dst, cap,
                                             _p(st), w, h, c)
    _windows_verdict(rc, st)
    return rc, (w.value, h.value, c.value)


def _opened(scaled):
    def run(L, ctx, p, s, dst, cap):
        o = C.c_void_p()
        assert L.himg_hip_open_stream_host(ctx, _p(s), s.nbytes, C.byref(o)) == OK   # (a head's verdict is the windows')
        w, h, c = _dims3()
        st = np.full(2, -77, np.int32)
        try:
            if scaled:
                rc = L.himg_hip_opened_scaled_regions_to(ctx, o, 1, 2, None, _p(p.horg), p.half_rect[2], p.half_rect[3],
                                                         dst, cap, _p(st), w, h, c)
            else:
                rc = L.himg_hip_opened_regions_to(ctx, o, 2, None, _p(p.org), p.full_rect[2], p.full_rect[3], dst, cap,
                                                  _p(st), w, h, c)
        finally:
            L.himg_hip_close_streams(ctx, o)
        if rc != CAPACITY:   # (the capacity rule comes before the launch: no verdict behind it)
            _windows_verdict(rc, st)
        return rc, (w.value, h.value, c.value)
    return run


def _whole(p):
    return (p.W, p.H, 4)


CALLS = [
    Call("decode_to", _decode_to, lambda p: p.pic, _whole, True),
    Call("prefix_to", _prefix_to, lambda p: p.pic, _whole, True),
    Call("prefix_more_to", _prefix_more_to, lambda p: p.pic, _whole, False, early=True),
    Call("conceal_to", _conceal_to, lambda p: p.pic, _whole, True),
    Call("pyramid_to", _pyramid_to, lambda p: np.concatenate([p.pic.ravel(), p.half.ravel()]), _whole, False, early=True),
    Call("planes_to", _planes_to, lambda p: p.planes, _whole, False),
    Call("preview_to", _preview_to, lambda p: p.eighth, lambda p: p.eighth.shape[1::-1] + (4,), True, bad=None),
    Call("region_to", _region_to, lambda p: p.crops[0], lambda p: p.full_rect[2:] + (4,), True),
    Call("scaled_region_to", _scaled_region_to, lambda p: p.hcrops[0], lambda p: p.half_rect[2:] + (4,), True),
    Call("scaled_to", _scaled_to, lambda p: p.half, lambda p: p.half.shape[1::-1] + (4,), True),
    Call("stream_regions_to", _stream_regions_to, lambda p: p.crops, lambda p: p.full_rect[2:] + (4,), True),
    Call("opened_regions_to", _opened(False), lambda p: p.crops, lambda p: p.full_rect[2:] + (4,), False, early=True),
    Call("opened_scaled_regions_to", _opened(True), lambda p: p.hcrops, lambda p: p.half_rect[2:] + (4,), False, early=True),
]
IDS = [c.name for c in CALLS]


def _fetch(L, ctx, n):
    """himg_hip_fetch_last into n bytes: (rc, size, bytes)."""
    buf = np.full(max(n, 1), 0xEE, np.uint8)
    size = C.c_size_t(123)
    rc = L.himg_hip_fetch_last(ctx, _p(buf), n, C.byref(size))
    return rc, size.value, buf[:n]


def _err(L, ctx):
    return L.himg_hip_last_error(ctx).decode()


def _dirty(L, ctx, long_stream):
    """The staging holds a long stream and its picture is the resident result."""
    out = np.empty(96 * 72 * 4, np.uint8)
    assert _decode_to(L, ctx, None, long_stream, _p(out), out.nbytes) == (OK, (96, 72, 4))


@pytest.mark.parametrize("pic", list(PICTURES))
@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_result_and_residence(engine, pics, long_stream, call, pic):
    """Behind a longer stream the call decodes bit-exactly and writes nothing behind its bytes; then
    himg_hip_fetch_last serves the result where the table says it stays, else "no result to fetch"."""
    L, ctx, p = himg_amd.lib(), engine._ctx, pics[pic]
    want = np.ascontiguousarray(call.want(p)).ravel()
    _dirty(L, ctx, long_stream)
    dst = np.full(want.size + 16, 0x5A, np.uint8)
    assert call.run(L, ctx, p, p.s, _p(dst), want.size) == (OK, call.dims(p))
    assert np.array_equal(dst[:want.size], want) and (dst[want.size:] == 0x5A).all()
    rc, size, got = _fetch(L, ctx, want.size)
    if call.resident:
        assert (rc, size) == (OK, want.size) and np.array_equal(got, want)
    else:
        assert (rc, size) == (ARG, 0) and _err(L, ctx) == "no result to fetch"


@pytest.mark.parametrize("pic", list(PICTURES))
@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_small_buffer(engine, pics, long_stream, call, pic):
    """A buffer one byte short, and none at all: the dimensions, HIMG_ERR_CAPACITY and its message; where the
    result stays resident himg_hip_fetch_last then delivers it, and where the rule comes behind the launch
    but nothing stays, it has nothing."""
    L, ctx, p = himg_amd.lib(), engine._ctx, pics[pic]
    want = np.ascontiguousarray(call.want(p)).ravel()
    for dst, cap in ((np.full(want.size, 0x5A, np.uint8), want.size - 1), (None, 0)):
        _dirty(L, ctx, long_stream)
        if call.name == "pyramid_to" and dst is None:
            continue   # (no buffer and no capacity at any level: no level wanted, another error)
        assert call.run(L, ctx, p, p.s, _p(dst), cap) == (CAPACITY, call.dims(p)), (call.name, cap)
        assert _err(L, ctx) == SMALL
        rc, size, got = _fetch(L, ctx, want.size)
        if call.resident:
            assert (rc, size) == (OK, want.size) and np.array_equal(got, want)
        elif not call.early:
            assert (rc, size) == (ARG, 0)


@pytest.mark.parametrize("pic", list(PICTURES))
@pytest.mark.parametrize("call", [c for c in CALLS if c.bad], ids=[c.name for c in CALLS if c.bad])
def test_damaged_stream(engine, pics, call, pic):
    """A stream whose QCFG chunk is gone: the device's verdict, the reference's message for that stage, and
    nothing resident -- but behind the stream-regions form, whose windows fail one by one: what the call
    delivered (here no window's pixels mean anything) stays to fetch."""
    L, ctx, p = himg_amd.lib(), engine._ctx, pics[pic]
    want = np.ascontiguousarray(call.want(p)).ravel()
    dst = np.full(want.size, 0x5A, np.uint8)
    rc, dims = call.run(L, ctx, p, p.bad, _p(dst), want.size)
    assert (rc, _err(L, ctx)) == call.bad
    assert _fetch(L, ctx, want.size)[:2] == ((OK, want.size) if call.name == "stream_regions_to" else (ARG, 0))


@pytest.mark.parametrize("pic", list(PICTURES))
def test_preview_reads_the_head_alone(engine, pics, pic):
    """The preview form does not see damage behind LRES."""
    L, ctx, p = himg_amd.lib(), engine._ctx, pics[pic]
    dst = np.full(p.eighth.size, 0x5A, np.uint8)
    assert _preview_to(L, ctx, p, p.bad, _p(dst), dst.size)[0] == OK and np.array_equal(dst, p.eighth.ravel())


@pytest.mark.parametrize("pic", list(PICTURES))
@pytest.mark.parametrize("run", [_prefix_to, _prefix_more_to], ids=["prefix_to", "prefix_more_to"])
def test_prefix_fallback_message(engine, pics, run, pic):
    """A prefix that ends behind FRMT and before the first block row: the prefix forms' own message."""
    L, ctx, p = himg_amd.lib(), engine._ctx, pics[pic]
    dst = np.full(p.pic.size, 0x5A, np.uint8)
    rc, _ = run(L, ctx, p, p.s, _p(dst), dst.size, avail=40)
    assert (rc, _err(L, ctx)) == (CAPACITY, SHORT)
    assert _fetch(L, ctx, dst.size)[:2] == (ARG, 0)


@pytest.mark.parametrize("pic", list(PICTURES))
def test_malloc_and_into_forms(engine, pics, long_stream, pic):
    """himg_hip_decode and himg_hip_decode_into_to: decode_to's decode, the result resident."""
    L, ctx, p = himg_amd.lib(), engine._ctx, pics[pic]
    _dirty(L, ctx, long_stream)
    assert np.array_equal(engine.decode(p.s).reshape(p.pic.shape), p.pic)
    rc, size, got = _fetch(L, ctx, p.pic.size)
    assert (rc, size) == (OK, p.pic.size) and np.array_equal(got, p.pic.ravel())
    _dirty(L, ctx, long_stream)
    data = np.full((p.H + 2, p.W + 3, 4), 0x5A, np.uint8)
    assert engine.decode_into(p.s, data, himg_amd.dst_desc(p.W + 3, p.H + 2, 4), 2, 1) == (p.W, p.H, 4)
    assert np.array_equal(data[1:1 + p.H, 2:2 + p.W], p.pic)
    data[1:1 + p.H, 2:2 + p.W] = 0x5A
    assert (data == 0x5A).all()
    rc, size, got = _fetch(L, ctx, p.pic.size)
    assert (rc, size) == (OK, p.pic.size) and np.array_equal(got, p.pic.ravel())
    with pytest.raises(himg_amd.HimgError) as e:
        engine.decode(p.bad)
    assert e.value.code == FORMAT and _err(L, ctx) == QCFG and _fetch(L, ctx, 1)[:2] == (ARG, 0)


@pytest.mark.parametrize("pic", list(PICTURES))
def test_open_stream_host_keeps_the_resident_result(engine, pics, long_stream, pic):
    """himg_hip_open_stream_host stages into memory of the handle's own: what himg_hip_fetch_last serves stays."""
    L, ctx, p = himg_amd.lib(), engine._ctx, pics[pic]
    out = np.empty(p.pic.size, np.uint8)
    assert _decode_to(L, ctx, p, p.s, _p(out), out.nbytes)[0] == OK
    o = C.c_void_p()
    assert L.himg_hip_open_stream_host(ctx, _p(long_stream), long_stream.nbytes, C.byref(o)) == OK
    L.himg_hip_close_streams(ctx, o)
    rc, size, got = _fetch(L, ctx, p.pic.size)
    assert (rc, size) == (OK, p.pic.size) and np.array_equal(got, p.pic.ravel())
