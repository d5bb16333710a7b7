"""GPU: many windows of one stream behind a single head pass -- decode_stream_regions_device (a window ->
stream map) and decode_stream_regions (one host stream) against the oracle's full decode, cropped, byte for
byte; against decode_regions_device over the batch with a stream copied per window, status word for status
word; the independence of windows within a damaged stream, by damage_model; bytes used; nothing else
written; argument errors; the host form; a caller's stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import himg_amd
import damage_model as dm
import stream_region_cases as sc
from test_gpu_region import _crop, _keep

pytestmark = pytest.mark.gpu

SENT_OUT, SENT_ST = 0x5A, -99


def _upload(streams, keeps=None):
    """The batch at one stride; keeps[i]: upload only those byte ranges of stream i and poison the rest."""
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5 if keeps else 0, np.uint8)
    for i, s in enumerate(streams):
        if keeps:
            for a, e in keeps[i]:
                buf[i, max(a, 0):e] = s[max(a, 0):e]
        else:
            buf[i, :len(s)] = s
    return torch.from_numpy(buf).cuda(), stride


def _run(eng, streams, W, H, Cn, stream_of, origins, w, h, keeps=None):
    """decode_stream_regions_device with sentinels behind d_out and d_status: (statuses, pixels [n, h, w, C])."""
    n = len(stream_of)
    d_in, stride = _upload(streams, keeps)
    d_out = torch.full((n * h * w * Cn + 64,), SENT_OUT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n + 4,), SENT_ST, dtype=torch.int32, device="cuda")
    eng.decode_stream_regions_device(d_in, stride, [len(s) for s in streams], len(streams), W, H, Cn, stream_of, origins,
                                     w, h, d_out, d_st)
    torch.cuda.synchronize()
    out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
    assert (out[n * h * w * Cn:] == SENT_OUT).all() and (st[n:] == SENT_ST).all()
    return st[:n], out[:n * h * w * Cn].reshape(n, h, w, Cn)


def _expanded(eng, streams, W, H, Cn, stream_of, origins, w, h):
    """decode_regions_device over the batch with a stream copied per window."""
    n = len(stream_of)
    batch = [streams[s] for s in stream_of]
    d_in, stride = _upload(batch)
    d_out = torch.full((n * h * w * Cn + 16,), SENT_OUT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), SENT_ST, dtype=torch.int32, device="cuda")
    eng.decode_regions_device(d_in, stride, [len(s) for s in batch], n, W, H, Cn, origins, w, h, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy()[:n * h * w * Cn].reshape(n, h, w, Cn)


_origins = sc.origins12


MAP12 = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1], np.int32)   # unsorted, one stream ten times, the other twice

SHAPES = [("randtile", 96, 72, 4, 50), ("gradn", 50, 41, 3, 90), ("randtile", 33, 9, 1, 50)]


@pytest.fixture(scope="module", params=[0, 1], ids=["count", "count_w"])
def eng_wave(request):
    e = himg_amd.Engine(0)
    e.set_option("count_wave", request.param)
    yield e
    e.close()


@pytest.mark.parametrize("kind,W,H,Cn,q", SHAPES)
def test_parity(eng_wave, kind, W, H, Cn, q):
    streams = [sc.stream(kind, W, H, Cn, q, seed) for seed in (0, 1)]
    fulls = [sc.full(kind, W, H, Cn, q, seed) for seed in (0, 1)]
    fix = sc.needs_fix(kind, W, H, Cn, q, 0)
    assert fix == sc.needs_fix(kind, W, H, Cn, q, 1)
    eng_wave.set_option("fix_t2", int(fix))
    try:
        _parity(eng_wave, kind, W, H, Cn, streams, fulls)
    finally:
        eng_wave.set_option("fix_t2", 0)


def _parity(eng_wave, kind, W, H, Cn, streams, fulls):
    rng = np.random.default_rng(17)
    for w, h in [(min(24, W), min(17, H)), (1, 1), (W, H)]:
        org = _origins(W, H, w, h, rng)
        st, out = _run(eng_wave, streams, W, H, Cn, MAP12, org, w, h)
        assert (st == 0).all(), (w, h, st)
        for k in range(12):
            assert np.array_equal(out[k], _crop(fulls[MAP12[k]], (org[k][0], org[k][1], w, h))), (kind, w, h, k)
    # identical windows given twice
    w, h = min(24, W), min(17, H)
    org = np.concatenate([_origins(W, H, w, h, rng)[3:6]] * 2)
    so = np.array([1, 0, 1] * 2, np.int32)
    st, out = _run(eng_wave, streams, W, H, Cn, so, org, w, h)
    assert (st == 0).all() and np.array_equal(out[:3], out[3:])
    for k in range(3):
        assert np.array_equal(out[k], _crop(fulls[so[k]], (org[k][0], org[k][1], w, h)))


def test_two_column_strips(engine):
    """Windows 4161 wide of an 8192-wide frame take two column strips of the row kernel; three overlap in rows."""
    W, H, Cn, w, h = 8192, 64, 4, 4161, 20
    s, full = sc.stream("randtile", W, H, Cn), sc.full("randtile", W, H, Cn)
    org = np.array([(0, 0), (W - w, 10), (2000, 5), (17, 44)], np.int32)
    st, out = _run(engine, [s], W, H, Cn, np.zeros(4, np.int32), org, w, h)
    assert (st == 0).all(), st
    for k in range(4):
        assert np.array_equal(out[k], _crop(full, (org[k][0], org[k][1], w, h))), k


def _corpus_windows(name, cls):
    """All of the corpus's rectangles of the base's window size -- origins(name, cls), drawn around each stream's
    damaged row, and one_rect -- once for each of the two streams.  (Class C damages no row: class P's origins.)"""
    pool = list(dm.origins(name, cls if cls != "C" else "P")) + [dm.one_rect(name)[:2]]
    org = np.array(pool + pool, np.int32)
    so = np.array([1] * len(pool) + [0] * len(pool), np.int32)
    return so, org


@pytest.mark.parametrize("cls", "PHC")
@pytest.mark.parametrize("name", [b.name for b in dm.BASES])
def test_equals_regions_device_on_the_corpus(engine, name, cls):
    """EVERY damaged stream of the corpus's class: one call on [good, bad] with all of the class's same-size
    rectangles for both streams (482 windows, 242 on the wide bases) against decode_regions_device over the
    expanded batch, a stream copied per window.  The status words are equal word for word, the pixels wherever
    the status is 0; the good stream's windows all pass, and over the class windows of the damaged streams
    both pass and fail (class C: a head verdict fails every window of its stream)."""
    b, m = dm.BASE[name], dm.good_model(name)
    ss = dm.streams(name, cls)
    if not ss:
        return   # (a frame of one block row has no size header to damage)
    engine.set_option("fix_t2", int(b.fix))
    w, h = b.win
    so, org = _corpus_windows(name, cls)
    n, wb = len(so), h * w * b.C
    d_so = torch.from_numpy(so.astype(np.int64)).cuda()
    d_out = torch.empty((2, (n * wb + 64 + 255) // 256 * 256), dtype=torch.uint8, device="cuda")   # (rows 16-byte aligned)
    d_st = torch.empty((2, n + 4), dtype=torch.int32, device="cuda")
    try:
        n_fail = n_ok = 0
        for i, s in enumerate(ss):
            streams = [m.packed, s.bad]
            d_in, stride = _upload(streams)
            sizes = [len(x) for x in streams]
            d_out.fill_(SENT_OUT)
            d_st.fill_(SENT_ST)
            engine.decode_stream_regions_device(d_in, stride, sizes, 2, b.W, b.H, b.C, so, org, w, h, d_out[0], d_st[0])
            engine.decode_regions_device(d_in[d_so].contiguous(), stride, [sizes[k] for k in so], n, b.W, b.H, b.C, org, w, h,
                                         d_out[1], d_st[1])
            torch.cuda.synchronize()
            st, out = d_st.cpu().numpy(), d_out.cpu().numpy()
            assert (out[:, n * wb:] == SENT_OUT).all() and (st[:, n:] == SENT_ST).all()
            assert np.array_equal(st[0, :n], st[1, :n]), (name, cls, i, np.flatnonzero(st[0, :n] != st[1, :n])[:8])
            ok = st[0, :n] == 0
            px = out[:, :n * wb].reshape(2, n, wb)
            assert np.array_equal(px[0][ok], px[1][ok]), (name, cls, i)
            assert ok[so == 0].all(), (name, cls, i)
            n_fail += int((~ok[so == 1]).sum())
            n_ok += int(ok[so == 1].sum())
        assert n_fail > 0 and (n_ok > 0 or b.H <= 8), (n_fail, n_ok)
    finally:
        engine.set_option("fix_t2", 0)


@pytest.mark.parametrize("name", ["payload", "header", "cut", "surplus", "head"])
def test_independence_within_a_stream(eng_wave, name):
    """Windows above, across and below the damage of stream 0, and windows of a clean stream 1: every window's
    verdict and pixels are damage_model.expect_region's for it alone."""
    good, bad, clean = sc.independence_cases()[name]
    so, org = sc.windows()
    st, out = _run(eng_wave, [bad, clean], sc.W, sc.H, sc.C, so, org, *sc.WIN)
    exp = sc.expected(name)
    for k, (code, crop) in enumerate(exp):
        assert (st[k] == 0) == (code == dm.OK), (name, k, so[k], org[k], st[k], code)
        if code == dm.OK:
            assert np.array_equal(out[k], crop), (name, k)
    st1, out1 = _expanded(eng_wave, [bad, clean], sc.W, sc.H, sc.C, so, org, *sc.WIN)
    assert np.array_equal(st, st1)
    # a failed window's neighbours in d_out are intact: they are the windows around it, judged above
    assert (st[so == 1] == 0).all()


def _keeps(streams, so, org, w, h):
    """Per stream, the union of its windows' _keep ranges (a stream no window names: nothing)."""
    keeps = [[] for _ in streams]
    for s, (x, y) in zip(so, org):
        keeps[s] += _keep(streams[s], himg_amd.region_peek(streams[s], int(x), int(y), w, h))
    return keeps


def test_bytes_used(engine):
    for kind, W, H, Cn, q in SHAPES[:2]:
        streams = [sc.stream(kind, W, H, Cn, q, seed) for seed in (0, 1)]
        fulls = [sc.full(kind, W, H, Cn, q, seed) for seed in (0, 1)]
        w, h = 24, 17
        org = _origins(W, H, w, h, np.random.default_rng(5))
        st, out = _run(engine, streams, W, H, Cn, MAP12, org, w, h, keeps=_keeps(streams, MAP12, org, w, h))
        assert (st == 0).all(), st
        for k in range(12):
            assert np.array_equal(out[k], _crop(fulls[MAP12[k]], (org[k][0], org[k][1], w, h))), (kind, k)
    # windows in the upper rows only: nothing below them is present
    s, full = sc.stream(), sc.full()
    so, org = np.zeros(3, np.int32), np.array([(0, 0), (40, 9), (72, 3)], np.int32)
    st, out = _run(engine, [s], sc.W, sc.H, sc.C, so, org, *sc.WIN, keeps=_keeps([s], so, org, *sc.WIN))
    assert (st == 0).all()
    for k in range(3):
        assert np.array_equal(out[k], _crop(full, (org[k][0], org[k][1]) + sc.WIN))


def test_a_stream_no_window_names(engine):
    s0, s1 = sc.stream(seed=0), sc.stream(seed=1)
    garbage = np.random.default_rng(9).integers(0, 256, len(s0), dtype=np.uint8)
    so, org = sc.windows()
    st, out = _run(engine, [s0, s1], sc.W, sc.H, sc.C, so, org, *sc.WIN)
    st2, out2 = _run(engine, [s0, garbage, s1], sc.W, sc.H, sc.C, so * 2, org, *sc.WIN)
    assert (st == 0).all() and np.array_equal(st, st2) and np.array_equal(out, out2)


def test_argument_errors(engine):
    s = sc.stream()
    d_in, stride = _upload([s, s])
    w, h = sc.WIN
    ok_so, ok_org = [0, 1], [(0, 0), (5, 5)]
    cases = [([0, 2], ok_org, w, h), ([-1, 0], ok_org, w, h), (ok_so, [(0, 0), (sc.W - w + 1, 0)], w, h),
             (ok_so, [(0, sc.H - h + 1), (0, 0)], w, h), (ok_so, [(0, 0), (-1, 0)], w, h), (ok_so, ok_org, 0, h),
             ([], [], w, h), ([0] * 65536, [(0, 0)] * 65536, 1, 1)]
    for so, org, ww, hh in cases:
        n = max(len(so), 1)
        d_out = torch.full((min(n, 4) * max(ww, 1) * hh * sc.C + 16,), SENT_OUT, dtype=torch.uint8, device="cuda")
        d_st = torch.full((min(n, 70000),), SENT_ST, dtype=torch.int32, device="cuda")
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_stream_regions_device(d_in, stride, [len(s)] * 2, 2, sc.W, sc.H, sc.C, so, org, ww, hh, d_out, d_st)
        assert e.value.code == himg_amd.HIMG_ERR_ARG, (so[:4], org[:4])
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENT_OUT).all() and (d_st.cpu().numpy() == SENT_ST).all(), (so[:4], org[:4])
    # NULLs and stream counts
    d_out = torch.full((2 * w * h * sc.C,), SENT_OUT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((2,), SENT_ST, dtype=torch.int32, device="cuda")
    good = dict(d_packed=d_in, in_stride=stride, h_sizes=[len(s)] * 2, n_streams=2, width=sc.W, height=sc.H,
                channels=sc.C, stream_of=ok_so, origins=ok_org, w=w, h=h, d_out=d_out, d_status=d_st)
    for key, val in [("d_packed", None), ("h_sizes", None), ("stream_of", None), ("origins", None), ("d_out", None),
                     ("d_status", None), ("n_streams", 0), ("n_streams", 65536)]:
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_stream_regions_device(**dict(good, **{key: val}))
        assert e.value.code == himg_amd.HIMG_ERR_ARG, key
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENT_OUT).all() and (d_st.cpu().numpy() == SENT_ST).all()


def _region_to(eng, s, rect):
    try:
        return 0, eng.decode_region(s, *rect)
    except himg_amd.HimgError as e:
        return e.code, None


def test_host_form(engine):
    """decode_stream_regions against decode_region per rectangle: clean streams, the damaged streams of the
    independence cases (the header case is a stream the host cannot index: the whole upload and the device
    walk), a frame of one block row; then the capacity protocol."""
    so, org = sc.windows()
    org0 = org[so == 0]
    todo = [(sc.stream(), org0, sc.WIN), (sc.stream("gradn", 50, 41, 3, 90), _origins(50, 41, 24, 17, np.random.default_rng(2)), (24, 17)),
            (sc.stream("randtile", 40, 8, 4, 50), np.array([(0, 0), (23, 3), (5, 1)], np.int32), (17, 5))]
    todo += [(sc.independence_cases()[k][1], org0, sc.WIN) for k in ("payload", "header", "cut", "surplus", "head")]
    for s, o, (w, h) in todo:
        got, st = engine.decode_stream_regions(s, o, w, h)
        assert got.shape[:3] == (len(o), h, w)
        for k, (x, y) in enumerate(o):
            code, px = _region_to(engine, s, (int(x), int(y), w, h))
            assert st[k] == code, (k, st, code)
            if code == 0:
                assert np.array_equal(got[k], px), k
    # the capacity protocol: the dimensions and the statuses come back, fetch_last copies the resident result
    s, L = sc.stream(), himg_amd.lib()
    o = np.ascontiguousarray(org0)
    n, (w, h) = len(o), sc.WIN
    want, _ = engine.decode_stream_regions(s, o, w, h)
    st = np.full(n, 7, np.int32)
    wo, ho, co = C.c_int(), C.c_int(), C.c_int()
    small = np.zeros(16, np.uint8)
    rc = L.himg_hip_decode_stream_regions_to(engine._ctx, s.ctypes.data, s.nbytes, n, o.ctypes.data, w, h, small.ctypes.data,
                                             small.nbytes, st.ctypes.data, C.byref(wo), C.byref(ho), C.byref(co))
    assert rc == himg_amd.HIMG_ERR_CAPACITY and (wo.value, ho.value, co.value) == (w, h, sc.C) and (st == 0).all()
    buf = np.zeros(n * h * w * sc.C, np.uint8)
    nb = C.c_size_t()
    assert L.himg_hip_fetch_last(engine._ctx, buf.ctypes.data, buf.nbytes, C.byref(nb)) == 0 and nb.value == buf.nbytes
    assert np.array_equal(buf.reshape(want.shape), want)
    with pytest.raises(himg_amd.HimgError) as e:
        engine.decode_stream_regions(s, [(0, 0), (sc.W, 0)], w, h)
    assert e.value.code == himg_amd.HIMG_ERR_ARG


def test_callers_stream_gated_and_queued_twice(engine):
    """The device entry behind tests/stream_gate.py's gate: the caller's non-blocking stream is held shut by a
    device-side delay; behind it the real input is copied over a decoy (the two streams swapped: a valid input
    with other pixels), the entry is called twice with different maps and no host wait between, and the outputs
    are copied to pinned memory, all on that stream; the host waits for the last copy alone.  A kernel or a
    staged word on the null stream would run while the gate is shut -- reading the decoy, or overwritten by the
    reset patterns' successors -- and a host synchronisation inside the entry would not return before the gate
    opens."""
    import stream_gate as sg
    streams = [sc.stream(seed=0), sc.stream(seed=1)]
    fulls = [sc.full(seed=0), sc.full(seed=1)]
    w, h = sc.WIN
    maps = [sc.windows(), (MAP12, _origins(sc.W, sc.H, w, h, np.random.default_rng(23)))]
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    real, decoy = np.zeros((2, stride), np.uint8), np.zeros((2, stride), np.uint8)
    for i, s in enumerate(streams):
        real[i, :len(s)] = s
        decoy[1 - i, :len(s)] = s
    sizes = [len(s) for s in streams]   # (the real input's, as tests/stream_cases.py packs its decoys)
    assert not np.array_equal(real, decoy)
    outs = {}
    for j, (so, _) in enumerate(maps):
        outs["pix%d" % j] = (len(so) * h * w * sc.C, SENT_OUT)
        outs["st%d" % j] = (4 * len(so), 0x9D)
    gate = sg.Gate(log=lambda *a: None)
    S = gate.self_check()
    assert S is not None, "inconclusive: no torch stream ran independently of the null stream"
    buf = sg.Buffers(torch, real, decoy, outs)

    def issue():
        for j, (so, org) in enumerate(maps):
            engine.decode_stream_regions_device(buf.d_in, stride, sizes, 2, sc.W, sc.H, sc.C, so, org, w, h,
                                                buf.outs["pix%d" % j][0], buf.outs["st%d" % j][0], stream=S.cuda_stream)

    def check(what):
        for j, (so, org) in enumerate(maps):
            st = buf.result("st%d" % j).view(np.int32)
            assert (st == 0).all(), (what, j, st)
            px = buf.result("pix%d" % j).reshape(len(so), h, w, sc.C)
            for k in range(len(so)):
                assert np.array_equal(px[k], _crop(fulls[so[k]], (org[k][0], org[k][1], w, h))), (what, j, k)

    # warm-up on S, ungated: the first call reserves (and may wait for the device), the second is timed on the host
    buf.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        buf.queue_input()
    issue()
    S.synchronize()
    host_s = sg.timed_call(issue)
    with torch.cuda.stream(S):
        buf.queue_collect()
    S.synchronize()
    check("warm-up")
    # gated: from here to the wait no device-wide synchronise, no .cpu(), nothing on the default stream
    buf.reset()
    torch.cuda.synchronize()
    opened = gate.shut(S, sg.gate_ms(host_s))
    with torch.cuda.stream(S):
        buf.queue_input()
    issue()
    returned_while_shut = not opened.query()
    with torch.cuda.stream(S):
        buf.queue_collect()
        done = torch.cuda.Event()
        done.record(S)
    done.synchronize()
    assert returned_while_shut, "the calls waited for the device (or the host was slower than the gate is long)"
    check("gated")
