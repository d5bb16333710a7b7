"""GPU (-m gpu): the scaled region decode (himg_hip_decode_scaled_region_to, _scaled_regions_device,
_scaled_regions_batch) against its definition, byte for byte: a window is the crop of the scaled
decode's model (tests/scaled_model.py) -- through the host call, the device batch with an origin per
frame and the host batch; a whole-picture window against decode_scaled; windows of two column strips
and batches of more rows than CUs; both count kernels; poisoned bytes outside the plan; the verdict
against decode_region's for the covered full-resolution rectangle on mutated streams; damaged frames
inside a batch; the capacity protocol; dhimg -s2 -r / -s4 -r / -r."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol
import scaled_model as sm
import test_gpu_region as tr
import test_gpu_scaled as ts
from himg_amd import build as hb
from scaled_region_rects import rects, up_rect

pytestmark = pytest.mark.gpu

SCALES = (1, 2)


def _crop(img, rect):
    x, y, w, h = rect
    return img[y:y + h, x:x + w]


def _origins(rect, ow, oh, n):
    """An origin per frame around the rectangle's, every one inside ow x oh."""
    x, y, w, h = rect
    return [(min(max(x + (3 * f) % 5 - 2, 0), ow - w), min(max(y + (2 * f) % 5 - 2, 0), oh - h)) if f else (x, y)
            for f in range(n)]


def _device(eng, streams, W, H, Cn, s, origins, w, h, plans=None, check=True):
    """decode_scaled_regions_device over a batch; plans: upload only the ranges of test_gpu_region._keep and
    poison the rest."""
    n = len(streams)
    stride = (max(len(b) for b in streams) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5 if plans else 0, np.uint8)
    for i, b in enumerate(streams):
        if plans:
            for a, e in tr._keep(b, plans[i]):
                buf[i, a:e] = b[a:e]
        else:
            buf[i, :len(b)] = b
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.zeros(n * h * w * Cn + 16, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_scaled_regions_device(d_in, stride, [len(b) for b in streams], n, W, H, Cn, s, origins, w, h, d_out, d_st)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert not out[n * h * w * Cn:].any()   # nothing behind the last frame
    return d_st.cpu().numpy(), out[:n * h * w * Cn].reshape(n, h, w, Cn)


def _gpu_rects(W, H, s):
    """The host test's rectangles (every x mod S and y mod S, single samples, the last ragged tile, the
    whole picture, a full-width row, a full-height column)."""
    return rects(W, H, s)


@pytest.mark.parametrize("kind,w,h,c,ycc,q", ts.PARITY)
def test_parity(kind, w, h, c, ycc, q):
    eng = himg_amd.Engine(0)
    big = w * h > 1920 * 1080
    seeds = [3, 4] if big else [3, 4, 5]
    streams = [ts._stream(kind, w, h, c, ycc, q, seed) for seed in seeds]
    fix = any(ts._needs_fix(b) for b in streams)   # (streams the reference rejects for T2: the fixed mode, not dropped)
    eng.set_option("fix_t2", int(fix))
    traces = []
    ol.oracle().himg_oracle_set_compat_fix(int(fix))
    try:
        for b in streams:
            rc, trc = ol.oracle_decode_trace(b)
            assert rc == 0
            traces.append(trc)
    finally:
        ol.oracle().himg_oracle_set_compat_fix(0)
    n = len(streams)
    for s in SCALES:
        wants = [sm.scaled_from_trace(t_, b, s) for t_, b in zip(traces, streams)]
        ow, oh = himg_amd.scaled_size(w, h, s)
        rl = _gpu_rects(w, h, s)
        for rect in rl:
            got = eng.decode_scaled_region(streams[0], s, *rect)
            assert got.shape == (rect[3], rect[2], c) and np.array_equal(got, _crop(wants[0], rect)), (s, rect, "host")
            org = _origins(rect, ow, oh, n)
            st, out = _device(eng, streams, w, h, c, s, org, rect[2], rect[3])
            assert (st == 0).all(), (s, rect, st)
            for i in range(n):
                assert np.array_equal(out[i], _crop(wants[i], org[i] + rect[2:])), (s, rect, "device", i)
        # the host batch: every rectangle of every stream in one call (windows of many sizes)
        items = [(i, r) for r in (rl[::4] if big else rl) for i in range(n)]
        got = eng.decode_scaled_regions([streams[i] for i, _ in items], s, [r for _, r in items])
        for (i, r), g in zip(items, got):
            assert np.array_equal(g, _crop(wants[i], r)), (s, r, "batch", i)
    eng.close()


def test_whole_picture_is_decode_scaled(engine):
    for kind, w, h, c, ycc, q in [("randtile", 1000, 72, 4, True, 50), ("gradn", 517, 61, 3, True, 90),
                                  ("rand", 203, 45, 1, False, 50)]:
        b = ts._stream(kind, w, h, c, ycc, q)
        for s in SCALES:
            ow, oh = himg_amd.scaled_size(w, h, s)
            want = engine.decode_scaled(b, s).copy()
            assert np.array_equal(engine.decode_scaled_region(b, s, 0, 0, ow, oh), want)
            st, out = _device(engine, [b, b], w, h, c, s, [(0, 0), (0, 0)], ow, oh)
            st2, out2 = ts._device(engine, [b, b], w, h, c, s)
            assert np.array_equal(st, st2) and (st == 0).all() and np.array_equal(out, out2)
            assert np.array_equal(out[0], want)
    # ... and its status: a damaged stream gets decode_scaled's code and message
    bad = b.copy()
    o, sz = sm.find_chunks(bad)["FRES"]
    bad[o + sz - 5] ^= 0x55
    bad[o + sz - 9] ^= 0xff
    for s in SCALES:
        ow, oh = himg_amd.scaled_size(203, 45, s)
        _, code, msg = ts._verdict(lambda: engine.decode_scaled(bad, s))
        _, code2, msg2 = ts._verdict(lambda: engine.decode_scaled_region(bad, s, 0, 0, ow, oh))
        assert (code, msg) == (code2, msg2)


def _strip_tiles(Cn, s):
    """scaled_strip_tiles (kernels_dec.hip): the widest column strip of the LDS layout, C x S * S segments
    of 4-byte-rounded tiles + 8 beside 27600 bytes of tables and state (test_gpu_region.py's figure for
    the region layout, which has the same fixed part)."""
    nseg = (16 if s == 1 else 4) * Cn
    return ((160 * 1024 - 1024 - 27600) // nseg & ~3) - 8


@pytest.mark.parametrize("s", SCALES)
def test_window_of_two_strips(engine, s):
    """A frame wider than one strip holds (three block rows high): windows of two strips, aligned and not."""
    S = 8 >> s
    tiles = _strip_tiles(4, s)
    W, H = 8 * (tiles + 37) + 3, 21
    b = ts._stream("rand", W, H, 4, True, 50)   # (noise: randtile this flat is trap T2, which the reference rejects)
    rc, want = sm.expected(b, s)
    assert rc == 0
    ow, oh = himg_amd.scaled_size(W, H, s)
    assert ow > S * tiles
    for rect in [(0, 0, ow, oh), (1, 1, ow - 1, oh - 2), (S * 3 + 1, 2, S * tiles + 2, 3), (ow - S * tiles - 5, 0, S * tiles + 5, oh)]:
        assert (rect[0] + rect[2] + S - 1) // S - rect[0] // S > tiles   # more tiles than a strip holds
        assert np.array_equal(engine.decode_scaled_region(b, s, *rect), _crop(want, rect)), (s, rect)
        org = [rect[:2], (0, 0)]
        st, out = _device(engine, [b, b], W, H, 4, s, org, rect[2], rect[3])
        assert (st == 0).all()
        for i in range(2):
            assert np.array_equal(out[i], _crop(want, org[i] + rect[2:])), (s, rect, i)


def test_batch_more_rows_than_cus(engine):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    W, H = 512, 512
    streams = [ts._stream("randtile", W, H, 4, True, 50, seed=k) for k in range(6)]
    for s in SCALES:
        S = 8 >> s
        wants = [sm.expected(b, s)[1] for b in streams]
        ow, oh = himg_amd.scaled_size(W, H, s)
        for rect in [(0, 0, ow, oh), (ow // 10, 3, ow // 2 + 3, oh - 9), (7, oh // 3, 9, 1)]:
            rows = (rect[1] + rect[3] + S - 1) // S - rect[1] // S
            n = 2 * n_cu // max(1, rows) + 1
            batch = [streams[i % 6] for i in range(n)]
            org = _origins(rect, ow, oh, n)
            st, out = _device(engine, batch, W, H, 4, s, org, rect[2], rect[3])
            assert (st == 0).all()
            assert sum((o[1] + rect[3] + S - 1) // S - o[1] // S for o in org) > n_cu
            for i in range(n):
                assert np.array_equal(out[i], _crop(wants[i % 6], org[i] + rect[2:])), (s, rect, i)


@pytest.mark.parametrize("wave", [0, 1])
def test_count_kernel_forms(wave):
    eng = himg_amd.Engine(0)
    eng.set_option("count_wave", wave)
    for kind, w, h, c, ycc, q in [("randtile", 1920, 40, 4, True, 50), ("rand", 8200, 40, 4, True, 50),
                                  ("gradn", 101, 37, 3, True, 90)]:
        b = ts._stream(kind, w, h, c, ycc, q, seed=1)
        for s in SCALES:
            want = sm.expected(b, s)[1]
            ow, oh = himg_amd.scaled_size(w, h, s)
            for rect in _gpu_rects(w, h, s)[::5]:
                assert np.array_equal(eng.decode_scaled_region(b, s, *rect), _crop(want, rect)), (wave, kind, s, rect)
                org = _origins(rect, ow, oh, 2)
                st, out = _device(eng, [b, b], w, h, c, s, org, rect[2], rect[3])
                assert (st == 0).all()
                for i in range(2):
                    assert np.array_equal(out[i], _crop(want, org[i] + rect[2:])), (wave, kind, s, rect, i)
    eng.close()


def test_planned_bytes_only_and_poison(engine):
    """Every byte outside the plan's two ranges and the size headers of rows 0 .. r1-1 (each widened by 4
    bytes) poisoned: output and status unchanged, on a narrow, a ragged and a 16384-pixel-wide stream."""
    for kind, W, H, Cn in [("randtile", 1920, 64, 4), ("rand", 16384, 40, 4), ("gradn", 101, 37, 3)]:
        b = tr._stream(kind, W, H, Cn, 90 if kind == "gradn" else 50)
        for s in SCALES:
            want = sm.expected(b, s)[1]
            for rect in _gpu_rects(W, H, s)[::6]:
                p = himg_amd.scaled_region_peek(b, s, *rect)
                clean = engine.decode_scaled_region(b, s, *rect).copy()
                assert np.array_equal(clean, _crop(want, rect)), (kind, s, rect)
                st0, out0 = _device(engine, [b], W, H, Cn, s, [rect[:2]], rect[2], rect[3])
                st, out = _device(engine, [b], W, H, Cn, s, [rect[:2]], rect[2], rect[3], plans=[p])
                assert st[0] == 0 and st0[0] == 0 and np.array_equal(out, out0) and np.array_equal(out[0], clean), (kind, s, rect)
                d = np.full_like(b, 0xA5)
                for a, e in tr._keep(b, p):
                    d[a:e] = b[a:e]
                assert np.array_equal(engine.decode_scaled_region(d, s, *rect), clean), (kind, s, rect)


def _peek(b):
    w_, h_, c_ = C.c_int(), C.c_int(), C.c_int()
    rc = himg_amd.lib().himg_hip_peek(b.ctypes.data, b.nbytes, C.byref(w_), C.byref(h_), C.byref(c_))
    return (w_.value, h_.value, c_.value) if rc == 0 else None


def _repaired(good, bad, p, fix):
    """`good` with the bytes the window's decode uses taken from `bad`: the head, the size headers of rows
    0 .. r1-1 (at good's offsets) and the plan's rows.  What the rest of `bad` holds is what the window's
    verdict does not look at."""
    offs, lens = himg_amd.index_host(good, fix)[3:5]
    d = good.copy()
    d[:p["head_bytes"]] = bad[:p["head_bytes"]]
    d[p["rows_begin"]:p["rows_end"]] = bad[p["rows_begin"]:p["rows_end"]]
    for r in range(p["row1"]):
        a = int(offs[r]) - (4 if lens[r] >= 0x8000 else 2)
        d[a:int(offs[r])] = bad[a:int(offs[r])]
    return d


@pytest.mark.parametrize("fix", [0, 1])
def test_verdict_fuzz(fix):
    """1000 mutated streams (test_gpu_region.py's mutator and base streams, the same mutation stream; the
    rectangles from a generator of their own: every third the whole picture, the others random, scales
    alternating).  On every mutant code and message equal decode_region's for the covered rectangle;
    where it accepts, the bytes are the crop of decode_scaled's -- of the mutant where decode_scaled
    accepts it, else of the mutant with the bytes the window does not use repaired from the base stream.
    A mutant neither way gives a whole picture for (its head is damaged -- the FRES tree -- so that the
    window's rows still decode and the base stream's other rows do not) has no picture to crop: there the
    host call's bytes must equal the device batch's (the device header walk instead of the host index);
    these are counted apart and not among the accepted ones the test requires.
    On an MI355X: without the fix 233 accepted (111 of them checked against a repaired stream, none without
    a picture) and 767 rejected; with it 553 (106, 1) and 447; no mutation made a rectangle invalid."""
    eng = himg_amd.Engine(0)
    eng.set_option("fix_t2", fix)
    rng = np.random.default_rng(7 + fix)
    rrng = np.random.default_rng(1007 + fix)
    bases = [tr._stream("randtile", 96, 48, 4, 50, True), tr._stream("gradn", 61, 27, 3, 90, True),
             tr._stream("rand", 64, 8, 1, 50, False), tr._stream("grad", 40, 40, 4, 0, True)]
    n_acc = n_rej = n_arg = n_repaired = n_alone = 0
    for t in range(1000):
        good = bases[t % len(bases)]
        W, H = int.from_bytes(good[21:25].tobytes(), "little"), int.from_bytes(good[25:29].tobytes(), "little")   # FRMT
        bad = tr._mutate(good, rng)
        s = 1 + t % 2
        F = 1 << s
        ow, oh = himg_amd.scaled_size(W, H, s)
        if t % 3 == 0:
            rect = (0, 0, ow, oh)
        else:
            x, y = int(rrng.integers(0, ow)), int(rrng.integers(0, oh))
            rect = (x, y, int(rrng.integers(1, ow - x + 1)), int(rrng.integers(1, oh - y + 1)))
        # the covered rectangle in the mutant's own geometry; where FRMT no longer holds the window, the
        # unclipped one (which it does not hold either)
        geom = _peek(bad)
        inside = False
        if geom is not None and geom[0] > 0 and geom[1] > 0:
            ow2, oh2 = himg_amd.scaled_size(geom[0], geom[1], s)
            inside = rect[0] + rect[2] <= ow2 and rect[1] + rect[3] <= oh2
        up = up_rect(geom[0], geom[1], s, rect) if inside else tuple(F * v for v in rect)
        want_r, rcode, rmsg = ts._verdict(lambda: eng.decode_region(bad, *up))
        got, code, msg = ts._verdict(lambda: eng.decode_scaled_region(bad, s, *rect))
        assert (code, msg) == (rcode, rmsg), (t, s, rect, up, code, rcode, msg, rmsg)
        if code == himg_amd.HIMG_ERR_ARG:
            assert not np.array_equal(bad[12:31], good[12:31]), (t, rect)   # only a mutated FRMT chunk
            n_arg += 1
            continue
        if code != 0:
            n_rej += 1
            continue
        n_acc += 1
        full, fcode, _ = ts._verdict(lambda: eng.decode_scaled(bad, s))
        if fcode != 0:   # damage the window does not look at
            p = himg_amd.scaled_region_peek(bad, s, *rect, fix_t2=bool(fix))
            full, fcode, fmsg = ts._verdict(lambda: eng.decode_scaled(_repaired(good, bad, p, bool(fix)), s))
            if fcode != 0:
                st, out = _device(eng, [bad], geom[0], geom[1], geom[2], s, [rect[:2]], rect[2], rect[3])
                assert st[0] == 0 and np.array_equal(out[0], got), (t, s, rect, fcode, fmsg)
                n_alone += 1
                continue
            n_repaired += 1
        assert np.array_equal(got, _crop(full, rect)), (t, s, rect)
    print("accepted %d (of them %d against a repaired stream, %d with no picture to crop), rejected %d, bad rectangle %d"
          % (n_acc, n_repaired, n_alone, n_rej, n_arg))
    assert n_acc + n_rej + n_arg == 1000
    assert n_acc - n_alone > 50 and n_rej > 50, (n_acc, n_alone, n_rej)
    eng.close()


def test_damaged_frames_in_a_batch():
    """A damaged frame in a device batch and in a host batch changes neither status nor bytes of the others."""
    eng = himg_amd.Engine(0)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = n_cu + 17
    w, h, c = 264, 40, 4
    streams = [ts._stream("randtile", w, h, 4, True, 50, seed=i) for i in range(8)]
    rng = np.random.default_rng(9)
    for s in SCALES:
        ow, oh = himg_amd.scaled_size(w, h, s)
        rect = (3, 1, ow - 7, oh - 2)
        wants = [sm.expected(b, s)[1] for b in streams]
        frames = [streams[i % 8] for i in range(n)]
        org = _origins(rect, ow, oh, n)
        st0, out0 = _device(eng, frames, w, h, c, s, org, rect[2], rect[3])
        assert (st0 == 0).all()
        ch = sm.find_chunks(frames[5])
        bad = {}
        for idx, tag in ((5, "FRES"), (n_cu + 3, "LRES"), (40, "FRES")):
            for _ in range(400):
                cand = frames[idx].copy()
                o, sz = ch[tag]
                i = o + sz // 2 + int(rng.integers(0, sz // 4))
                cand[i] ^= 1 << int(rng.integers(0, 8))
                cand[i + 1] ^= 1 << int(rng.integers(0, 8))
                _, code, _ = ts._verdict(lambda: eng.decode_region(cand, *up_rect(w, h, s, org[idx] + rect[2:])))
                if code != 0:
                    bad[idx] = cand
                    break
            assert idx in bad
        for idx, cand in bad.items():
            frames[idx] = cand
        frames[n - 3] = ts._stream("randtile", w + 8, h, 4, True, 50, seed=1)   # another geometry
        st, out = _device(eng, frames, w, h, c, s, org, rect[2], rect[3])
        for i in range(n):
            if i in bad:
                assert st[i] & 15 == 4, (i, st[i])
            elif i == n - 3:
                assert st[i] & 15 == 1, st[i]
            else:
                assert st[i] == 0 and np.array_equal(out[i], _crop(wants[i % 8], org[i] + rect[2:])), (s, i)
                assert np.array_equal(out[i], out0[i]), (s, i)
        # the host batch: the damaged frames fail, the others' bytes are the clean run's
        sub = list(range(0, 48))
        rl = [org[i] + rect[2:] for i in sub]
        L = himg_amd.lib()
        m = len(sub)
        outs = [np.zeros(rect[2] * rect[3] * c, np.uint8) for _ in sub]
        src = (C.c_void_p * m)(*[frames[i].ctypes.data for i in sub])
        szs = (C.c_size_t * m)(*[frames[i].nbytes for i in sub])
        dst = (C.c_void_p * m)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * m)(*[o.nbytes for o in outs])
        ws, hs, cs = (C.c_int * m)(), (C.c_int * m)(), (C.c_int * m)()
        ra = np.ascontiguousarray(np.asarray(rl, np.int32))
        rc = L.himg_hip_decode_scaled_regions_batch(eng._ctx, src, szs, m, s, ra.ctypes.data, dst, caps, ws, hs, cs)
        assert rc == himg_amd.HIMG_ERR_FORMAT
        for k, i in enumerate(sub):
            if i in bad:
                assert (ws[k], hs[k], cs[k]) == (0, 0, 0), i
            else:
                assert (ws[k], hs[k], cs[k]) == (rect[2], rect[3], c), i
                assert np.array_equal(outs[k].reshape(rect[3], rect[2], c), out0[i]), (s, i)
    eng.close()


def test_batch_mixed_geometries(engine):
    items = [("randtile", 264, 40, 4, True), ("gradn", 517, 61, 3, True), ("randtile", 264, 40, 4, True),
             ("rand", 100, 20, 1, False), ("gradn", 517, 61, 3, True), ("rand", 72, 24, 4, True)]
    streams = [ts._stream(k, w, h, c, y, 50, seed=i) for i, (k, w, h, c, y) in enumerate(items)]
    for s in SCALES:
        rl = []
        for i, (_, w, h, _, _) in enumerate(items):
            r = _gpu_rects(w, h, s)
            rl.append(r[(7 * i + 3) % len(r)] if i != 2 else rl[0])   # frames 0 and 2 share a launch
        got = engine.decode_scaled_regions(streams, s, rl)
        for b, r, g in zip(streams, rl, got):
            assert np.array_equal(g, _crop(sm.expected(b, s)[1], r)), (s, r)
    for bad_scale in (0, 3, -1):
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_scaled_regions(streams[:1], bad_scale, [(0, 0, 1, 1)])
        assert e.value.code == himg_amd.HIMG_ERR_ARG
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_scaled_region(streams[0], bad_scale, 0, 0, 1, 1)
        assert e.value.code == himg_amd.HIMG_ERR_ARG
    # a bad rectangle in a batch fails its own frame only
    ow, oh = himg_amd.scaled_size(264, 40, 1)
    with pytest.raises(himg_amd.HimgError) as e:
        engine.decode_scaled_regions(streams[:1], 1, [(ow - 1, 0, 2, 1)])
    assert e.value.code == himg_amd.HIMG_ERR_ARG


def test_capacity_protocol_and_fetch_last(engine):
    b = ts._stream("randtile", 264, 40, 4, True, 50)
    L = himg_amd.lib()
    for s in SCALES:
        ow, oh = himg_amd.scaled_size(264, 40, s)
        rect = (5, 2, ow - 9, oh - 3)
        want = np.ascontiguousarray(_crop(sm.expected(b, s)[1], rect))
        w_, h_, c_ = C.c_int(), C.c_int(), C.c_int()
        small = np.zeros(want.size - 1, np.uint8)
        for dst, cap in ((None, 0), (small.ctypes.data, small.nbytes)):
            rc = L.himg_hip_decode_scaled_region_to(engine._ctx, b.ctypes.data, b.nbytes, s, *rect, dst, cap, C.byref(w_),
                                                    C.byref(h_), C.byref(c_))
            assert rc == himg_amd.HIMG_ERR_CAPACITY and (w_.value, h_.value, c_.value) == (rect[2], rect[3], 4)
            out, n = np.zeros(want.size, np.uint8), C.c_size_t()
            assert L.himg_hip_fetch_last(engine._ctx, out.ctypes.data, out.nbytes, C.byref(n)) == 0
            assert n.value == want.size and np.array_equal(out.reshape(want.shape), want)
        assert not small.any()
        buf = np.zeros(want.size, np.uint8)   # a reused output buffer
        got = engine.decode_scaled_region(b, s, *rect, out=buf)
        assert np.shares_memory(got, buf) and np.array_equal(got, want)


def test_origin_outside_its_frame_writes_nothing(engine):
    w, h, c = 264, 40, 4
    b = ts._stream("randtile", w, h, 4, True, 50)
    for s in SCALES:
        ow, oh = himg_amd.scaled_size(w, h, s)
        ww, hh = 20, 7
        for org in ([(0, 0), (ow - ww + 1, 0)], [(0, oh - hh + 1), (0, 0)], [(-1, 0), (0, 0)], [(0, 0), (0, -1)]):
            stride = (len(b) + 3 + 255) // 256 * 256
            buf = np.zeros((2, stride), np.uint8)
            buf[:, :len(b)] = b
            d_in = torch.from_numpy(buf).cuda()
            d_out = torch.full((2 * hh * ww * c,), 0x5A, dtype=torch.uint8, device="cuda")
            d_st = torch.full((2,), -99, dtype=torch.int32, device="cuda")
            with pytest.raises(himg_amd.HimgError) as e:
                engine.decode_scaled_regions_device(d_in, stride, [len(b)] * 2, 2, w, h, c, s, org, ww, hh, d_out, d_st)
            assert e.value.code == himg_amd.HIMG_ERR_ARG
            torch.cuda.synchronize()
            assert (d_out.cpu().numpy() == 0x5A).all() and (d_st.cpu().numpy() == -99).all()
    for bad_scale in (0, 3):
        d_in = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_scaled_regions_device(d_in, 1024, [100], 1, 64, 64, 4, bad_scale, [(0, 0)], 1, 1, d_out, d_st)
        assert e.value.code == himg_amd.HIMG_ERR_ARG


@pytest.mark.parametrize("flag,s", [("-s2", 1), ("-s4", 2), (None, 0)])
def test_dhimg_region(tmp_path, engine, flag, s):
    """dhimg [-s2 | -s4] -r x,y,w,h image outfile: the window as the Python call gives it, through the tool's
    own row flip and channel swap."""
    dhimg = hb.build_cli()[1]
    b = ts._stream("randtile", 264, 136, 4, True, 70)
    src, out = str(tmp_path / "a.himg"), str(tmp_path / "a.pam")
    b.tofile(src)
    ow, oh = himg_amd.scaled_size(264, 136, s) if s else (264, 136)
    for rect in [(5, 3, ow - 11, oh - 7), (0, 0, ow, oh), (ow - 1, oh - 1, 1, 1)]:
        args = ([flag] if flag else []) + ["-r", "%d,%d,%d,%d" % rect, src, out]
        r = subprocess.run([dhimg] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == "File size: %d\n" % b.size, (r.stdout, r.stderr)
        want = engine.decode_scaled_region(b, s, *rect) if s else engine.decode_region(b, *rect)
        assert np.array_equal(ts._read_pnm(out), want[::-1, :, [2, 1, 0, 3]]), (flag, rect)
    # a rectangle outside the picture: the library's message, then the tool's
    args = ([flag] if flag else []) + ["-r", "0,0,%d,%d" % (ow + 1, oh), src, out]
    r = subprocess.run([dhimg] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 255 and r.stdout.splitlines()[-2:] == ["bad rectangle", "Unable to decode image."]
    # a malformed rectangle is a bad argument
    args = ([flag] if flag else []) + ["-r", "1,2,3", src, out]
    r = subprocess.run([dhimg] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("Usage: ")
