"""GPU: the region decode with a window per frame -- decode_regions_device (a batch in HBM, an
origin per frame) and decode_regions (host streams, a rectangle each) against the oracle's full
decode, cropped, byte for byte; the one-origin call; both count-kernel forms; per-frame verdicts;
poisoned bytes outside each frame's plan; mutated streams; host-batch failures and multi-launch
groups; argument errors that leave the outputs alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol
from test_gpu_region import _crop, _ends_after_row, _full, _keep, _mutate, _stream

pytestmark = pytest.mark.gpu


def _origins(W, H, w, h, rng, extra=4):
    """Corners, (0, 0), tile-aligned and unaligned origins, x % 8 and y % 8 of both 0 and 7."""
    X, Y = W - w, H - h
    o = [(0, 0), (X, Y), (X, 0), (0, Y)]
    for a, b in [(8, 8), (7, 7), (8, 7), (7, 8), (16, 15), (23, 40), (5, 3)]:
        o.append((min(a, X), min(b, Y)))
    o += [(int(rng.integers(0, X + 1)), int(rng.integers(0, Y + 1))) for _ in range(extra)]
    return np.array(list(dict.fromkeys(o)), np.int32)   # (distinct: a whole-frame window has one origin)


def _upload(streams, plans=None):
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5 if plans else 0, np.uint8)
    for i, s in enumerate(streams):
        if plans:
            for a, e in _keep(s, plans[i]):
                buf[i, a:e] = s[a:e]
        else:
            buf[i, :len(s)] = s
    return torch.from_numpy(buf).cuda(), stride


def _regions(eng, streams, W, H, Cn, origins, w, h, plans=None):
    """decode_regions_device; plans: upload only each frame's _keep ranges and poison the rest."""
    n = len(streams)
    d_in, stride = _upload(streams, plans)
    d_out = torch.full((n * h * w * Cn + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_regions_device(d_in, stride, [len(s) for s in streams], n, W, H, Cn, origins, w, h, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy()[:n * h * w * Cn].reshape(n, h, w, Cn)


def _region_one_origin(eng, streams, W, H, Cn, x, y, w, h):
    n = len(streams)
    d_in, stride = _upload(streams)
    d_out = torch.full((n * h * w * Cn + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_region_device(d_in, stride, [len(s) for s in streams], n, W, H, Cn, x, y, w, h, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy()[:n * h * w * Cn].reshape(n, h, w, Cn)


def _to(eng, s, rect):
    """decode_region_to's verdict: (code, message, pixels)."""
    try:
        return 0, "", eng.decode_region(s, *rect)
    except himg_amd.HimgError as e:
        return e.code, str(e).split(":", 1)[-1].strip(), None


def _batch(eng, streams, rects, caps=None):
    """himg_hip_decode_regions_batch through ctypes: (rc, message, [(w, h, c)], outputs); streams[i] may be None."""
    L = himg_amd.lib()
    n = len(streams)
    rc_ = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(n, 4))
    outs = []
    for i, s in enumerate(streams):
        c = 4 if s is None else int(s[29])   # FRMT's channel byte
        cap = int(rc_[i, 2]) * int(rc_[i, 3]) * c if caps is None or caps[i] is None else caps[i]
        outs.append(np.full(max(cap, 1), 0x3C, np.uint8))
    src = (C.c_void_p * n)(*[None if s is None else s.ctypes.data for s in streams])
    szs = (C.c_size_t * n)(*[0 if s is None else len(s) for s in streams])
    dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    cps = (C.c_size_t * n)(*[(o.nbytes if caps is None or caps[i] is None else caps[i]) for i, o in enumerate(outs)])
    ws, hs, cs = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    rc = L.himg_hip_decode_regions_batch(eng._ctx, src, szs, n, rc_.ctypes.data, dst, cps, ws, hs, cs)
    msg = L.himg_hip_last_error(eng._ctx).decode().strip()
    return rc, msg, [(ws[i], hs[i], cs[i]) for i in range(n)], outs


SHAPES = [  # kind, W, H, C, q, windows (w, h)
    ("randtile", 4096, 4096, 4, 50, [(256, 256), (1, 1), (4096, 4096)]),
    ("randtile", 4096, 4096, 4, 90, [(256, 256), (33, 17)]),
    ("randtile", 1920, 1080, 4, 50, [(1, 1), (300, 200), (1920, 1080)]),
    ("gradn", 1000, 600, 3, 90, [(1, 1), (129, 77), (1000, 600)]),
    ("randtile", 1001, 333, 1, 50, [(1, 1), (100, 50), (1001, 333)]),
    ("randtile", 8192, 64, 4, 50, [(5000, 9), (4161, 64), (8192, 64)]),   # windows of two column strips
]


def _streams_for(eng, kind, W, H, Cn, q, seeds):
    out = []
    for s in seeds:
        img = himg_amd.synth(kind, s, W, H)
        if Cn != 4:
            img = np.ascontiguousarray(img[:, :, :Cn])
        b = eng.encode(img, q, True) if W * H >= 4096 * 4096 else np.frombuffer(ol.oracle_encode(img, q, True), np.uint8).copy()
        out.append(b)
    return out


@pytest.mark.parametrize("kind,W,H,Cn,q,wins", SHAPES)
def test_parity_per_frame_origins(engine, kind, W, H, Cn, q, wins):
    rng = np.random.default_rng(W + H + q)
    streams = _streams_for(engine, kind, W, H, Cn, q, [0] if W * H >= 4096 * 4096 else [0, 1])
    fulls = [_full(s) for s in streams]
    for w, h in wins:
        org = _origins(W, H, w, h, rng)
        batch = [streams[i % len(streams)] for i in range(len(org))]
        st, out = _regions(engine, batch, W, H, Cn, org, w, h)
        assert (st == 0).all(), (w, h, st)
        for f, (x, y) in enumerate(org):
            assert np.array_equal(out[f], _crop(fulls[f % len(streams)], (x, y, w, h))), (kind, W, H, w, h, x, y)
        # every origin the same: the one-origin call's bytes and statuses
        x, y = (int(v) for v in org[-1])
        k = min(3, len(batch))
        st1, out1 = _region_one_origin(engine, batch[:k], W, H, Cn, x, y, w, h)
        stn, outn = _regions(engine, batch[:k], W, H, Cn, np.array([[x, y]] * k, np.int32), w, h)
        assert np.array_equal(st1, stn) and np.array_equal(out1, outn), (w, h, x, y)


@pytest.mark.parametrize("wave", [0, 1, -1])
def test_count_kernel_forms(wave):
    eng = himg_amd.Engine(0)
    eng.set_option("count_wave", wave)
    rng = np.random.default_rng(11)
    if wave >= 0:
        W, H, Cn = 1920, 64, 4
        streams = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(2)] + [_stream("rand", W, H, Cn, 90, True)]
        w, h = 700, 23
    else:
        # more than 8192 touched rows: k_region_count_w by rule
        W, H, Cn = 1920, 1080, 4
        streams = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(2)]
        w, h = 64, 1073
    fulls = [_full(s) for s in streams]
    n = 64 if wave < 0 else 12
    org = np.array([(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))) for _ in range(n)], np.int32)
    batch = [streams[i % len(streams)] for i in range(n)]
    if wave < 0:
        assert sum((y + h + 7) // 8 - y // 8 for _, y in org) > 8192
    eng.profile(True)
    eng.profile_reset()
    st, out = _regions(eng, batch, W, H, Cn, org, w, h)
    stages = eng.profile_read()
    eng.profile(False)
    assert (st == 0).all(), st
    assert ("k_region_count_w" in stages) == (wave != 0), stages.keys()
    for f, (x, y) in enumerate(org):
        assert np.array_equal(out[f], _crop(fulls[f % len(streams)], (x, y, w, h))), (wave, f, x, y)
    eng.close()


def _damage_header(b, r):
    """b with the size header of block row r made to overrun the chunk."""
    offs = himg_amd.index_host(b)[3]
    d = b.copy()
    hdr = int(offs[r]) - 2
    d[hdr], d[hdr + 1] = 0xFF, 0x7F
    return d


def _damage_inside(eng, b, rect, rng):
    """b with bytes of the rectangle's first row payload flipped until decode_region_to rejects it."""
    offs, lens = himg_amd.index_host(b)[3:5]
    r0 = rect[1] // 8
    for _ in range(200):
        d = b.copy()
        for _ in range(4):
            i = int(offs[r0]) + int(rng.integers(0, int(lens[r0])))
            d[i] ^= 1 << int(rng.integers(0, 8))
        if _to(eng, d, rect)[0] == himg_amd.HIMG_ERR_FORMAT:
            return d
    raise AssertionError("no rejected mutation found")


def test_per_frame_verdicts(engine):
    W, H, Cn = 256, 96, 4
    rng = np.random.default_rng(5)
    good = [_stream("randtile", W, H, Cn, 50, True, seed=s) for s in range(3)]
    fulls = [_full(s) for s in good]
    w, h = 40, 20
    below = _damage_header(good[0], 9)            # rows 9.. are below a window on rows 1..3
    inside = _damage_inside(engine, good[1], (30, 11, w, h), rng)
    cut = _ends_after_row(good[2], 6)              # chunk ends right behind row 5
    frames = [(good[0], (3, 9)), (below, (17, 12)), (good[1], (60, 76)), (inside, (30, 11)), (good[2], (200, 70)),
              (cut, (5, 27)), (cut, (9, 30)), (good[0], (W - w, H - h)), (good[2], (0, 0))]
    streams = [s for s, _ in frames]
    org = np.array([o for _, o in frames], np.int32)
    st, out = _regions(engine, streams, W, H, Cn, org, w, h)
    intact_src = {0: 0, 2: 1, 4: 2, 7: 0, 8: 2}
    for f, (s, (x, y)) in enumerate(frames):
        code, msg, px = _to(engine, s, (x, y, w, h))
        assert (st[f] != 0) == (code != 0), (f, st[f], code)
        st1, out1 = _regions(engine, [s], W, H, Cn, org[f:f + 1], w, h)   # the frame alone
        assert st1[0] == st[f], (f, st1, st[f])
        if code == 0:
            assert np.array_equal(out[f], px) and np.array_equal(out[f], out1[0]), f
        if f in intact_src:
            assert np.array_equal(out[f], _crop(fulls[intact_src[f]], (x, y, w, h))), f
    assert st[1] == 0 and st[3] != 0 and st[5] == 0 and st[6] != 0
    # the host batch: each frame's verdict and wording is decode_region_to's
    rects = [(x, y, w, h) for _, (x, y) in frames]
    rc, _, dims, outs = _batch(engine, streams, rects)
    assert rc == himg_amd.HIMG_ERR_FORMAT
    for f, (s, rect) in enumerate(zip(streams, rects)):
        code, msg, px = _to(engine, s, rect)
        rc1, msg1, dims1, outs1 = _batch(engine, [s], [rect])
        assert rc1 == code and (code == 0 or msg1 == msg), (f, rc1, code, msg1, msg)
        assert (dims[f] == (0, 0, 0)) == (code != 0), (f, dims[f])
        if code == 0:
            assert np.array_equal(outs[f].reshape(px.shape), px), f


def test_poisoned_bytes_outside_each_plan(engine):
    for kind, W, H, Cn, w, h in [("randtile", 1920, 64, 4, 333, 17), ("gradn", 101, 37, 3, 9, 30), ("rand", 4096, 48, 4, 1, 1)]:
        rng = np.random.default_rng(W)
        streams = [_stream(kind, W, H, Cn, 90 if kind == "gradn" else 50, True, seed=s) for s in range(2)]
        org = _origins(W, H, w, h, rng)
        batch = [streams[i % 2] for i in range(len(org))]
        plans = [himg_amd.region_peek(s, int(x), int(y), w, h) for s, (x, y) in zip(batch, org)]
        st0, out0 = _regions(engine, batch, W, H, Cn, org, w, h)
        st1, out1 = _regions(engine, batch, W, H, Cn, org, w, h, plans=plans)
        assert (st0 == 0).all() and np.array_equal(st0, st1) and np.array_equal(out0, out1), kind
        # the host batch with the caller's bytes outside each frame's plan poisoned
        poisoned = []
        for s, p in zip(batch, plans):
            d = np.full_like(s, 0xA5)
            for a, e in _keep(s, p):
                d[a:e] = s[a:e]
            poisoned.append(d)
        rects = [(int(x), int(y), w, h) for x, y in org]
        rc, _, _, outs = _batch(engine, poisoned, rects)
        assert rc == 0
        for f in range(len(batch)):
            assert np.array_equal(outs[f].reshape(h, w, Cn), out0[f]), (kind, f)


def test_mutation_fuzz():
    eng = himg_amd.Engine(0)
    rng = np.random.default_rng(2024)
    bases = [("randtile", 96, 48, 4, 50), ("gradn", 61, 27, 3, 90), ("rand", 64, 16, 1, 50), ("randtile", 200, 40, 4, 90)]
    n_acc = n_rej = 0
    for kind, W, H, Cn, q in bases:
        good = _stream(kind, W, H, Cn, q, True)
        for _ in range(5):
            n = 52
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            bad = [_mutate(good, rng) for _ in range(n)]
            org = np.array([(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))) for _ in range(n)], np.int32)
            st, out = _regions(eng, bad, W, H, Cn, org, w, h)
            rects = [(int(x), int(y), w, h) for x, y in org]
            rc, _, dims, outs = _batch(eng, bad, rects)
            for f in range(n):
                code, _, px = _to(eng, bad[f], rects[f])
                if code == himg_amd.HIMG_ERR_ARG:   # a mutated FRMT no longer holds the rectangle
                    assert dims[f] == (0, 0, 0)
                    continue
                assert (dims[f] == (0, 0, 0)) == (code != 0), (kind, f, dims[f], code)
                if code == 0:
                    assert np.array_equal(outs[f].reshape(px.shape), px), (kind, f)
                if not np.array_equal(bad[f][12:31], good[12:31]):
                    continue   # (the device entry decodes the caller's geometry, not the stream's)
                assert (st[f] != 0) == (code != 0), (kind, f, st[f], code)
                if code == 0:
                    assert np.array_equal(out[f], px), (kind, f)
                    n_acc += 1
                else:
                    n_rej += 1
    assert n_acc + n_rej >= 1000 - 100 and n_acc > 50 and n_rej > 50
    eng.close()


def test_host_batch(engine):
    specs = [("randtile", 256, 96, 4, 50, (3, 5, 40, 20)), ("gradn", 101, 37, 3, 90, (7, 1, 60, 30)),
             ("randtile", 256, 96, 4, 50, (100, 70, 40, 20)), ("rand", 64, 16, 1, 50, (0, 0, 64, 16)),
             ("randtile", 256, 96, 4, 90, (8, 8, 17, 3)), ("gradn", 101, 37, 3, 90, (0, 30, 60, 7)),
             ("randtile", 256, 96, 4, 50, (216, 76, 40, 20))]
    streams = [_stream(k, W, H, Cn, q, True, seed=i) for i, (k, W, H, Cn, q, _) in enumerate(specs)]
    rects = [r for *_, r in specs]
    want = [_crop(_full(s), r) for s, r in zip(streams, rects)]
    rc, msg, dims, outs = _batch(engine, streams, rects)
    assert rc == 0, msg
    for i, r in enumerate(rects):
        assert dims[i] == (r[2], r[3], want[i].shape[2]) and np.array_equal(outs[i].reshape(want[i].shape), want[i]), i
    got = engine.decode_regions(streams, rects)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # a bad rectangle, a too-small dst, a NULL stream: only that frame fails, with its own code
    for bad, code in [("rect", himg_amd.HIMG_ERR_ARG), ("cap", himg_amd.HIMG_ERR_CAPACITY), ("null", himg_amd.HIMG_ERR_FORMAT)]:
        s2, r2, caps = list(streams), list(rects), [None] * len(streams)
        if bad == "rect":
            r2[2] = (250, 70, 40, 20)
        elif bad == "cap":
            caps[2] = 40 * 20 * 4 - 1
        else:
            s2[2] = None
        rc, msg, dims, outs = _batch(engine, s2, r2, caps)
        assert rc == code, (bad, rc, msg)
        for i in range(len(specs)):
            if i == 2:
                assert dims[i] == (0, 0, 0), bad
            else:
                assert np.array_equal(outs[i].reshape(want[i].shape), want[i]), (bad, i)
    # more than 256 frames of one group: several launches
    W, H = 64, 40
    base = [_stream("randtile", W, H, 4, 50, True, seed=s) for s in range(3)]
    bf = [_full(s) for s in base]
    rng = np.random.default_rng(3)
    n = 300
    rects = [(int(rng.integers(0, W - 13)), int(rng.integers(0, H - 9)), 13, 9) for _ in range(n)]
    got = engine.decode_regions([base[i % 3] for i in range(n)], rects)
    for i in range(n):
        assert np.array_equal(got[i], _crop(bf[i % 3], rects[i])), i


def test_device_argument_errors(engine):
    W, H, Cn = 96, 48, 4
    b = _stream("randtile", W, H, Cn, 50, True)
    d_in, stride = _upload([b, b])
    for org, w, h in [([(0, 0), (57, 0)], 40, 8), ([(0, 0), (-1, 0)], 4, 4), ([(0, 41), (0, 0)], 4, 8), ([(0, 0), (0, 0)], 0, 4)]:
        d_out = torch.full((2 * max(w, 1) * h * Cn + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.full((2,), -99, dtype=torch.int32, device="cuda")
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_regions_device(d_in, stride, [len(b)] * 2, 2, W, H, Cn, np.array(org, np.int32), w, h, d_out, d_st)
        assert e.value.code == himg_amd.HIMG_ERR_ARG
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x5A).all() and (d_st.cpu().numpy() == -99).all(), org
