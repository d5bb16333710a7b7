"""GPU (-m gpu): the decode of a stream prefix -- decode_prefix_device (a batch in HBM, the bytes present
per frame) and decode_prefix (a host slice) against tests/prefix_model.py, byte for byte: the rows that
are whole are the oracle's full decode, the others the low-res plane's picture, d_rows and the status are
the model's walk.  No tolerances."""
import functools

import numpy as np
import pytest
import torch

import assembled_cases as ac
import golden_util as gu
import himg_amd
import oracle_lib as ol
import prefix_model as pm

pytestmark = pytest.mark.gpu

ST_SHORT = 5      # a frame's word in the status array for a prefix below its first row header (HIMG_ERR_CAPACITY)
SENTINEL = 0x5A


@pytest.fixture
def eng(engine):
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)
    yield engine
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)


def _stream(kind, w, h, c=4, q=50, ycbcr=True, seed=0):
    img = himg_amd.synth(kind, seed, w, h)
    if c != img.shape[2]:
        img = np.ascontiguousarray(img[:, :, :c] if c > 1 else img[:, :, 0])
    return np.frombuffer(ol.oracle_encode(img, q, ycbcr), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def _model(kind, w, h, c=4, q=50, ycbcr=True, seed=0, fix=False):
    return pm.Model(_stream(kind, w, h, c, q, ycbcr, seed), fix)


def _prefix(eng, streams, avails, W, H, Cn, tail="junk", stride=None):
    """decode_prefix_device: frame f holds streams[f][:avails[f]]; behind them, up to the stride,
    junk bytes (a pattern, or random ones) or the stream's true tail.  (status, rows, pictures)."""
    n = len(streams)
    stride = stride or (max(max(avails), 4) + 3 + 255) // 256 * 256
    if tail == "random":
        buf = np.random.default_rng(99).integers(0, 256, (n, stride), dtype=np.uint8)
    else:
        buf = np.full((n, stride), 0xA5, np.uint8)
    for i, s in enumerate(streams):
        m = min(len(s), stride) if tail == "true" else avails[i]
        buf[i, :m] = s[:m]
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.full((n * H * W * Cn + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    d_rows = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_prefix_device(d_in, stride, avails, n, W, H, Cn, d_out, d_rows, d_st)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n * H * W * Cn:] == SENTINEL).all()
    return d_st.cpu().numpy(), d_rows.cpu().numpy(), out[:n * H * W * Cn].reshape(n, H, W, Cn)


def _check(models, avails, st, rows, out, what=""):
    """Every frame against its model: pixels, d_rows, status; a frame without a picture is untouched."""
    for f, (m, a) in enumerate(zip(models, avails)):
        code, k, pic = m.expect(a)
        if code == pm.CAPACITY:
            assert st[f] == ST_SHORT and rows[f] == -1, (what, f, a, st[f], rows[f])
            assert (out[f] == SENTINEL).all(), (what, f, a)
        else:
            assert code == 0 and st[f] == 0 and rows[f] == k, (what, f, a, code, st[f], rows[f], k)
            assert np.array_equal(out[f], pic), (what, f, a, k)


def test_every_k_at_a_row_boundary(eng):
    m = _model("randtile", 64, 64)
    ends = m.row_ends()
    assert len(ends) == 9
    avails = sorted({min(max(e + d, 0), m.T) for e in ends for d in (-1, 0, 1, 2, 3)})
    ks = [m.expect(a)[1] for a in avails]
    assert set(ks) == set(range(-1, 9))        # below the head, and every k from 0 to 8
    st, rows, out = _prefix(eng, [m.packed] * len(avails), avails, 64, 64, 4)
    _check([m] * len(avails), avails, st, rows, out)


@pytest.mark.parametrize("W,H", [(4096, 32), (2048, 16), (1920, 24)])
def test_row_kernel_forms(eng, W, H):
    """The 512-, 256- and 240-column rows: cut at every row's end, inside a payload, and whole.  (Frames
    this flat are smaller than a block row's symbols: trap T2, decoded under HIMG_OPT_FIX_T2.)"""
    eng.set_option("fix_t2", 1)
    m = _model("randtile", W, H, fix=True)
    ends = m.row_ends()
    avails = sorted(set(ends + [(a + b) // 2 for a, b in zip(ends, ends[1:])] + [m.T, ends[0] + 1]))
    st, rows, out = _prefix(eng, [m.packed] * len(avails), avails, W, H, 4)
    _check([m] * len(avails), avails, st, rows, out, (W, H))


@pytest.mark.parametrize("wave", [-1, 0, 1])
def test_more_frames_than_cus(eng, wave):
    """256 x 72: nine block rows, a single row in the last group; 300 frames, each with its own avail."""
    eng.set_option("count_wave", wave)
    ms = [_model("randtile", 256, 72, seed=s) for s in range(3)]
    rng = np.random.default_rng(5)
    n = 300 if wave == -1 else 24
    models = [ms[f % 3] for f in range(n)]
    avails = [int(rng.integers(m.plan["head_bytes"], m.T + 1)) for m in models]
    avails[0], avails[1], avails[2] = models[0].plan["head_bytes"], models[1].T, models[2].row_ends()[8]
    avails[3] = models[0].plan["head_bytes"] - 1
    ks = {m.expect(a)[1] for m, a in zip(models, avails)}
    assert {-1, 0, 8, 9} <= ks
    st, rows, out = _prefix(eng, [m.packed for m in models], avails, 256, 72, 4)
    _check(models, avails, st, rows, out, wave)


@pytest.mark.parametrize("W,H,Cn,ycc,fix", [(100, 45, 3, True, False), (37, 19, 1, True, False), (72, 40, 3, False, False),
                                            (40, 8, 4, True, True)])
def test_ragged_shapes_and_few_channels(eng, W, H, Cn, ycc, fix):
    eng.set_option("fix_t2", int(fix))
    m = _model("randtile", W, H, Cn, 90, ycc, 3, fix)
    ends = m.row_ends()
    if m.rows == 1:   # one block row, no size header: whole only with the chunk's last byte
        avails = [m.T - 1, m.T, ends[0]]
        assert [m.expect(a)[1] for a in avails] == [0, 1, 0]
    else:
        avails = sorted(set(ends + [ends[1] + 1, m.T - 1]))
    st, rows, out = _prefix(eng, [m.packed] * len(avails), avails, W, H, Cn)
    _check([m] * len(avails), avails, st, rows, out, (W, H, Cn))


def test_four_byte_headers(eng):
    m = _model("rand", 4096, 16, q=100, seed=7)
    ends = m.row_ends()
    assert ends[1] - ends[0] > 0x8000 + 4 and len(ends) == 3
    avails = [ends[0], ends[0] + 1, ends[0] + 2, ends[0] + 3, ends[0] + 4, (ends[0] + ends[1]) // 2, ends[1] - 1, ends[1],
              ends[1] + 2, ends[1] + 3, ends[1] + 4 + 20000, m.T - 1, m.T]
    st, rows, out = _prefix(eng, [m.packed] * len(avails), avails, 4096, 16, 4)
    _check([m] * len(avails), avails, st, rows, out)
    assert list(rows) == [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2]


def test_bytes_at_or_beyond_avail_do_not_count(eng):
    m = _model("randtile", 256, 72)
    ends = m.row_ends()
    avails = [ends[0], ends[3], ends[3] + 1, (ends[4] + ends[5]) // 2, ends[8] + 2, m.T - 1]
    n = len(avails)
    stride = (m.T + 3 + 255) // 256 * 256
    a = _prefix(eng, [m.packed] * n, avails, 256, 72, 4, tail="random", stride=stride)
    b = _prefix(eng, [m.packed] * n, avails, 256, 72, 4, tail="true", stride=stride)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _check([m] * n, avails, *a)
    # a byte flipped behind the bytes present changes nothing; one inside a complete row that the decoder
    # notices (the oracle says which) fails that frame alone
    flipped = m.packed.copy()
    flipped[avails[3]] ^= 0xff
    bad = None
    for off in range(ends[1] + 6, ends[2], 7):
        t = m.packed.copy()
        t[off] ^= 0x55
        if ol.oracle_decode(t)[0] != 0:
            bad = t
            break
    assert bad is not None
    av = [avails[3]] * 4
    st, rows, out = _prefix(eng, [m.packed, flipped, bad, m.packed], av, 256, 72, 4, tail="true", stride=stride)
    assert st[2] & 15 == 4 and rows[2] == -1
    _check([m] * 3, av[:3], st[[0, 1, 3]], rows[[0, 1, 3]], out[[0, 1, 3]])
    # the damaged row has not arrived whole: not seen
    st, rows, out = _prefix(eng, [bad], [ends[1] + 6], 256, 72, 4, tail="true", stride=stride)
    _check([m], [ends[1] + 6], st, rows, out)


def _full(eng, streams, W, H, Cn):
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.zeros((n, stride), np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = s
    d_out = torch.full((n * H * W * Cn + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_device(torch.from_numpy(buf).cuda(), stride, [len(s) for s in streams], n, W, H, Cn, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy()[:n * H * W * Cn].reshape(n, H, W, Cn)


def _whole_equals_decode(eng, streams, W, H, Cn, what):
    for fix in (0, 1):
        eng.set_option("fix_t2", fix)
        st0, out0 = _full(eng, streams, W, H, Cn)
        st, rows, out = _prefix(eng, streams, [len(s) for s in streams], W, H, Cn)
        assert np.array_equal(st, st0), (what, fix, st, st0)
        for f in range(len(streams)):
            if st0[f] == 0:
                assert rows[f] == (H + 7) // 8 and np.array_equal(out[f], out0[f]), (what, fix, f)
            else:
                assert rows[f] == -1, (what, fix, f)
    return st0


def test_whole_stream_is_decode_device_goldens(eng):
    names = [n for n in gu.cases(max_pixels=64 * 64) if "fixture" in gu.GOLDEN[n] and gu.GOLDEN[n]["channels"] == 4]
    streams = [gu.fixture(gu.GOLDEN[n]) for n in names]
    _whole_equals_decode(eng, streams, 64, 64, 4, names)
    # the grad stream is trap T2: rejected as today without the fix, decoded with it
    g = [gu.fixture(gu.GOLDEN["grad_s0_64x64_q50"])]
    eng.set_option("fix_t2", 0)
    st, rows, _ = _prefix(eng, g, [g[0].size], 64, 64, 4)
    assert st[0] & 15 == 4 and st[0] == _full(eng, g, 64, 64, 4)[0][0] and rows[0] == -1
    eng.set_option("fix_t2", 1)
    st, rows, _ = _prefix(eng, g, [g[0].size], 64, 64, 4)
    assert st[0] == 0 and rows[0] == 8
    for n in ("randtile_s5_64x64_q50_c1", "randtile_s5_64x64_q50_c3"):
        r = gu.GOLDEN[n]
        _whole_equals_decode(eng, [gu.fixture(r)], 64, 64, r["channels"], n)


# The assembled streams (valid streams no encoder writes, and those the reference rejects): every case of
# assembled_cases._list() but the two multi-chunk pictures (1024 x 512 and 2048 x 1024), a launch per shape.
ASSEMBLED_SHAPES = sorted({k[1:] for k in ac._list() if k[1] * k[2] <= 4352 * 16 * 2})


@pytest.mark.parametrize("shape", ASSEMBLED_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_whole_stream_is_decode_device_assembled(eng, shape):
    keys = [k for k in ac._list() if k[1:] == shape]
    streams = [ac.case(*k).stream for k in keys]
    st0 = _whole_equals_decode(eng, streams, *shape, shape)
    if shape == (64, 24, 4):   # the rejected ones are among them
        assert (st0 != 0).any() and (st0 == 0).any()


def test_below_the_head(eng):
    m = _model("randtile", 64, 64)
    head = m.plan["head_bytes"]
    avails = [m.T, head - 1, 0, 11, 12, 100, m.row_ends()[4]]
    st, rows, out = _prefix(eng, [m.packed] * len(avails), avails, 64, 64, 4)
    assert list(st) == [0, ST_SHORT, ST_SHORT, ST_SHORT, ST_SHORT, ST_SHORT, 0]
    assert list(rows) == [8, -1, -1, -1, -1, -1, 4]
    _check([m] * len(avails), avails, st, rows, out)


def test_host_form(eng):
    m = _model("randtile", 100, 45, 3, 90, True, 3)
    ends = m.row_ends()
    for a in (ends[0], ends[2] + 1, m.T - 1, m.T):
        piece = m.packed[:a].copy()                       # exactly the bytes present: nothing behind them exists
        pic, k = eng.decode_prefix(piece)
        code, want_k, want = m.expect(a)
        assert code == 0 and k == want_k and np.array_equal(pic, want), a
    assert np.array_equal(eng.decode_prefix(m.packed)[0], eng.decode(m.packed))
    # the capacity protocol: geometry and k are set, fetch_last copies the resident result
    import ctypes as C
    L = himg_amd.lib()
    piece = m.packed[:ends[3]].copy()
    w, h, c, k = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = L.himg_hip_decode_prefix_to(eng._ctx, piece.ctypes.data, piece.nbytes, None, 0, C.byref(w), C.byref(h),
                                     C.byref(c), C.byref(k))
    assert rc == himg_amd.HIMG_ERR_CAPACITY and (w.value, h.value, c.value, k.value) == (100, 45, 3, 3)
    got = np.zeros(100 * 45 * 3, np.uint8)
    n = C.c_size_t()
    assert L.himg_hip_fetch_last(eng._ctx, got.ctypes.data, got.nbytes, C.byref(n)) == 0 and n.value == got.nbytes
    assert np.array_equal(got.reshape(45, 100, 3), m.picture(3))
    # below the head: HIMG_ERR_CAPACITY with rows_complete = -1
    for a in (0, 20, ends[0] - 1):
        piece = m.packed[:a].copy()
        rc = L.himg_hip_decode_prefix_to(eng._ctx, piece.ctypes.data if a else None, a, got.ctypes.data, got.nbytes,
                                         C.byref(w), C.byref(h), C.byref(c), C.byref(k))
        assert rc == himg_amd.HIMG_ERR_CAPACITY and k.value == -1, a
        with pytest.raises(himg_amd.HimgError) as e:
            eng.decode_prefix(piece)
        assert e.value.code == himg_amd.HIMG_ERR_CAPACITY
    # FRMT's channel count 0: the walk goes on past FRMT, the verdict is the full decode's all the same
    d = m.packed.copy()
    d[29] = 0
    for fn in (eng.decode_prefix, eng.decode):
        with pytest.raises(himg_amd.HimgError) as e:
            fn(d)
        assert e.value.code == himg_amd.HIMG_ERR_UNSUPPORTED and "unsupported geometry" in str(e.value)
    # a damaged head: the full decode's wording
    d = m.packed.copy()
    d[0] = 0x51
    for fn in (eng.decode_prefix, eng.decode):
        with pytest.raises(himg_amd.HimgError) as e:
            fn(d)
        assert e.value.code == himg_amd.HIMG_ERR_FORMAT and "Not a RIFF HIMG file." in str(e.value)
