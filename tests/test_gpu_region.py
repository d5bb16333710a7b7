"""GPU: the region decode against the oracle's full decode, cropped, byte for byte -- through
decode_region (host stream), decode_region_device (batch in HBM) and region_peek followed by an
upload of only the planned bytes; both count-kernel forms; poisoned bytes outside the plan; and
mutated streams (the run returns every time; accepted streams match the crop; a whole-frame
rectangle gets the full decode's verdict)."""
import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _stream(kind, w, h, c=4, q=50, ycbcr=True, seed=0):
    img = himg_amd.synth(kind, seed, w, h)
    if c != img.shape[2]:
        img = np.ascontiguousarray(img[:, :, :c])
    return np.frombuffer(ol.oracle_encode(img, q, ycbcr), np.uint8).copy()


def _full(b, fix=False):
    rc, img = ol.oracle_decode(b, fix_t2=fix)
    assert rc == 0
    return img


def _rects(W, H, strip=None):
    r = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]
    r += [(min(8, W - 8), 0, min(8, W), min(8, H)), (min(3, W - 1), min(2, H - 1), 1, 1)]        # aligned; inside one tile
    r += [(min(5, W - 1), min(3, H - 1), max(1, min(W - 6, W // 2)), max(1, min(H - 4, H // 2)))]  # unaligned x, y, w, h
    if W > 9 and H > 9:
        r += [(7, 7, 2, 2), (W - 9, H - 9, 9, 9), (W // 2 - 1, 1, W // 2, H - 2)]                 # crossing tile edges
    if strip is not None:
        for tw in (strip, strip + 1):
            if 8 * tw <= W:
                r += [(0, 1, 8 * tw, 9), (W - 8 * tw - 3, 5, 8 * tw + 1, 3), (4, 0, 8 * tw, 2)]
    return [t for t in r if t[0] + t[2] <= W and t[1] + t[3] <= H]


def _crop(img, rect):
    x, y, w, h = rect
    return img[y:y + h, x:x + w]


def _keep(s, p, pad=4):
    """The byte ranges the region decode may read: [0, head), the size header of every row
    0 .. row1-1, [rows_begin, rows_end), each widened by `pad` bytes."""
    offs, lens = himg_amd.index_host(s)[3:5]
    out = [(0, p["head_bytes"] + pad), (max(0, p["rows_begin"] - pad), p["rows_end"] + pad)]
    for r in range(p["row1"]):
        hdr = 4 if lens[r] >= 0x8000 else 2
        out.append((int(offs[r]) - hdr - pad, int(offs[r]) + pad))
    return [(a, min(e, len(s))) for a, e in out]


def _device(eng, streams, W, H, Cn, rect, plans=None):
    """decode_region_device over a batch; plans: upload only the ranges of _keep and poison the rest."""
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5 if plans else 0, np.uint8)
    for i, s in enumerate(streams):
        if plans:
            for a, e in _keep(s, plans[i]):
                buf[i, a:e] = s[a:e]
        else:
            buf[i, :len(s)] = s
    x, y, w, h = rect
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.zeros(n * h * w * Cn + 16, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_region_device(d_in, stride, [len(s) for s in streams], n, W, H, Cn, x, y, w, h, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy()[:n * h * w * Cn].reshape(n, h, w, Cn)


SHAPES = [  # kind, W, H, C, q, ycbcr
    ("randtile", 1920, 40, 4, 50, True), ("rand", 4096, 40, 4, 90, True), ("randtile", 4352, 40, 3, 100, False), ("grad", 4352, 40, 3, 90, False),
    ("gradn", 4360, 40, 4, 10, True), ("randtile", 16384, 40, 4, 50, True), ("randtile", 101, 37, 1, 50, True),
    ("gradn", 61, 19, 2, 90, False), ("rand", 203, 45, 3, 50, True), ("randtile", 16384, 40, 2, 100, False),
]


@pytest.mark.parametrize("kind,W,H,Cn,q,ycc", SHAPES)
def test_parity_host_and_device(engine, kind, W, H, Cn, q, ycc):
    b = _stream(kind, W, H, Cn, q, ycc)
    fix = ol.oracle_decode(b)[0] != 0   # (a flat stream the reference rejects: the fixed mode, HIMG_OPT_FIX_T2)
    engine.set_option("fix_t2", int(fix))
    full = _full(b, fix)
    strip = None
    if W >= 4096:
        # the widest strip of the LDS layout (region_strip_tiles): C x 64 segments of 4-byte-rounded tiles + 8
        # beside 27600 bytes of tables and state
        strip = ((160 * 1024 - 1024 - 27600) // (64 * Cn) & ~3) - 8
    for rect in _rects(W, H, strip):
        got = engine.decode_region(b, *rect)
        assert np.array_equal(got, _crop(full, rect)), (kind, W, H, Cn, rect)
    for rect in _rects(W, H)[:6]:
        st, out = _device(engine, [b, b], W, H, Cn, rect)
        assert (st == 0).all(), (rect, st)
        assert np.array_equal(out[0], _crop(full, rect)) and np.array_equal(out[1], _crop(full, rect)), rect
    engine.set_option("fix_t2", 0)


@pytest.mark.parametrize("wave", [0, 1])
def test_count_kernel_forms(wave):
    eng = himg_amd.Engine(0)
    eng.set_option("count_wave", wave)
    for kind, W, H, Cn, q, ycc in [("randtile", 1920, 40, 4, 50, True), ("rand", 16384, 40, 4, 50, True),
                                   ("gradn", 101, 37, 3, 90, True)]:
        b = _stream(kind, W, H, Cn, q, ycc, seed=1)
        full = _full(b)
        for rect in _rects(W, H)[:8]:
            assert np.array_equal(eng.decode_region(b, *rect), _crop(full, rect)), (wave, kind, rect)
            st, out = _device(eng, [b], W, H, Cn, rect)
            assert st[0] == 0 and np.array_equal(out[0], _crop(full, rect)), (wave, kind, rect)


def test_batch_more_rows_than_cus(engine):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    W, H = 512, 512
    streams = [_stream("randtile", W, H, 4, 50, True, seed=s) for s in range(6)]
    fulls = [_full(s) for s in streams]
    for rect in [(0, 0, W, H), (101, 3, 300, 500), (7, 250, 9, 1)]:
        n = 2 * n_cu // max(1, (rect[1] + rect[3] + 7) // 8 - rect[1] // 8) + 1
        batch = [streams[i % 6] for i in range(n)]
        st, out = _device(engine, batch, W, H, 4, rect)
        assert (st == 0).all()
        for i in range(n):
            assert np.array_equal(out[i], _crop(fulls[i % 6], rect)), (rect, i)


def test_planned_bytes_only_and_poison(engine):
    for kind, W, H, Cn in [("randtile", 1920, 64, 4), ("rand", 16384, 40, 4), ("gradn", 101, 37, 3)]:
        b = _stream(kind, W, H, Cn, 90 if kind == "gradn" else 50)
        full = _full(b)
        for rect in _rects(W, H)[:8]:
            p = himg_amd.region_peek(b, *rect)
            st, out = _device(engine, [b], W, H, Cn, rect, plans=[p])
            assert st[0] == 0 and np.array_equal(out[0], _crop(full, rect)), (kind, rect)
            # the host path with every byte outside the plan (widened by 4) poisoned
            d = np.full_like(b, 0xA5)
            for a, e in _keep(b, p):
                d[a:e] = b[a:e]
            got = engine.decode_region(d, *rect)
            assert np.array_equal(got, _crop(full, rect)), (kind, rect)


def _mutate(good, rng):
    bad = good.copy()
    for _ in range(1 + int(rng.integers(0, 3))):
        i = int(rng.integers(0, len(bad))) if rng.random() < 0.3 else int(rng.integers(len(bad) // 3, len(bad)))
        bad[i] ^= 1 << int(rng.integers(0, 8))
    return bad


STAGE_MSG = {1: "Not a RIFF HIMG file.\n", 2: "Error decoding header.\n", 3: "Error decoding low-res mapping function.\n",
             4: "Error decoding low-res data.\n", 5: "Error decoding quantization configuration.\n",
             6: "Error decoding full-res mapping function.\n"}   # decoder.cpp:96-135 (the oracle returns -stage)
FRES_MSG = "Error decoding full-res data.\n"


@pytest.mark.parametrize("fix", [0, 1])
def test_verdict_fuzz(fix):
    """A partial rectangle of a stream the oracle rejects in the FRES stage is judged in test_gpu_partial_damage.py."""
    eng = himg_amd.Engine(0)
    eng.set_option("fix_t2", fix)
    rng = np.random.default_rng(7 + fix)
    bases = [_stream("randtile", 96, 48, 4, 50, True), _stream("gradn", 61, 27, 3, 90, True),
             _stream("rand", 64, 8, 1, 50, False), _stream("grad", 40, 40, 4, 0, True)]
    n_acc = n_rej = n_head = 0
    for t in range(1000):
        good = bases[t % len(bases)]
        W, H = int.from_bytes(good[21:25].tobytes(), "little"), int.from_bytes(good[25:29].tobytes(), "little")   # FRMT
        bad = _mutate(good, rng)
        rc, img = ol.oracle_decode(bad, fix_t2=bool(fix))
        whole = t % 3 == 0
        rect = (0, 0, W, H) if whole else (int(rng.integers(0, W)), int(rng.integers(0, H)), 1, 1)
        if not whole:
            rect = (rect[0], rect[1], int(rng.integers(1, W - rect[0] + 1)), int(rng.integers(1, H - rect[1] + 1)))
        try:
            got = eng.decode_region(bad, *rect)
            code, msg = 0, ""
        except himg_amd.HimgError as e:
            got, code, msg = None, e.code, str(e)
        if code == himg_amd.HIMG_ERR_ARG:
            # only a mutated FRMT chunk (header or body) can stop holding the rectangle
            assert not np.array_equal(bad[12:31], good[12:31]), (t, rect)
            continue
        if rc == 0:   # the reference accepts: so does the region, with the crop's pixels
            if code == himg_amd.HIMG_ERR_UNSUPPORTED:   # (an engine limit, a tree deeper than 32: shared with the full decode)
                with pytest.raises(himg_amd.HimgError) as e:
                    eng.decode(bad)
                assert e.value.code == code, (t, rect)
                continue
            assert code == 0, (t, rect, msg)
            assert np.array_equal(got, _crop(img, rect)), (t, rect)
            n_acc += 1
            continue
        n_rej += 1
        if whole or -6 <= rc <= -1:
            # a whole frame, or a head stage (RIFF .. FMAP) failing: himg_hip_decode's verdict and wording
            try:
                eng.decode(bad)
                full_code, full_msg = 0, ""
            except himg_amd.HimgError as e:
                full_code, full_msg = e.code, str(e)
            assert code == full_code, (t, rect, rc, code, full_code)
            full_msg, msg = full_msg.split(":", 1)[-1], msg.split(":", 1)[-1]
            if whole or not full_msg.endswith(FRES_MSG):
                assert msg == full_msg, (t, rect, msg, full_msg)
            else:
                # The full decode's verdict is the FRES stage's (its row walk or a row failed as well: the
                # engine reports the latest failing stage).  The region sees the head and only its own rows:
                # the FRES verdict, or a head stage at or after the one the reference stops at.
                assert msg.endswith(FRES_MSG) or any(msg.endswith(STAGE_MSG[k]) for k in range(-rc, 7)), (t, rect, msg)
        if -6 <= rc <= -1:
            n_head += 1
    assert n_acc > 50 and n_rej > 50 and n_head > 50


def _ends_after_row(b, r1):
    """b with its FRES chunk (the last one) cut right behind block row r1 - 1's payload."""
    offs, lens = himg_amd.index_host(b)[3:5]
    end = int(offs[r1 - 1]) + int(lens[r1 - 1])
    d = b[:end].copy()
    i = 12
    while True:   # the FRES chunk's size field, then RIFF's
        sz = int.from_bytes(d[i + 4:i + 8].tobytes(), "little")
        if d[i:i + 4].tobytes() == b"FRES":
            d[i + 4:i + 8] = np.frombuffer((end - i - 8).to_bytes(4, "little"), np.uint8)
            break
        i += 8 + sz
    d[4:8] = np.frombuffer((end - 8).to_bytes(4, "little"), np.uint8)
    return d


def test_chunk_ending_behind_the_last_touched_row(engine):
    """Rows from r1 on are not looked at, even when the chunk holds none of them: the host-indexed and
    the device-walked paths agree (accept, with the crop's pixels), and a rectangle reaching row r1
    is rejected like the full decode."""
    W, H, Cn = 256, 64, 4
    b = _stream("randtile", W, H, Cn)
    full = _full(b)
    d = _ends_after_row(b, 5)
    rect = (3, 17, 200, 23)   # rows 2 .. 4
    p = himg_amd.region_peek(d, *rect)
    assert p["row1"] == 5 and p["rows_end"] == len(d)
    assert np.array_equal(engine.decode_region(d, *rect), _crop(full, rect))
    st, out = _device(engine, [d, b], W, H, Cn, rect)
    assert (st == 0).all(), st
    assert np.array_equal(out[0], _crop(full, rect)) and np.array_equal(out[1], _crop(full, rect))
    for bad_rect in [(0, 0, W, H), (0, 39, 8, 2)]:
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_region(d, *bad_rect)
        assert e.value.code == himg_amd.HIMG_ERR_FORMAT
        st, _ = _device(engine, [d], W, H, Cn, bad_rect)
        assert st[0] != 0
