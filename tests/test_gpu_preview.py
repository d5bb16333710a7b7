"""GPU (-m gpu): the 1/8-scale preview (himg_hip_preview_*) against the oracle.  The expected
preview is the oracle decoder's low-res plane (oracle_decode_trace(...)["lowres"]) interleaved,
through a numpy restatement of YCbCr::YCbCrToRGB (ycbcr.cpp:54-82) where FRMT asks for it; the
verdict is the oracle's for its first four stages (-1 .. -4) and nothing behind them."""
import struct

import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol

pytestmark = pytest.mark.gpu

STAGE_MSG = {-1: "Not a RIFF HIMG file.\n", -2: "Error decoding header.\n",
             -3: "Error decoding low-res mapping function.\n", -4: "Error decoding low-res data.\n"}


def _chunks(b):
    b, out, i = bytes(b), {}, 12
    while i + 8 <= len(b):
        sz = struct.unpack("<I", b[i + 4:i + 8])[0]
        out[b[i:i + 4].decode("latin-1")] = (i + 8, sz)
        i += 8 + sz
    return out


def _ycc_to_rgb(p):
    """ycbcr.cpp:54-82 in int16 arithmetic, then the clamp; channels 3.. pass."""
    p = p.copy()
    y = p[..., 0].astype(np.int16)
    cb = (p[..., 1].astype(np.int16) << 1) - 255
    cr = (p[..., 2].astype(np.int16) << 1) - 255
    g = y - ((cb + cr + 2) >> 2)
    b = g + cb
    r = g + cr
    p[..., 0], p[..., 1], p[..., 2] = (np.clip(v, 0, 255).astype(np.uint8) for v in (r, g, b))
    return p


def _trace(packed, fix):
    ol.oracle().himg_oracle_set_compat_fix(1 if fix else 0)
    try:
        return ol.oracle_decode_trace(packed)
    finally:
        ol.oracle().himg_oracle_set_compat_fix(0)


def expected(packed, fix=False):
    """(oracle rc for the full decode, the preview or None).  A stream the reference rejects only
    behind the head (-5 .. -7) has the preview of its LRES plane: the trace with the fixed mode
    (the T2 rule is the FRES stream's; the LRES decode is the same either way)."""
    rc, tr = _trace(packed, fix)
    if rc < -4 and not fix:
        rc2, tr = _trace(packed, True)
        if rc2 != 0:
            tr = None
    if tr is None:
        return rc, None
    h, w, c = tr["pixels"].shape
    rows, cols = (h + 7) // 8, (w + 7) // 8
    low = tr["lowres"].reshape(c, rows, cols).transpose(1, 2, 0).copy()
    off, _ = _chunks(packed)["FRMT"]
    if packed[off + 10] != 0 and c >= 3:
        low = _ycc_to_rgb(low)
    return rc, low


def _head(packed):
    o, s = _chunks(packed)["LRES"]
    return o + s


def _preview_device(eng, streams, w, h, c, poison=False):
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5 if poison else 0, np.uint8)
    for i, s in enumerate(streams):
        if poison:   # every byte behind the head (rounded up to a dword) is garbage
            hb = (_head(s) + 3) // 4 * 4
            buf[i, :hb] = s[:hb]
        else:
            buf[i, :len(s)] = s
    d_in = torch.from_numpy(buf).cuda()
    ph, pw = (h + 7) // 8, (w + 7) // 8
    d_out = torch.zeros(n * ph * pw * c, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.preview_device(d_in, stride, [len(s) for s in streams], n, w, h, c, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy().reshape(n, ph, pw, c)


def _img(kind, w, h, seed=3):
    return himg_amd.synth(kind, seed, w, h)


PARITY = [  # kind, w, h, channels, ycbcr, quality
    ("randtile", 1000, 72, 4, True, 50), ("gradn", 517, 61, 3, True, 90), ("rand", 517, 61, 1, False, 50),
    ("randtile", 1000, 72, 2, False, 100), ("grad", 1000, 72, 4, False, 0), ("gradn", 1920, 1080, 4, True, 50),
    ("randtile", 1920, 1080, 3, False, 90), ("rand", 1920, 1080, 4, True, 100), ("grad", 517, 61, 3, True, 50),
    ("randtile", 517, 61, 4, True, 0), ("gradn", 1000, 72, 1, False, 100), ("rand", 1000, 72, 2, True, 0),
    ("randtile", 4096, 4096, 4, True, 50),
]


@pytest.mark.parametrize("kind,w,h,c,ycc,q", PARITY)
def test_parity(engine, kind, w, h, c, ycc, q):
    img = _img(kind, w, h)
    packed = ol.oracle_encode(img, q, ycc, channels=c, stride=4)
    rc, want = expected(packed)
    assert want is not None and rc in (0, -7), rc
    assert want.shape == ((h + 7) // 8, (w + 7) // 8, c)
    got = engine.preview(packed)
    assert np.array_equal(got, want)
    # only the head is present (rounded up to a dword), the whole stream's size is given
    hb = (_head(packed) + 3) // 4 * 4
    assert np.array_equal(engine.preview(packed[:hb].copy(), packed_size=len(packed)), want)
    b = engine.preview_batch([packed, packed])
    assert np.array_equal(b[0], want) and np.array_equal(b[1], want)
    st, out = _preview_device(engine, [packed], w, h, c)
    assert st[0] == 0 and np.array_equal(out[0], want)
    st, out = _preview_device(engine, [packed], w, h, c, poison=True)
    assert st[0] == 0 and np.array_equal(out[0], want)


def test_large_frame_16384():
    """One 16384^2 frame (GPU encode): LRES chunk counts near the 1024-chunk cap."""
    eng = himg_amd.Engine(0)
    img = _img("randtile", 16384, 16384, 1)
    packed = eng.encode(img, 50, True)
    del img
    rc, want = expected(packed)
    assert rc == 0
    assert np.array_equal(eng.preview(packed), want)
    st, out = _preview_device(eng, [packed], 16384, 16384, 4, poison=True)
    assert st[0] == 0 and np.array_equal(out[0], want)
    eng.close()


def _mutate(good, ch, rng, t):
    """A hostile stream: t % 2 == 0 in the head (RIFF header, FRMT, LMAP, the LRES tree or
    payload, chunk headers), t % 2 == 1 behind it (QCFG, FMAP, FRES)."""
    bad = good.copy()
    flip = lambda i: bad.__setitem__(i, bad[i] ^ (1 << int(rng.integers(0, 8))))
    if t % 2 == 0:
        k = (t // 2) % 7
        if k == 0:
            flip(int(rng.integers(0, 12)))                                  # RIFF, size, HIMG
        elif k == 1:
            o, s = ch["FRMT"]
            i = int(rng.choice([o - 8, o - 4, o, o + 1, o + 5, o + 10]))  # header, version, W/H low bytes, colour
            if i in (o + 1, o + 5):
                bad[i] ^= 1 << int(rng.integers(0, 3))
            else:
                flip(i)
        elif k == 2:
            o, s = ch["LMAP"]
            flip(int(rng.integers(o - 8, o + s)))                           # header and body
        elif k == 3:
            o, s = ch["LRES"]
            flip(int(rng.integers(o - 8, o)))                               # LRES header
        elif k == 4:
            o, s = ch["LRES"]
            for _ in range(1 + t % 3):
                flip(o + int(rng.integers(0, min(s, 340))))                 # tree
        else:
            o, s = ch["LRES"]
            i = int(rng.integers(o + min(400, s // 2), o + s))              # payload
            if t % 11 == 0:
                bad[i] = int(rng.integers(0, 256))
            else:
                flip(i)
    else:
        which = ("QCFG", "FMAP", "FRES", "FRES")[(t // 2) % 4]
        o, s = ch[which]
        flip(int(rng.integers(o - 8 if which != "FRES" else o, o + s)))
    return bad


FUZZ_BASES = [("randtile", 256, 64, 4, True, 50), ("gradn", 200, 120, 3, True, 70), ("rand", 128, 64, 1, False, 50),
              ("randtile", 64, 8, 4, True, 50)]     # 8 rows: the reference rejects the full decode (T2)
PER_BASE = 260   # x 5 bases (with the flat frame) x 2 modes = 2600 streams


def _frmt_geom(b):
    """(W, H, C) of the FRMT chunk the reference's forward search finds, or None."""
    b, i = bytes(b), 12
    while i + 8 <= len(b):
        tag, sz = b[i:i + 4], struct.unpack("<I", b[i + 4:i + 8])[0]
        i += 8
        if sz > 0x7fffffff or i + sz > len(b):
            return None
        if tag == b"FRMT":
            return struct.unpack("<II", b[i + 1:i + 9]) + (b[i + 9],) if sz >= 11 else None
        i += sz
    return None


def _splice(bad, good):
    """The head of `bad` with the clean chunks behind the head of `good` (RIFF size fixed up):
    stages 1-4 are bad's, so the oracle's low-res plane of it is what bad's preview must be."""
    hb = himg_amd.preview_peek(bad)[3]
    s = np.concatenate([bad[:hb], good[_head(good):]])
    s[4:8] = np.frombuffer(struct.pack("<I", len(s) - 8), np.uint8)
    return s


@pytest.mark.parametrize("fix", [0, 1])
def test_verdict_fuzz(fix):
    """Host path (preview_to) on every mutation; the head mutations and some behind the head
    once more in one preview_device batch per base, so that the device parse's checks of
    stages 1-4 (k_dec_parse_head) meet the damage too."""
    eng = himg_amd.Engine(0)
    eng.set_option("fix_t2", fix)
    rng = np.random.default_rng(4242 + fix)
    flat = np.full((48, 96, 4), 77, np.uint8)
    bases = [ol.oracle_encode(_img(k, w, h), q, y, channels=c, stride=4) for k, w, h, c, y, q in FUZZ_BASES]
    bases.append(ol.oracle_encode(flat, 50, True))   # flat: the reference rejects the full decode (T2)
    for good in bases[-2:]:
        assert ol.oracle_decode(good)[0] == -7 and ol.oracle_decode(good, fix_t2=True)[0] == 0
    fails = passes = spliced = unverified = dev_frames = deep = 0
    for good in bases:
        ch = _chunks(good)
        geom = _frmt_geom(good)
        rc0, clean = expected(good, bool(fix))
        assert clean is not None
        assert np.array_equal(eng.preview(good), clean)
        dev = []   # (stream, oracle rc, host preview or None)
        for t in range(PER_BASE):
            bad = _mutate(good, ch, rng, t)
            rc, want = expected(bad, bool(fix))
            try:
                got, err = eng.preview(bad), None
            except himg_amd.HimgError as e:
                got, err = None, e
            where = "mutation %d (%s)" % (t, "head" if t % 2 == 0 else "behind the head")
            if t % 2 == 0 or t % 8 == 1:
                dev.append((bad, rc, got))
            if -4 <= rc <= -1:
                assert got is None, "%s: oracle %d, preview accepted" % (where, rc)
                # FORMAT with the stage's message; UNSUPPORTED only for the documented deviation of
                # stage 4 (an LRES code deeper than 32 bits)
                if err.code == himg_amd.HIMG_ERR_UNSUPPORTED and rc == -4:
                    deep += 1
                else:
                    assert err.code == himg_amd.HIMG_ERR_FORMAT, (where, rc, str(err))
                    assert str(err).endswith(STAGE_MSG[rc]), (where, rc, str(err))
                fails += 1
                continue
            assert got is not None, "%s: oracle %d, preview rejected: %s" % (where, rc, err)
            passes += 1
            if t % 2 == 1:
                assert np.array_equal(got, clean), where
            if want is None and t % 2 == 0:
                # rejected behind the head even in the fixed mode: the head with clean chunks behind it
                rc2, want = expected(_splice(bad, good), bool(fix))
                spliced += 1
                if want is None:
                    unverified += 1
                    assert got.shape == ((geom[1] + 7) // 8, (geom[0] + 7) // 8, geom[2]) or _frmt_geom(bad) != geom
            if want is not None:
                assert np.array_equal(got, want), where
        # the device path: one launch with the base's geometry
        w, h, c = geom
        st, out = _preview_device(eng, [d[0] for d in dev], w, h, c)
        for k, (bad, rc, got) in enumerate(dev):
            same = _frmt_geom(bad) == geom
            if -4 <= rc <= -1:
                assert st[k] != 0, (k, rc)
                if st[k] & 15 == 4:
                    assert (st[k] >> 4) & 7 == -rc, (k, rc, st[k])
                elif st[k] & 15 == 3:
                    assert rc == -4, (k, rc, st[k])
                else:
                    assert st[k] & 15 == 1 and not same, (k, rc, st[k])
            elif same:
                assert st[k] == 0 and np.array_equal(out[k], got), (k, rc, st[k])
            else:
                assert st[k] & 15 == 1, (k, rc, st[k])
        dev_frames += len(dev)
    assert fails > 100 and passes > 100 and dev_frames > 600
    # every accepted head mutation had its pixels checked, but for a handful at most
    assert unverified <= 5, (unverified, spliced)
    assert deep <= fails // 10, deep
    eng.close()


def test_prefix_shorter_than_the_head(engine):
    """A buffer that ends before the end of the LRES chunk, with the whole stream's size: the
    binding refuses it (HIMG_ERR_CAPACITY, head_bytes reported) without reading past it."""
    packed = ol.oracle_encode(_img("randtile", 264, 40), 50, True)
    head = _head(packed)
    lres_hdr = _chunks(packed)["LRES"][0]
    for n, want_head in ((head - 1, head), (head // 2 if head // 2 >= lres_hdr else lres_hdr, head), (lres_hdr - 1, 0), (20, 0)):
        with pytest.raises(himg_amd.HimgError) as e:
            engine.preview(packed[:n].copy(), packed_size=len(packed))
        assert e.value.code == himg_amd.HIMG_ERR_CAPACITY and e.value.head_bytes == want_head, n
    assert np.array_equal(engine.preview(packed[:head].copy(), packed_size=len(packed)), expected(packed)[1])


def test_device_batch_statuses():
    """A device batch larger than the CU count, one damaged stream (LRES payload) and one of
    another geometry: per-frame statuses, the other frames right."""
    eng = himg_amd.Engine(0)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = n_cu + 17
    w, h, c = 264, 40, 4
    streams, wants = [], []
    for i in range(8):
        s = ol.oracle_encode(_img("randtile", w, h, seed=i), 50, True)
        streams.append(s)
        wants.append(expected(s)[1])
    frames = [streams[i % 8] for i in range(n)]
    want = [wants[i % 8] for i in range(n)]
    good = frames[5]
    ch = _chunks(good)
    bad = None
    rng = np.random.default_rng(9)
    for _ in range(200):
        cand = good.copy()
        o, s = ch["LRES"]
        cand[o + s // 2] ^= 1 << int(rng.integers(0, 8))
        cand[o + s // 2 + 1] ^= 1 << int(rng.integers(0, 8))
        if ol.oracle_decode(cand)[0] == -4:
            bad = cand
            break
    assert bad is not None
    frames[5] = bad
    other = ol.oracle_encode(_img("randtile", w + 8, h, seed=1), 50, True)   # another geometry
    frames[n - 3] = other
    st, out = _preview_device(eng, frames, w, h, c)
    for i in range(n):
        if i == 5:
            assert st[i] & 15 == 4, st[i]
        elif i == n - 3:
            assert st[i] & 15 == 1, st[i]
        else:
            assert st[i] == 0 and np.array_equal(out[i], want[i]), i
    eng.close()


def test_preview_batch_mixed_geometries(engine):
    items = [("randtile", 264, 40, 4, True), ("gradn", 517, 61, 3, True), ("randtile", 264, 40, 4, True),
             ("rand", 100, 20, 1, False), ("gradn", 517, 61, 3, True)]
    streams = [ol.oracle_encode(_img(k, w, h, seed=i), 50, y, channels=c, stride=4)
               for i, (k, w, h, c, y) in enumerate(items)]
    got = engine.preview_batch(streams)
    for s, g in zip(streams, got):
        assert np.array_equal(g, expected(s)[1])
    # a failing frame does not stop the others (the call reports it)
    bad = streams[1].copy()
    bad[0] ^= 1
    with pytest.raises(himg_amd.HimgError):
        engine.preview_batch([streams[0], bad, streams[2]])


def test_preview_batch_more_frames_than_one_launch(engine):
    """More frames of one geometry than one launch takes (256): several launches, every frame right."""
    streams = [ol.oracle_encode(_img("randtile", 72, 24, seed=i), 50, True) for i in range(4)]
    wants = [expected(s)[1] for s in streams]
    other = ol.oracle_encode(_img("gradn", 40, 16, seed=1), 50, False, channels=3, stride=4)
    batch = [streams[i % 4] for i in range(300)] + [other]
    got = engine.preview_batch(batch)
    assert len(got) == 301
    for i in range(300):
        assert np.array_equal(got[i], wants[i % 4]), i
    assert np.array_equal(got[300], expected(other)[1])
