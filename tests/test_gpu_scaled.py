"""GPU (-m gpu): the decode at 1/2 and 1/4 scale (himg_hip_decode_scaled_*) against its
definition restated in numpy (tests/scaled_model.py, from the oracle decoder's trace), byte for
byte: parity over shapes, channel counts, colour spaces and qualities through the host call, the
device batch and the host batch; the verdict against decode()'s on mutated streams; damaged frames
inside a batch; the capacity protocol; dhimg -s2 / -s4."""
import subprocess

import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol
import scaled_model as sm
from golden_util import GOLDEN
from himg_amd import build as hb

pytestmark = pytest.mark.gpu

SCALES = (1, 2)


def _img(kind, w, h, seed=3):
    return himg_amd.synth(kind, seed, w, h)


def _stream(kind, w, h, c, ycc, q, seed=3):
    return ol.oracle_encode(_img(kind, w, h, seed), q, ycc, channels=c, stride=4)


def _device(eng, streams, w, h, c, s):
    n = len(streams)
    stride = (max(len(b) for b in streams) + 3 + 255) // 256 * 256
    buf = np.zeros((n, stride), np.uint8)
    for i, b in enumerate(streams):
        buf[i, :len(b)] = b
    ow, oh = himg_amd.scaled_size(w, h, s)
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.zeros(n * oh * ow * c + 16, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_scaled_device(d_in, stride, [len(b) for b in streams], n, w, h, c, s, d_out, d_st)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert not out[n * oh * ow * c:].any()   # nothing behind the last frame
    return d_st.cpu().numpy(), out[:n * oh * ow * c].reshape(n, oh, ow, c)


def _needs_fix(packed):
    """A stream the reference rejects on its own (trap T2: one block row, flat pictures) is decoded in
    the fixed mode, HIMG_OPT_FIX_T2."""
    return ol.oracle_decode(packed)[0] != 0


# kind, w, h, channels, ycbcr, quality: tests/test_gpu_preview.py's PARITY shapes ...
PARITY = [
    ("randtile", 1000, 72, 4, True, 50), ("gradn", 517, 61, 3, True, 90), ("rand", 517, 61, 1, False, 50),
    ("randtile", 1000, 72, 2, False, 100), ("grad", 1000, 72, 4, False, 0), ("gradn", 1920, 1080, 4, True, 50),
    ("randtile", 1920, 1080, 3, False, 90), ("rand", 1920, 1080, 4, True, 100), ("grad", 517, 61, 3, True, 50),
    ("randtile", 517, 61, 4, True, 0), ("gradn", 1000, 72, 1, False, 100), ("rand", 1000, 72, 2, True, 0),
    ("randtile", 4096, 4096, 4, True, 50),
    # ... one-row and one-column frames, a pixel, q10, 4096^2 at q90 (rows past 36 KiB), a frame wider
    # than the full decode's LDS limit, and noise at q100 with four channels and both colour spaces
    # (coefficients that wrap in the int16 store of the dequantisation)
    ("randtile", 300, 1, 4, True, 50), ("gradn", 1, 200, 3, True, 90), ("rand", 1, 1, 4, True, 50),
    ("rand", 9, 9, 4, True, 10), ("gradn", 203, 45, 3, True, 10), ("randtile", 4096, 4096, 4, True, 90),
    ("randtile", 8200, 72, 4, True, 50), ("rand", 8200, 24, 3, False, 100), ("rand", 203, 45, 4, False, 100),
    ("rand", 64, 8, 4, True, 100),
]


@pytest.mark.parametrize("kind,w,h,c,ycc,q", PARITY)
def test_parity(kind, w, h, c, ycc, q):
    eng = himg_amd.Engine(0)
    big = w * h > 1920 * 1080
    seeds = [3, 4, 5, 6, 7]
    streams = [_stream(kind, w, h, c, ycc, q, seed) for seed in seeds]
    fix = any(_needs_fix(b) for b in streams)
    eng.set_option("fix_t2", int(fix))
    traces = []
    ol.oracle().himg_oracle_set_compat_fix(int(fix))
    try:
        for b in streams:
            rc, tr = ol.oracle_decode_trace(b)
            assert rc == 0
            traces.append(tr)
    finally:
        ol.oracle().himg_oracle_set_compat_fix(0)
    for s in SCALES:
        wants = [sm.scaled_from_trace(tr, b, s) for tr, b in zip(traces, streams)]
        assert wants[0].shape == himg_amd.scaled_size(w, h, s)[::-1] + (c,)
        got = eng.decode_scaled(streams[0], s)
        assert got.shape == wants[0].shape and np.array_equal(got, wants[0]), (s, "decode_scaled")
        st, out = _device(eng, streams, w, h, c, s)
        assert (st == 0).all(), st
        for i in range(len(streams)):
            assert np.array_equal(out[i], wants[i]), (s, "decode_scaled_device", i)
        sub = streams[:2] if big else streams
        b = eng.decode_scaled_batch(sub, s)
        for i in range(len(sub)):
            assert np.array_equal(b[i], wants[i]), (s, "decode_scaled_batch", i)
    eng.close()


def test_large_frame_16384():
    """The 16384^2 golden frame (GPU encode, the stream checked against the golden table): one column
    strip of 2048 tiles at either scale.  One frame: a trace of it takes the oracle most of a minute."""
    rec = GOLDEN["randtile_s0_16384x16384_q50"]
    eng = himg_amd.Engine(0)
    img = _img("randtile", 16384, 16384, 0)
    packed = eng.encode(img, 50, True)
    del img
    assert packed.size == rec["packed_size"] and himg_amd.fnv1a64(packed) == rec["stream_fnv"]
    rc, tr = ol.oracle_decode_trace(packed)
    assert rc == 0
    for s in SCALES:
        want = sm.scaled_from_trace(tr, packed, s)
        assert np.array_equal(eng.decode_scaled(packed, s), want), s
        st, out = _device(eng, [packed], 16384, 16384, 4, s)
        assert st[0] == 0 and np.array_equal(out[0], want), s
        got = eng.decode_scaled_batch([packed], s)
        assert np.array_equal(got[0], want), s
    eng.close()


@pytest.mark.parametrize("wave", [0, 1])
def test_count_kernel_forms(wave):
    """Both count kernels behind the scaled row kernel (launch_decode's rule picks by batch size)."""
    eng = himg_amd.Engine(0)
    eng.set_option("count_wave", wave)
    for kind, w, h, c, ycc, q in [("randtile", 1920, 40, 4, True, 50), ("rand", 8200, 40, 4, True, 50),
                                  ("gradn", 101, 37, 3, True, 90)]:
        b = _stream(kind, w, h, c, ycc, q, seed=1)
        for s in SCALES:
            want = sm.expected(b, s)[1]
            assert np.array_equal(eng.decode_scaled(b, s), want), (wave, kind, s)
            st, out = _device(eng, [b, b], w, h, c, s)
            assert (st == 0).all() and np.array_equal(out[0], want) and np.array_equal(out[1], want), (wave, kind, s)
    eng.close()


def _mutate(good, ch, rng, t):
    """tests/test_gpu_preview.py's mutators (head: RIFF header, FRMT, LMAP, the LRES tree or payload,
    chunk headers; behind the head: QCFG, FMAP, FRES) and tests/test_gpu_region.py's (a few bit
    flips, mostly in the last two thirds of the stream), in turn."""
    bad = good.copy()
    flip = lambda i: bad.__setitem__(i, bad[i] ^ (1 << int(rng.integers(0, 8))))
    if t % 3 == 2:
        for _ in range(1 + int(rng.integers(0, 3))):
            flip(int(rng.integers(0, len(bad))) if rng.random() < 0.3 else int(rng.integers(len(bad) // 3, len(bad))))
    elif t % 2 == 0:
        k = (t // 2) % 7
        if k == 0:
            flip(int(rng.integers(0, 12)))
        elif k == 1:
            o, s = ch["FRMT"]
            i = int(rng.choice([o - 8, o - 4, o, o + 1, o + 5, o + 10]))
            if i in (o + 1, o + 5):
                bad[i] ^= 1 << int(rng.integers(0, 3))
            else:
                flip(i)
        elif k == 2:
            o, s = ch["LMAP"]
            flip(int(rng.integers(o - 8, o + s)))
        elif k == 3:
            o, s = ch["LRES"]
            flip(int(rng.integers(o - 8, o)))
        elif k == 4:
            o, s = ch["LRES"]
            for _ in range(1 + t % 3):
                flip(o + int(rng.integers(0, min(s, 340))))
        else:
            o, s = ch["LRES"]
            i = int(rng.integers(o + min(400, s // 2), o + s))
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
PER_BASE = 90   # x 5 bases (with the flat frame) x 2 modes = 900 streams, each at one of the two scales


def _verdict(call):
    try:
        return call(), 0, ""
    except himg_amd.HimgError as e:
        return None, e.code, str(e).split(":", 1)[-1]


@pytest.mark.parametrize("fix", [0, 1])
def test_verdict_fuzz(fix):
    """Status and message equal decode()'s for every stream; where both accept, the pixels equal the
    model on the mutated stream.  Then the same streams of a base in one device batch: each frame's
    status is zero exactly where decode() accepted it."""
    eng = himg_amd.Engine(0)
    eng.set_option("fix_t2", fix)
    rng = np.random.default_rng(777 + fix)
    flat = np.full((48, 96, 4), 77, np.uint8)
    bases = [_stream(k, w, h, c, y, q) for k, w, h, c, y, q in FUZZ_BASES]
    bases.append(ol.oracle_encode(flat, 50, True))
    n_acc = n_rej = n_dev = 0
    for bi, good in enumerate(bases):
        ch = sm.find_chunks(good)
        o = ch["FRMT"][0]
        geom = (int.from_bytes(bytes(good[o + 1:o + 5]), "little"), int.from_bytes(bytes(good[o + 5:o + 9]), "little"),
                int(good[o + 9]))
        dev = []
        for t in range(PER_BASE):
            s = 1 + (t + bi) % 2
            bad = _mutate(good, ch, rng, t)
            full, fcode, fmsg = _verdict(lambda: eng.decode(bad))
            got, code, msg = _verdict(lambda: eng.decode_scaled(bad, s))
            assert code == fcode, (bi, t, s, code, fcode, msg, fmsg)
            assert msg == fmsg, (bi, t, s, msg, fmsg)
            rc, want = sm.expected(bad, s, bool(fix)) if code == 0 else (None, None)
            if code == 0:
                assert rc == 0 and np.array_equal(got, want), (bi, t, s)
                n_acc += 1
            else:
                n_rej += 1
            if t % 3 == 0:
                dev.append((bad, s, fcode, want))
        for s in SCALES:
            grp = [d for d in dev if d[1] == s]
            st, out = _device(eng, [d[0] for d in grp], geom[0], geom[1], geom[2], s)
            for k, (bad, _, fcode, want) in enumerate(grp):
                assert (st[k] == 0) == (fcode == 0) or (fcode == 0 and st[k] & 15 == 1), (bi, s, k, st[k], fcode)
                if st[k] == 0:
                    assert np.array_equal(out[k], want), (bi, s, k)
            n_dev += len(grp)
    assert n_acc > 100 and n_rej > 100 and n_dev > 100, (n_acc, n_rej, n_dev)
    eng.close()


def test_damaged_frames_in_a_batch():
    """A device batch larger than the CU count in which some frames are damaged (an FRES payload, an
    LRES payload, a frame of another geometry): the others' bytes and statuses do not change."""
    eng = himg_amd.Engine(0)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = n_cu + 17
    w, h, c = 264, 40, 4
    streams = [_stream("randtile", w, h, 4, True, 50, seed=i) for i in range(8)]
    rng = np.random.default_rng(9)
    for s in SCALES:
        wants = [sm.expected(b, s)[1] for b in streams]
        frames = [streams[i % 8] for i in range(n)]
        st0, out0 = _device(eng, frames, w, h, c, s)
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
                if ol.oracle_decode(cand)[0] != 0:
                    bad[idx] = cand
                    break
            assert idx in bad
        for idx, cand in bad.items():
            frames[idx] = cand
        frames[n - 3] = _stream("randtile", w + 8, h, 4, True, 50, seed=1)   # another geometry
        st, out = _device(eng, frames, w, h, c, s)
        for i in range(n):
            if i in bad:
                assert st[i] & 15 == 4, (i, st[i])
            elif i == n - 3:
                assert st[i] & 15 == 1, st[i]
            else:
                assert st[i] == 0 and np.array_equal(out[i], wants[i % 8]) and np.array_equal(out[i], out0[i]), (s, i)
    eng.close()


def test_capacity_protocol_and_fetch_last(engine):
    import ctypes as C
    b = _stream("randtile", 264, 40, 4, True, 50)
    L = himg_amd.lib()
    for s in SCALES:
        want = sm.expected(b, s)[1]
        ow, oh = himg_amd.scaled_size(264, 40, s)
        w_, h_, c_ = C.c_int(), C.c_int(), C.c_int()
        small = np.zeros(want.size - 1, np.uint8)
        for dst, cap in ((None, 0), (small.ctypes.data, small.nbytes)):
            rc = L.himg_hip_decode_scaled_to(engine._ctx, b.ctypes.data, b.nbytes, s, dst, cap, C.byref(w_), C.byref(h_),
                                             C.byref(c_))
            assert rc == himg_amd.HIMG_ERR_CAPACITY and (w_.value, h_.value, c_.value) == (ow, oh, 4)
            out, n = np.zeros(want.size, np.uint8), C.c_size_t()
            assert L.himg_hip_fetch_last(engine._ctx, out.ctypes.data, out.nbytes, C.byref(n)) == 0
            assert n.value == want.size and np.array_equal(out.reshape(want.shape), want)
        assert not small.any()
        # a reused output buffer
        buf = np.zeros(want.size, np.uint8)
        got = engine.decode_scaled(b, s, out=buf)
        assert np.shares_memory(got, buf) and np.array_equal(got, want)
    for bad_scale in (0, 3, -1):
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_scaled(b, bad_scale)
        assert e.value.code == himg_amd.HIMG_ERR_ARG
        with pytest.raises(himg_amd.HimgError) as e:
            engine.decode_scaled_batch([b], bad_scale)
        assert e.value.code == himg_amd.HIMG_ERR_ARG


def test_batch_mixed_geometries_and_failing_frames(engine):
    items = [("randtile", 264, 40, 4, True), ("gradn", 517, 61, 3, True), ("randtile", 264, 40, 4, True),
             ("rand", 100, 20, 1, False), ("gradn", 517, 61, 3, True)]
    streams = [_stream(k, w, h, c, y, 50, seed=i) for i, (k, w, h, c, y) in enumerate(items)]
    for s in SCALES:
        got = engine.decode_scaled_batch(streams, s)
        for b, g in zip(streams, got):
            assert np.array_equal(g, sm.expected(b, s)[1])
    # a failing frame does not stop the others: widths[i] = 0 for it, the first error returned
    import ctypes as C
    bad = streams[1].copy()
    bad[0] ^= 1
    trio = [streams[0], bad, streams[2]]
    with pytest.raises(himg_amd.HimgError):
        engine.decode_scaled_batch(trio, 1)
    n = 3
    outs = [np.zeros(1 << 16, np.uint8) for _ in range(n)]
    src = (C.c_void_p * n)(*[b.ctypes.data for b in trio])
    szs = (C.c_size_t * n)(*[b.nbytes for b in trio])
    dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
    caps[2] = 10   # too small
    ws, hs, cs = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    rc = himg_amd.lib().himg_hip_decode_scaled_batch(engine._ctx, src, szs, n, 1, dst, caps, ws, hs, cs)
    assert rc == himg_amd.HIMG_ERR_FORMAT
    want = sm.expected(streams[0], 1)[1]
    assert (ws[0], hs[0], cs[0]) == (132, 20, 4) and np.array_equal(outs[0][:want.size].reshape(want.shape), want)
    assert ws[1] == 0 and ws[2] == 0 and not outs[2].any()


def test_batch_more_frames_than_one_launch(engine):
    """More frames of one geometry than one launch takes (256): several launches, every frame right."""
    streams = [_stream("rand", 72, 24, 4, True, 50, seed=i) for i in range(4)]   # (noise: randtile this small is trap T2)
    other = _stream("rand", 40, 16, 3, False, 50, seed=1)   # (noise: a stream the reference accepts)
    batch = [streams[i % 4] for i in range(300)] + [other]
    for s in SCALES:
        wants = [sm.expected(b, s)[1] for b in streams]
        got = engine.decode_scaled_batch(batch, s)
        assert len(got) == 301
        for i in range(300):
            assert np.array_equal(got[i], wants[i % 4]), i
        assert np.array_equal(got[300], sm.expected(other, s, fix=False)[1])


def _read_pnm(path):
    with open(path, "rb") as fh:
        data = fh.read()
    assert data[:2] == b"P7"
    head, body = data.split(b"ENDHDR\n", 1)
    f = dict(line.split(b" ", 1) for line in head.split(b"\n")[1:] if b" " in line)
    w, h, c = int(f[b"WIDTH"]), int(f[b"HEIGHT"]), int(f[b"DEPTH"])
    return np.frombuffer(body, np.uint8).reshape(h, w, c)


@pytest.mark.parametrize("flag,s", [("-s2", 1), ("-s4", 2)])
def test_dhimg_scaled(tmp_path, flag, s):
    """dhimg -s2 / -s4 image outfile: the scaled picture, through the tool's own row flip and
    channel swap (the stream holds the picture bottom-up, BGRA)."""
    dhimg = hb.build_cli()[1]
    b = _stream("randtile", 264, 136, 4, True, 70)
    src, out = str(tmp_path / "a.himg"), str(tmp_path / "a.pam")
    b.tofile(src)
    r = subprocess.run([dhimg, flag, src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "File size: %d\n" % b.size, (r.stdout, r.stderr)
    want = sm.expected(b, s)[1][::-1, :, [2, 1, 0, 3]]
    assert np.array_equal(_read_pnm(out), want)
    # without the flag nothing changes: the full picture
    r = subprocess.run([dhimg, src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "File size: %d\n" % b.size
    assert np.array_equal(_read_pnm(out), ol.oracle_decode(b)[1][::-1, :, [2, 1, 0, 3]])
    # a stream the decoder rejects: the library's message, then the tool's
    bad = b.copy()
    bad[0] ^= 1
    bad.tofile(src)
    r = subprocess.run([dhimg, flag, src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 255 and r.stdout.splitlines()[-2:] == ["Not a RIFF HIMG file.", "Unable to decode image."]
