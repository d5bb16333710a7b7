"""GPU: the device entry points at byte offsets beyond 4 GiB.  Every kernel adds products such as
f * in_stride, f * out_stride, f * frame_pitch, y * row_pitch or f * bytes-per-frame to a base pointer; a
product or an intermediate kept in 32 bits would wrap silently at 2^32 (at 2^31 if it were signed).

  A. tiny pictures, far frames: a stride or pitch of 2^30 + a little puts frame 4 of 5 beyond 2^32 and
     frames 2 and 3 beyond 2^31 (row_pitch = 2^26 + 4: row 64 of one picture);
  B. dense batches of 2048 x 2048 frames whose f * bytes-per-frame passes 2^32 with two whole frames
     beyond it -- the only way to push the workspace planes past 4 GiB as well.

Frame f holds picture f % 3 of three distinct pictures, so an offset that wraps lands on ANOTHER valid
picture or stream and shows as wrong bytes or a wrong status.  Every expected byte comes from the CPU
oracle and the models the forms already have; every output buffer is filled with 0xA5, has a 64-byte
tail and is compared WHOLE on the device (far_model.check_buffer / check_dense), whose message names
the byte offset, the offset modulo 2^32 and the frame.  The module has an engine of its own: a context
keeps its workspace at the largest size it has seen.

Device memory: each test's need is computed in far_model.py and stands in its docstring; with less
free memory the test skips."""
import functools
import gc

import numpy as np
import pytest
import torch

import budget_model as bm
import conceal_model as cm
import damage_model as dm
import far_model as fm
import himg_amd
import oracle_lib as ol
import prefix_model as pm
import scaled_model as sm
import target_model as tgm
import tensor_model as tm
from test_gpu_into import _padded, _paste, _status
from test_gpu_preview import expected as preview_expected
from test_gpu_region import _crop, _full, _stream
from test_gpu_regions import _upload

pytestmark = pytest.mark.gpu

B, K, TAIL, SENTINEL = fm.FAR_BATCH, fm.K, fm.TAIL, fm.SENTINEL
STRIDE = fm.FAR_STRIDE
POISON32 = 0x5a5a5a5a
GIB = 1 << 30


# ---- the module's engine, memory ------------------------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    e = himg_amd.Engine(0)
    yield e
    torch.cuda.synchronize()
    e.close()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _tidy(eng):
    """The engine's options back and the big tensors gone behind every test."""
    saved = {k: eng.get_option(k) for k in ("fix_t2", "row_tokens", "front")}
    yield
    torch.cuda.synchronize()
    for k, v in saved.items():
        eng.set_option(k, v)
    gc.collect()
    torch.cuda.empty_cache()


def _require(need):
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %d bytes of device memory, %d are free" % (need, free))


class _Meter:
    """Prints what a test took: torch's peak, and the drop of free device memory that torch's reserve does
    not explain (the library's workspace is not torch's)."""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.free0, self.res0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        drop = self.free0 - torch.cuda.mem_get_info()[0]
        grown = torch.cuda.memory_reserved() - self.res0
        print("%s: torch peak %.2f GiB, free memory fell by %.2f GiB, of which %.2f GiB outside torch"
              % (self.what, torch.cuda.max_memory_allocated() / GIB, drop / GIB, (drop - grown) / GIB))


def _sentinel(nbytes):
    return torch.full((nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")


def _dev(a):
    """A numpy array's bytes as a 1-D uint8 tensor on the device."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _ok(d_st, what, **pitches):
    """Every d_status is HIMG_OK.  pitches: the bytes from a frame to the next of the call's buffers by name; a
    frame that failed is reported with where its bytes start in each -- a wrapped offset shows there."""
    st = d_st.cpu().numpy()
    bad = [f for f in range(st.size) if st[f] != himg_amd.HIMG_OK]
    if bad:
        lines = ["frame %d: status %d%s" % (f, st[f], "".join("; its %s starts at %s" % (k, fm.where(f * v))
                                                               for k, v in pitches.items())) for f in bad[:fm.MAX_REPORTS]]
        raise AssertionError("%s: %d of %d frames failed: %s" % (what, len(bad), st.size, " | ".join(lines)))


def _sizes(d_sizes, want, what, **pitches):
    """d_sizes is exact; a frame whose size differs is reported as _ok reports a failed one."""
    got = d_sizes.cpu().tolist()
    bad = [f for f in range(len(want)) if got[f] != want[f]]
    if bad:
        lines = ["frame %d: %d bytes, expected %d%s" % (f, got[f], want[f], "".join(
            "; its %s starts at %s" % (k, fm.where(f * v)) for k, v in pitches.items())) for f in bad[:fm.MAX_REPORTS]]
        raise AssertionError("%s: d_sizes of %d of %d frames differ: %s" % (what, len(bad), len(want), " | ".join(lines)))


# ---- A. far frames by stride and pitch --------------------------------------------------------------

CASES = [(72, 40, 4, True, 50), (264, 40, 3, False, 90)]   # W, H, C, ycbcr, quality
CASE_IDS = ["72x40x4-ycbcr", "264x40x3-rgb"]
WIN = (40, 17)


@functools.lru_cache(maxsize=None)
def _case(W, H, Cn, ycc, q):
    """Three oracle streams of distinct pictures, the decode mode they need, the oracle's pictures."""
    streams = [_stream("randtile", W, H, Cn, q, ycc, seed=s + 1) for s in range(K)]
    fix = any(ol.oracle_decode(s)[0] != 0 for s in streams)
    pics = [_full(s, fix).reshape(H, W, Cn) for s in streams]
    assert not any(np.array_equal(pics[a], pics[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    return streams, fix, pics


@functools.lru_cache(maxsize=None)
def _models(W, H, Cn, ycc, q):
    streams, fix, _ = _case(W, H, Cn, ycc, q)
    return [pm.Model(s, fix) for s in streams]


@pytest.fixture(scope="module")
def far_in():
    """The input of A.1, once for the module: stream f at f * (2^30 + 256)."""
    n = (B - 1) * STRIDE + (1 << 20)
    _require(fm.need_far(n))
    t = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    yield t
    del t


def _place(far_in, streams):
    """Stream f at f * STRIDE of the far input; the sizes.  The offsets the call must reach are far."""
    for f, s in enumerate(streams):
        assert (len(s) + 3) // 4 * 4 <= STRIDE and f * STRIDE + len(s) + 4 <= far_in.numel()
        far_in[f * STRIDE:f * STRIDE + len(s)] = torch.from_numpy(s).cuda()
    fm.assert_far([f * STRIDE for f in range(len(streams))])
    return [len(s) for s in streams]


def _far_decode(eng, far_in, case, frame_bytes, wants, call, what, streams=None):
    """One call on the far input: frame f is picture f % 3 (or streams[f]); wants[f]: its expected bytes.
    call(sizes, d_out, d_status).  Statuses, then the whole output."""
    good, fix, _ = _case(*case)
    eng.set_option("fix_t2", int(fix))
    sizes = _place(far_in, streams or [good[f % K] for f in range(B)])
    d_out, d_st = _sentinel(B * frame_bytes), _status(B)
    call(sizes, d_out, d_st)
    torch.cuda.synchronize()
    _ok(d_st, what, input=STRIDE)
    fm.check_buffer(d_out, [(f * frame_bytes, _dev(wants[f])) for f in range(B)], what, pitch=frame_bytes)
    return d_out


def _origins(W, H, w, h):
    cycle = [(3, 5), (W - w, H - h), (8, 8)]   # inside, the corner, aligned
    return [cycle[f % 3] for f in range(B)]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_decode(eng, far_in, case):
    """decode_device with in_stride = 2^30 + 256.  Need: 8.0 GiB (the 4 GiB + 1 MiB input, 1 GiB of
    workspace allowance, 3 GiB for the comparison's chunks); measured: 4.0 GiB in torch, a workspace below 0.01 GiB."""
    W, H, Cn = case[:3]
    pics = _case(*case)[2]
    _far_decode(eng, far_in, case, H * W * Cn, [pics[f % K] for f in range(B)],
                lambda sizes, d_out, d_st: eng.decode_device(far_in, STRIDE, sizes, B, W, H, Cn, d_out, d_st), "decode_device")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_region_and_regions(eng, far_in, case):
    """decode_region_device (one rectangle) and decode_regions_device (an origin per frame).  Need: 8.0 GiB."""
    W, H, Cn = case[:3]
    pics = _case(*case)[2]
    w, h = WIN
    rect = (5, 3, w, h)
    _far_decode(eng, far_in, case, h * w * Cn, [_crop(pics[f % K], rect) for f in range(B)],
                lambda sizes, d_out, d_st: eng.decode_region_device(far_in, STRIDE, sizes, B, W, H, Cn, *rect, d_out, d_st),
                "decode_region_device")
    org = _origins(W, H, w, h)
    _far_decode(eng, far_in, case, h * w * Cn, [_crop(pics[f % K], org[f] + WIN) for f in range(B)],
                lambda sizes, d_out, d_st: eng.decode_regions_device(far_in, STRIDE, sizes, B, W, H, Cn, org, w, h, d_out, d_st),
                "decode_regions_device")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_tensor_f16(eng, far_in, case):
    """decode_tensor_device, float16, ImageNet mean / std.  Need: 8.0 GiB."""
    W, H, Cn = case[:3]
    pics = _case(*case)[2]
    desc = tm.imagenet(tm.F16, min(Cn, 3))
    fb = himg_amd.tensor_bytes(desc, Cn, W, H)
    _far_decode(eng, far_in, case, fb, [tm.expected(pics[f % K], desc) for f in range(B)],
                lambda sizes, d_out, d_st: eng.decode_tensor_device(far_in, STRIDE, sizes, B, W, H, Cn, desc, d_out, d_st),
                "decode_tensor_device")


@functools.lru_cache(maxsize=None)
def _levels(case):
    """Per picture {level: the model's picture}: the oracle's, scaled_model's (1/2, 1/4), the preview's (1/8)."""
    streams, fix, pics = _case(*case)
    out = []
    for s, p in zip(streams, pics):
        lv = {0: p}
        for k in (1, 2):
            rc, lv[k] = sm.expected(s, k, fix)
            assert rc == 0
        rc, lv[3] = preview_expected(s, fix)
        assert rc == 0
        out.append(lv)
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_scaled_and_preview(eng, far_in, case):
    """decode_scaled_device (1/2, 1/4), decode_scaled_regions_device (a window per frame of the 1/2-scale
    picture) and preview_device.  Need: 8.0 GiB."""
    W, H, Cn = case[:3]
    lv = _levels(case)
    for s in (1, 2):
        ow, oh = himg_amd.scaled_size(W, H, s)
        _far_decode(eng, far_in, case, oh * ow * Cn, [lv[f % K][s] for f in range(B)],
                    lambda sizes, d_out, d_st: eng.decode_scaled_device(far_in, STRIDE, sizes, B, W, H, Cn, s, d_out, d_st),
                    "decode_scaled_device 1/%d" % (1 << s))
    ow, oh = himg_amd.scaled_size(W, H, 1)
    w, h = 16, 9
    cycle = [(1, 2), (ow - w, oh - h), (4, 4)]
    org = [cycle[f % 3] for f in range(B)]
    _far_decode(eng, far_in, case, h * w * Cn, [_crop(lv[f % K][1], org[f] + (w, h)) for f in range(B)],
                lambda sizes, d_out, d_st: eng.decode_scaled_regions_device(far_in, STRIDE, sizes, B, W, H, Cn, 1, org, w, h,
                                                                            d_out, d_st), "decode_scaled_regions_device")
    ph, pw = lv[0][3].shape[:2]
    _far_decode(eng, far_in, case, ph * pw * Cn, [lv[f % K][3] for f in range(B)],
                lambda sizes, d_out, d_st: eng.preview_device(far_in, STRIDE, sizes, B, W, H, Cn, d_out, d_st), "preview_device")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_pyramid(eng, far_in, case):
    """decode_pyramid_device, all four levels.  Need: 8.0 GiB."""
    W, H, Cn = case[:3]
    good, fix, _ = _case(*case)
    lv = _levels(case)
    eng.set_option("fix_t2", int(fix))
    sizes = _place(far_in, [good[f % K] for f in range(B)])
    fbs = [int(np.prod(lv[0][k].shape)) for k in range(4)]
    bufs = [_sentinel(B * fb) for fb in fbs]
    d_st = _status(B)
    eng.decode_pyramid_device(far_in, STRIDE, sizes, B, W, H, Cn, himg_amd.pyramid_desc(*bufs), d_st)
    torch.cuda.synchronize()
    _ok(d_st, "decode_pyramid_device", input=STRIDE)
    for k in range(4):
        fm.check_buffer(bufs[k], [(f * fbs[k], _dev(lv[f % K][k])) for f in range(B)], "pyramid level %d" % k, pitch=fbs[k])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_prefix(eng, far_in, case):
    """decode_prefix_device: whole streams (even frames) and a cut inside the third block row (odd frames).
    Need: 8.0 GiB."""
    W, H, Cn = case[:3]
    models = _models(*case)
    avail, want, rows = [], [], []
    for f in range(B):
        m = models[f % K]
        ends = m.row_ends()
        a = m.T if f % 2 == 0 else (ends[2] + ends[3]) // 2
        code, k, pic = m.expect(a)
        assert code == pm.OK and k == (m.rows if f % 2 == 0 else 2)
        avail.append(a)
        want.append(pic)
        rows.append(k)
    d_rows = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    _far_decode(eng, far_in, case, H * W * Cn, want,
                lambda sizes, d_out, d_st: eng.decode_prefix_device(far_in, STRIDE, avail, B, W, H, Cn, d_out, d_rows, d_st),
                "decode_prefix_device")
    assert d_rows.cpu().tolist() == rows


@functools.lru_cache(maxsize=None)
def _damaged(case, r=2):
    """Picture 1's stream with one bit flipped inside block row r's payload, a flip that the oracle rejects
    (so the row is concealed): (stream, (picture, rowmap) of conceal_model)."""
    streams, fix, _ = _case(*case)
    m = _models(*case)[1]
    o, n = dm.rows_of(streams[1], fix)[1][r]
    for at in range(o + n // 2, o + n):
        bad = streams[1].copy()
        bad[at] ^= 0x10
        pic, rowmap = cm.expect(m, bad, fix)
        if rowmap[r]:
            assert int(rowmap.sum()) == 1
            return bad, pic, rowmap
    raise AssertionError("no rejected flip in row %d" % r)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_conceal(eng, far_in, case):
    """decode_conceal_device: clean frames, and frames 1 and 4 (the one beyond 2^32) with a damaged block
    row that is concealed from the low-res plane.  Need: 8.0 GiB."""
    W, H, Cn = case[:3]
    good, fix, pics = _case(*case)
    bad, bad_pic, bad_map = _damaged(case)
    rows = (H + 7) // 8
    streams = [bad if f in (1, 4) else good[f % K] for f in range(B)]
    want = [bad_pic if f in (1, 4) else pics[f % K] for f in range(B)]
    maps = [bad_map if f in (1, 4) else np.zeros(rows, np.uint8) for f in range(B)]
    d_cn = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    d_map = _sentinel(B * rows)
    _far_decode(eng, far_in, case, H * W * Cn, want,
                lambda sizes, d_out, d_st: eng.decode_conceal_device(far_in, STRIDE, sizes, B, W, H, Cn, d_out, d_cn, d_map, d_st),
                "decode_conceal_device", streams=streams)
    assert d_cn.cpu().tolist() == [int(m.sum()) for m in maps]
    fm.check_buffer(d_map, [(0, _dev(np.concatenate(maps)))], "the row maps")


def _into_want(dst, n, windows):
    """The whole destination of n pictures: the sentinel, with windows [(f, x, y, picture)] pasted."""
    nbytes = max(f * dst.frame_pitch + (y + p.shape[0] - 1) * dst.row_pitch + (x + p.shape[1]) * dst.pixel_stride
                 for f, x, y, p in windows)
    want = np.full(nbytes + TAIL, SENTINEL, np.uint8)
    for f, x, y, p in windows:
        _paste(want, dst, f, x, y, p)
    return want


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_in_stride_into(eng, far_in, case):
    """decode_into_device from the far input into small padded pictures.  Need: 8.0 GiB."""
    W, H, Cn = case[:3]
    good, fix, pics = _case(*case)
    eng.set_option("fix_t2", int(fix))
    sizes = _place(far_in, [good[f % K] for f in range(B)])
    dst = _padded(W + 24, H + 16, Cn)
    cycle = [(0, 0), (5, 3), (4, 8), (24, 16)]
    org = [cycle[f % 4] for f in range(B - 1)] + [cycle[3]]
    want = _into_want(dst, B, [(f, org[f][0], org[f][1], pics[f % K]) for f in range(B)])
    assert himg_amd.dst_extent(dst, Cn, org, W, H) == want.size - TAIL
    d_dst, d_st = _sentinel(want.size - TAIL), _status(B)
    eng.decode_into_device(far_in, STRIDE, sizes, B, W, H, Cn, d_dst, dst, org, d_st)
    torch.cuda.synchronize()
    _ok(d_st, "decode_into_device", input=STRIDE)
    fm.check_buffer(d_dst, [(0, _dev(want))], "decode_into_device", pitch=dst.frame_pitch)


# ---- A.2: out_stride ------------------------------------------------------------------------------------

ENC = [("front-tokens", 512, 64, 4, {"front": 1, "row_tokens": 1}, True),   # k_front, k_tok and k_emit_tok write
       ("defaults", 72, 40, 4, {}, False)]
ENC_IDS = [c[0] for c in ENC]
QUALS = (10, 50, 90, 100, 0)     # encode_device_q, encode_windows_device: a quality per frame
PICKS = (20, 50, 80, 35, 65)     # the qualities whose sizes / distortions are the budgets / targets


@functools.lru_cache(maxsize=None)
def _enc_picture(k, w, h, ch):
    return np.ascontiguousarray(himg_amd.synth("randtile", k + 1, w, h)[:, :, :ch])


@functools.lru_cache(maxsize=None)
def _enc_stream(k, w, h, ch, q, ycc):
    return np.frombuffer(ol.oracle_encode(_enc_picture(k, w, h, ch), q, ycc), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def _sse_of(k, w, h, ch, q, ycc):
    """test_gpu_target's definition: the oracle's stream at q through the oracle's fixed decode."""
    rc, dec = ol.oracle_decode(_enc_stream(k, w, h, ch, q, ycc), fix_t2=True)
    assert rc == 0
    return tgm.sse(_enc_picture(k, w, h, ch), dec.reshape(h, w, ch))


def _stream_spans(d_out, slot, wants, w, h, ch):
    """The spans of an encode's output: stream f at f * slot; the bytes of a slot between the end of a stream
    and far_model.encoder_clears are unspecified (include/himg_hip.h) and stand for themselves."""
    spans, end = [], fm.encoder_clears(w, h, ch)
    for f, s in enumerate(wants):
        spans.append((f * slot, _dev(s)))
        if s.size < end:
            spans.append((f * slot + s.size, d_out[f * slot + s.size:f * slot + end].clone()))
    return spans


def _far_encode(eng, enc, call, want_q, what):
    """One encode whose frame f goes to f * (2^30 + 256) of a 5 GiB output: call(d_frames, d_out, d_sizes,
    d_status); frame f must be the oracle's stream of picture f % 3 at want_q[f], d_sizes exact, and every
    other byte of the output the sentinel."""
    name, w, h, ch, opts, ycc = enc
    _require(fm.need_far(B * STRIDE, (B - 1) * STRIDE + (1 << 20)))
    for k, v in opts.items():
        eng.set_option(k, v)
    assert STRIDE % 256 == 0 and STRIDE >= himg_amd.max_packed_size(w, h, ch)
    fm.assert_far([f * STRIDE for f in range(B)])
    d_frames = torch.from_numpy(np.stack([_enc_picture(f % K, w, h, ch) for f in range(B)])).cuda()
    d_out = _sentinel(B * STRIDE)
    d_sizes = torch.full((B,), POISON32, dtype=torch.int32, device="cuda")
    d_st = _status(B)
    with _Meter(what + " " + name):
        call(d_frames, d_out, d_sizes, d_st)
    _ok(d_st, what, output=STRIDE)
    wants = [_enc_stream(f % K, w, h, ch, want_q[f], ycc) for f in range(B)]
    _sizes(d_sizes, [s.size for s in wants], what, output=STRIDE)
    # (every stream is longer than what the encoder clears of a slot: all behind a stream is the sentinel)
    assert min(s.size for s in wants) >= fm.encoder_clears(w, h, ch)
    fm.check_buffer(d_out, _stream_spans(d_out, STRIDE, wants, w, h, ch), what + " " + name, pitch=STRIDE)


@pytest.mark.parametrize("enc", ENC, ids=ENC_IDS)
def test_out_stride_encode(eng, enc):
    """encode_device and encode_device_q with out_stride = 2^30 + 256.  Need: 13.0 GiB (the 5 GiB output,
    the module's 4 GiB input, workspace allowance, the comparison's chunks); measured: 9.0 GiB in torch, a
    workspace below 0.01 GiB."""
    name, w, h, ch, opts, ycc = enc
    _far_encode(eng, enc, lambda d_frames, d_out, d_sizes, d_st: eng.encode_device(
        d_frames, B, w, h, ch, ch, 50, ycc, d_out, STRIDE, d_sizes, d_st), [50] * B, "encode_device")
    _far_encode(eng, enc, lambda d_frames, d_out, d_sizes, d_st: eng.encode_device_q(
        d_frames, B, w, h, ch, ch, QUALS, ycc, d_out, STRIDE, d_sizes, d_st), QUALS, "encode_device_q")


@pytest.mark.parametrize("enc", ENC, ids=ENC_IDS)
def test_out_stride_windows(eng, enc):
    """encode_windows_device from small padded source pictures, out_stride = 2^30 + 256.  Need: 13.0 GiB."""
    name, w, h, ch, opts, ycc = enc
    sw, sh = w + 24, h + 16
    rp = sw * ch + 12
    src = himg_amd.src_desc(sw, sh, ch, rp, ((sh - 1) * rp + sw * ch + 15) // 16 * 16)
    cycle = [(0, 0), (5, 3), (24, 16)]
    org = [cycle[f % 3] for f in range(B - 1)] + [cycle[2]]
    buf = _into_want(src, B, [(f, org[f][0], org[f][1], _enc_picture(f % K, w, h, ch)) for f in range(B)])
    assert himg_amd.windows_extent(src, ch, org, w, h) == buf.size - TAIL
    d_src = torch.from_numpy(buf).cuda()
    _far_encode(eng, enc, lambda d_frames, d_out, d_sizes, d_st: eng.encode_windows_device(
        d_src, src, B, ch, org, w, h, QUALS, ycc, d_out, STRIDE, d_sizes, d_st), QUALS, "encode_windows_device")


@pytest.mark.parametrize("enc", ENC, ids=ENC_IDS)
def test_out_stride_budget(eng, enc):
    """encode_budget_device: every frame's budget is its own stream's size at a quality, so budget_model
    gives every frame a result.  Need: 13.0 GiB."""
    name, w, h, ch, opts, ycc = enc
    size = lambda f, q: _enc_stream(f % K, w, h, ch, q, ycc).size   # noqa: E731
    budgets = [size(f, PICKS[f]) for f in range(B)]
    want_q = [bm.search(lambda q, f=f: size(f, q), budgets[f], 0, 100)[0] for f in range(B)]
    assert min(want_q) >= 0
    d_q = torch.full((B,), POISON32, dtype=torch.int32, device="cuda")
    _far_encode(eng, enc, lambda d_frames, d_out, d_sizes, d_st: eng.encode_budget_device(
        d_frames, B, w, h, ch, ch, 0, 100, ycc, budgets, d_out, STRIDE, d_sizes, d_q, d_st), want_q, "encode_budget_device")
    assert d_q.cpu().tolist() == want_q


@pytest.mark.parametrize("enc", ENC, ids=ENC_IDS)
def test_out_stride_target(eng, enc):
    """encode_target_device: every frame's target is its own distortion at a quality (target_model).
    Need: 13.0 GiB."""
    name, w, h, ch, opts, ycc = enc
    sse = lambda f, q: _sse_of(f % K, w, h, ch, q, ycc)   # noqa: E731
    targets = [sse(f, PICKS[f]) for f in range(B)]
    want_q = [tgm.search(lambda q, f=f: sse(f, q), targets[f], 0, 100)[0] for f in range(B)]
    assert min(want_q) >= 0
    d_q = torch.full((B,), POISON32, dtype=torch.int32, device="cuda")
    d_sse = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    _far_encode(eng, enc, lambda d_frames, d_out, d_sizes, d_st: eng.encode_target_device(
        d_frames, B, w, h, ch, ch, 0, 100, ycc, targets, d_out, STRIDE, d_sizes, d_q, d_sse, d_st), want_q,
        "encode_target_device")
    assert d_q.cpu().tolist() == want_q
    assert d_sse.cpu().tolist() == [sse(f, want_q[f]) for f in range(B)]


# ---- A.3 / A.4: frame_pitch and row_pitch of a destination -------------------------------------------------

def _far_pitch(ps):
    return fm.FAR_PITCH + (1 if ps == 3 else 0)       # 3-byte pixels: an odd pitch


def _far_row_pitch(ps):
    return fm.FAR_ROW_PITCH + (1 if ps == 3 else 0)


def _picture_spans(desc, windows):
    """Far pictures: per frame one span, the picture's own bytes (rows row_pitch apart, the sentinel with
    its windows pasted) at f * frame_pitch."""
    one = himg_amd.dst_desc(desc.width, desc.height, desc.pixel_stride, desc.row_pitch, 0)
    spans = []
    for f in sorted({t[0] for t in windows}):
        mine = [(0, x, y, p) for g, x, y, p in windows if g == f]
        local = _into_want(one, 1, mine)
        spans.append((f * desc.frame_pitch, _dev(local[:local.size - TAIL])))
    return spans


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dst_frame_pitch(eng, case):
    """decode_into_device and decode_regions_into_device with dst frame_pitch = 2^30 + 260 (3-byte pixels:
    + 261, odd): picture 4 lies beyond 2^32.  Need: 12.0 GiB (a 4 GiB destination)."""
    W, H, Cn = case[:3]
    good, fix, pics = _case(*case)
    eng.set_option("fix_t2", int(fix))
    d_in, stride = _upload([good[f % K] for f in range(B)])
    sizes = [len(good[f % K]) for f in range(B)]
    Wd, Hd = W + 24, H + 16
    pad = _padded(Wd, Hd, Cn)
    dst = himg_amd.dst_desc(Wd, Hd, Cn, pad.row_pitch, _far_pitch(Cn))
    fm.assert_far([f * dst.frame_pitch for f in range(B)])
    cycle = [(0, 0), (5, 3), (4, 8), (Wd - W, Hd - H)]
    org = [cycle[f % 4] for f in range(B - 1)] + [cycle[3]]
    n = fm.extent(dst.frame_pitch, dst.row_pitch, Cn, org, W, H)
    _require(fm.need_far(n, (B - 1) * STRIDE))
    assert himg_amd.dst_extent(dst, Cn, org, W, H) == n
    d_dst, d_st = _sentinel(n), _status(B)
    assert d_dst.numel() - TAIL == himg_amd.dst_extent(dst, Cn, org, W, H)
    eng.decode_into_device(d_in, stride, sizes, B, W, H, Cn, d_dst, dst, org, d_st)
    torch.cuda.synchronize()
    _ok(d_st, "decode_into_device", destination=dst.frame_pitch)
    fm.check_buffer(d_dst, _picture_spans(dst, [(f, org[f][0], org[f][1], pics[f % K]) for f in range(B)]),
                    "decode_into_device", pitch=dst.frame_pitch)
    del d_dst
    # windows of the frames into windows of the far pictures
    w, h = WIN
    src_org = _origins(W, H, w, h)
    dcycle = [(1, 1), (Wd - w - 1, Hd - h), (7, 3)]
    dst_org = [dcycle[f % 3] for f in range(B - 1)] + [(Wd - w, Hd - h)]
    n = fm.extent(dst.frame_pitch, dst.row_pitch, Cn, dst_org, w, h)
    d_dst, d_st = _sentinel(n), _status(B)
    assert d_dst.numel() - TAIL == himg_amd.dst_extent(dst, Cn, dst_org, w, h)
    eng.decode_regions_into_device(d_in, stride, sizes, B, W, H, Cn, src_org, w, h, d_dst, dst, dst_org, d_st)
    torch.cuda.synchronize()
    _ok(d_st, "decode_regions_into_device", destination=dst.frame_pitch)
    fm.check_buffer(d_dst, _picture_spans(dst, [(f, dst_org[f][0], dst_org[f][1], _crop(pics[f % K], src_org[f] + WIN))
                                                for f in range(B)]), "decode_regions_into_device", pitch=dst.frame_pitch)


ROW_CASES = [(72, 8, 4, True, 50), (72, 8, 3, False, 90)]   # one block row: windows above, across and below row 64
ROW_IDS = ["72x8x4-ycbcr", "72x8x3-rgb"]
ROW_Y = (50, 60, 64)       # rows 50..57 (beyond 2^31), 60..67 (across 2^32), 64..71 (beyond it)
ROW_X = (3, 100, 192)


def _row_spans(rp, ps, windows):
    """Windows of ONE far picture: a span per row."""
    spans = []
    for x, y, p in windows:
        rows = _dev(p).reshape(p.shape[0], -1)
        spans += fm.window_spans(fm.window_base(0, rp, ps, 0, x, y), rows, rp)
    return spans


@pytest.mark.parametrize("case", ROW_CASES, ids=ROW_IDS)
def test_dst_row_pitch(eng, case):
    """One 264 x 72 destination picture (frame_pitch = 0) with row_pitch = 2^26 + 4 (3-byte pixels: + 5):
    y * row_pitch passes 2^32 at y = 64.  decode_into_device puts three 72 x 8 pictures above, across and
    below row 64; decode_regions_into_device three 40 x 7 windows of them.  Need: 12.4 GiB (a 4.4 GiB
    destination)."""
    W, H, Cn = case[:3]
    good, fix, pics = _case(*case)
    eng.set_option("fix_t2", int(fix))
    d_in, stride = _upload(good)
    sizes = [len(s) for s in good]
    rp = _far_row_pitch(Cn)
    dst = himg_amd.dst_desc(264, 72, Cn, rp, 0)
    org = list(zip(ROW_X, ROW_Y))
    fm.assert_far([(y + i) * rp for _, y in org for i in range(H)], whole_beyond=H + 4)
    n = fm.extent(0, rp, Cn, org, W, H)
    _require(fm.need_far(n, (B - 1) * STRIDE))
    d_dst, d_st = _sentinel(n), _status(K)
    assert d_dst.numel() - TAIL == himg_amd.dst_extent(dst, Cn, org, W, H)
    eng.decode_into_device(d_in, stride, sizes, K, W, H, Cn, d_dst, dst, org, d_st)
    torch.cuda.synchronize()
    _ok(d_st, "decode_into_device")
    fm.check_buffer(d_dst, _row_spans(rp, Cn, [(org[f][0], org[f][1], pics[f]) for f in range(K)]),
                    "decode_into_device, row_pitch", pitch=rp)
    del d_dst
    w, h = 40, 7
    src_org = [(3, 1), (72 - w, 0), (8, 1)]
    dst_org = [(1, 51), (264 - w, 61), (7, 65)]
    n = fm.extent(0, rp, Cn, dst_org, w, h)
    d_dst, d_st = _sentinel(n), _status(K)
    assert d_dst.numel() - TAIL == himg_amd.dst_extent(dst, Cn, dst_org, w, h)
    eng.decode_regions_into_device(d_in, stride, sizes, K, W, H, Cn, src_org, w, h, d_dst, dst, dst_org, d_st)
    torch.cuda.synchronize()
    _ok(d_st, "decode_regions_into_device")
    fm.check_buffer(d_dst, _row_spans(rp, Cn, [(dst_org[f][0], dst_org[f][1], _crop(pics[f], src_org[f] + (w, h)))
                                               for f in range(K)]), "decode_regions_into_device, row_pitch", pitch=rp)


# ---- A.5: frame_pitch and row_pitch of a source ---------------------------------------------------------------

def _small_out(n, cap):
    d_out = _sentinel(n * cap)
    d_sizes = torch.full((n,), POISON32, dtype=torch.int32, device="cuda")
    return d_out, d_sizes, _status(n)


def _check_streams(d_out, d_sizes, d_st, cap, wants, what, w, h, ch, pitch=0):
    torch.cuda.synchronize()
    _ok(d_st, what, source=pitch)
    _sizes(d_sizes, [s.size for s in wants], what, source=pitch)
    fm.check_buffer(d_out, _stream_spans(d_out, cap, wants, w, h, ch), what, pitch=cap)


@pytest.mark.parametrize("enc", ENC, ids=ENC_IDS)
def test_src_frame_pitch(eng, enc):
    """encode_windows_device from source pictures frame_pitch = 2^30 + 260 apart: picture 4 lies beyond
    2^32.  The source is 0xA5 but for the pictures pasted in.  Need: 12.0 GiB (a 4 GiB source)."""
    name, w, h, ch, opts, ycc = enc
    for k, v in opts.items():
        eng.set_option(k, v)
    sw, sh = w + 24, h + 16
    src = himg_amd.src_desc(sw, sh, ch, sw * ch + 12, _far_pitch(ch))
    fm.assert_far([f * src.frame_pitch for f in range(B)])
    cycle = [(0, 0), (5, 3), (24, 16)]
    org = [cycle[f % 3] for f in range(B - 1)] + [cycle[2]]
    n = fm.extent(src.frame_pitch, src.row_pitch, ch, org, w, h)
    _require(fm.need_far(n, (B - 1) * STRIDE))
    assert himg_amd.windows_extent(src, ch, org, w, h) == n
    d_src = _sentinel(n)
    for off, t in _picture_spans(src, [(f, org[f][0], org[f][1], _enc_picture(f % K, w, h, ch)) for f in range(B)]):
        d_src[off:off + t.numel()] = t
    cap = himg_amd.max_packed_size(w, h, ch)
    d_out, d_sizes, d_st = _small_out(B, cap)
    eng.encode_windows_device(d_src, src, B, ch, org, w, h, QUALS, ycc, d_out, cap, d_sizes, d_st)
    _check_streams(d_out, d_sizes, d_st, cap, [_enc_stream(f % K, w, h, ch, QUALS[f], ycc) for f in range(B)],
                   "encode_windows_device, frame_pitch, " + name, w, h, ch, pitch=src.frame_pitch)


@pytest.mark.parametrize("ch,ycc", [(4, True), (3, False)], ids=["rgba-ycbcr", "rgb"])
def test_src_row_pitch(eng, ch, ycc):
    """encode_windows_device of three 72 x 8 windows above, across and below row 64 of ONE 264 x 72 source
    picture with row_pitch = 2^26 + 4 (3-byte pixels: + 5).  Need: 12.4 GiB (a 4.4 GiB source)."""
    w, h = 72, 8
    rp = _far_row_pitch(ch)
    src = himg_amd.src_desc(264, 72, ch, rp, 0)
    org = list(zip(ROW_X, ROW_Y))
    fm.assert_far([(y + i) * rp for _, y in org for i in range(h)], whole_beyond=h + 4)
    n = fm.extent(0, rp, ch, org, w, h)
    _require(fm.need_far(n, (B - 1) * STRIDE))
    assert himg_amd.windows_extent(src, ch, org, w, h) == n
    d_src = _sentinel(n)
    for off, t in _row_spans(rp, ch, [(org[f][0], org[f][1], _enc_picture(f, w, h, ch)) for f in range(K)]):
        d_src[off:off + t.numel()] = t
    cap = himg_amd.max_packed_size(w, h, ch)
    d_out, d_sizes, d_st = _small_out(K, cap)
    quals = QUALS[:K]
    eng.encode_windows_device(d_src, src, K, ch, org, w, h, quals, ycc, d_out, cap, d_sizes, d_st)
    _check_streams(d_out, d_sizes, d_st, cap, [_enc_stream(f, w, h, ch, quals[f], ycc) for f in range(K)],
                   "encode_windows_device, row_pitch", w, h, ch)


# ---- B. dense batches whose frame offsets pass 4 GiB ----------------------------------------------------------

S = fm.DENSE
DENSE_YCC = (True, True, False)     # the decodes take each frame's colour lift from its stream
FB = S * S * 4


@functools.lru_cache(maxsize=None)
def _dense():
    """Three oracle streams of distinct 2048 x 2048 RGBA pictures and the oracle's decodes of them."""
    streams = [np.frombuffer(ol.oracle_encode(himg_amd.synth("randtile", k + 1, S, S), 50, DENSE_YCC[k]), np.uint8).copy()
               for k in range(K)]
    pics = [_full(s).reshape(S, S, 4) for s in streams]
    return streams, pics


def _dense_input(streams, pick):
    """The batch on the device: the distinct streams uploaded once, replicated with an index copy."""
    d_few, stride = _upload(streams)
    idx = torch.tensor(pick, dtype=torch.int64, device="cuda")
    return d_few.index_select(0, idx), stride, [len(streams[k]) for k in pick]


def _dense_batch(frame_bytes):
    batch = fm.dense_batch(frame_bytes)
    assert batch * frame_bytes >= fm.WRAP + 2 * frame_bytes > (batch - 1) * frame_bytes
    fm.assert_far([f * frame_bytes for f in range(batch)], whole_beyond=2)
    return batch


def _dense_decode(eng, frame_bytes, wants, call, what, streams=None, pick=None, expected_bytes=None):
    """One dense decode: call(d_in, stride, sizes, batch, d_out, d_status); frame f against wants[f % 3] (or
    wants(f)), the tail against the sentinel."""
    batch = _dense_batch(frame_bytes)
    streams = streams or _dense()[0]
    pick = pick or [f % K for f in range(batch)]
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    _require(fm.need_dense_decode(batch, stride, batch * frame_bytes, expected_bytes or K * frame_bytes))
    d_in, stride, sizes = _dense_input(streams, pick)
    d_out, d_st = _sentinel(batch * frame_bytes), _status(batch)
    with _Meter(what):
        call(d_in, stride, sizes, batch, d_out, d_st)
    _ok(d_st, what, input=stride, output=frame_bytes)
    fm.check_dense(d_out, frame_bytes, batch, wants, what)
    return batch


def test_dense_decode(eng):
    """decode_device, 258 frames of 2048 x 2048 x 4: 4.03 GiB of pictures.  Need: 26.1 GiB (18 GiB of it
    the workspaces a context keeps once the module's dense decodes and encodes have run); measured:
    14.1 GiB in torch at the peak (the module's far input and the comparison's chunk included), 4.8 GiB of
    decode workspace."""
    pics = _dense()[1]
    wants = [_dev(p) for p in pics]
    batch = _dense_decode(eng, FB, wants, lambda d_in, stride, sizes, n, d_out, d_st: eng.decode_device(
        d_in, stride, sizes, n, S, S, 4, d_out, d_st), "decode_device")
    assert batch == 258


def test_dense_tensor_f32(eng):
    """decode_tensor_device, float32, three output channels: 12 bytes per pixel, 88 frames.
    Need: 25.6 GiB; measured: 8.8 GiB in torch."""
    pics = _dense()[1]
    desc = tm.imagenet(tm.F32, 3)
    fb = himg_amd.tensor_bytes(desc, 4, S, S)
    assert fb == S * S * 12
    wants = [_dev(tm.expected(p, desc)) for p in pics]
    batch = _dense_decode(eng, fb, wants, lambda d_in, stride, sizes, n, d_out, d_st: eng.decode_tensor_device(
        d_in, stride, sizes, n, S, S, 4, desc, d_out, d_st), "decode_tensor_device")
    assert batch == 88


REGION = (2040, 2041)   # windows at origins (f % 8, f % 7)


def test_dense_regions(eng):
    """decode_regions_device, 2040 x 2041 windows at (f % 8, f % 7), 260 frames.  Need: 26.1 GiB;
    measured: 9.7 GiB in torch."""
    pics = [torch.from_numpy(p).cuda() for p in _dense()[1]]
    w, h = REGION
    batch = fm.dense_batch(h * w * 4)
    org = [(f % 8, f % 7) for f in range(batch)]
    _dense_decode(eng, h * w * 4, lambda f: pics[f % K][org[f][1]:org[f][1] + h, org[f][0]:org[f][0] + w].contiguous(),
                  lambda d_in, stride, sizes, n, d_out, d_st: eng.decode_regions_device(
                      d_in, stride, sizes, n, S, S, 4, org, w, h, d_out, d_st), "decode_regions_device")


def test_dense_regions_tensor_f32(eng):
    """decode_regions_tensor_device, float32, three output channels, the same windows, 88 frames.
    Need: 25.6 GiB; measured: 8.8 GiB in torch."""
    desc = tm.imagenet(tm.F32, 3)
    tens = [torch.from_numpy(tm.expected(p, desc).view(np.int32)).cuda() for p in _dense()[1]]
    w, h = REGION
    fb = himg_amd.tensor_bytes(desc, 4, w, h)
    batch = fm.dense_batch(fb)
    org = [(f % 8, f % 7) for f in range(batch)]
    _dense_decode(eng, fb, lambda f: tens[f % K][:, org[f][1]:org[f][1] + h, org[f][0]:org[f][0] + w].contiguous().view(torch.uint8),
                  lambda d_in, stride, sizes, n, d_out, d_st: eng.decode_regions_tensor_device(
                      d_in, stride, sizes, n, S, S, 4, org, w, h, desc, d_out, d_st), "decode_regions_tensor_device")


def test_dense_pyramid(eng):
    """decode_pyramid_device, all four levels, 258 frames: level 0 passes 4 GiB, levels 1 to 3 (1.0, 0.25
    and 0.06 GiB) are compared as well.  Need: 27.5 GiB; measured: 11.0 GiB in torch."""
    streams, pics = _dense()
    batch = _dense_batch(FB)
    lv = []
    for s, p in zip(streams, pics):
        one = {0: p, 1: sm.expected(s, 1)[1], 2: sm.expected(s, 2)[1], 3: preview_expected(s)[1]}
        lv.append({k: _dev(v) for k, v in one.items()})
    fbs = [lv[0][k].numel() for k in range(4)]
    assert fbs == [FB, FB // 4, FB // 16, FB // 64]
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    _require(fm.need_dense_decode(batch, stride, batch * sum(fbs) + 3 * TAIL, K * sum(fbs)))
    d_in, stride, sizes = _dense_input(streams, [f % K for f in range(batch)])
    bufs = [_sentinel(batch * fb) for fb in fbs]
    d_st = _status(batch)
    with _Meter("decode_pyramid_device"):
        eng.decode_pyramid_device(d_in, stride, sizes, batch, S, S, 4, himg_amd.pyramid_desc(*bufs), d_st)
    _ok(d_st, "decode_pyramid_device", input=stride, output=FB)
    for k in range(4):
        fm.check_dense(bufs[k], fbs[k], batch, [lv[j][k] for j in range(K)], "pyramid level %d" % k)


def test_dense_prefix(eng):
    """decode_prefix_device with about half of every stream: whole rows exact, the rest from the low-res
    plane, full-size pictures.  258 frames.  Need: 26.1 GiB; measured: 9.7 GiB in torch."""
    streams, _ = _dense()
    models = [pm.Model(s) for s in streams]
    avail = [len(s) // 2 for s in streams]
    want, rows = [], []
    for m, a in zip(models, avail):
        code, k, pic = m.expect(a)
        assert code == pm.OK and 0 < k < m.rows
        want.append(_dev(pic))
        rows.append(k)
    batch = _dense_batch(FB)
    d_rows = torch.full((batch,), -99, dtype=torch.int32, device="cuda")
    _dense_decode(eng, FB, want, lambda d_in, stride, sizes, n, d_out, d_st: eng.decode_prefix_device(
        d_in, stride, [avail[f % K] for f in range(n)], n, S, S, 4, d_out, d_rows, d_st), "decode_prefix_device")
    assert d_rows.cpu().tolist() == [rows[f % K] for f in range(batch)]


def test_dense_conceal(eng):
    """decode_conceal_device, 258 frames, every third one (f % 3 == 0) with a damaged block row that is
    concealed.  Need: 26.1 GiB; measured: 9.7 GiB in torch."""
    streams, pics = _dense()
    r = 100
    o, n = dm.rows_of(streams[0])[1][r]
    bad = streams[0].copy()
    bad[o + n // 2] ^= 1
    bad_pic, bad_map = fm.conceal_one_row(pm.Model(streams[0]), bad, r)
    assert bad_map[r] == 1, "the oracle accepts the flip: choose another"
    batch = _dense_batch(FB)
    rows = S // 8
    wants = [_dev(bad_pic), _dev(pics[1]), _dev(pics[2])]
    d_cn = torch.full((batch,), -99, dtype=torch.int32, device="cuda")
    d_map = _sentinel(batch * rows)
    _dense_decode(eng, FB, wants, lambda d_in, stride, sizes, n_, d_out, d_st: eng.decode_conceal_device(
        d_in, stride, sizes, n_, S, S, 4, d_out, d_cn, d_map, d_st), "decode_conceal_device",
        streams=[bad, streams[1], streams[2]])
    assert d_cn.cpu().tolist() == [1 if f % K == 0 else 0 for f in range(batch)]
    clean = np.zeros(rows, np.uint8)
    fm.check_dense(d_map, rows, batch, [_dev(bad_map), _dev(clean), _dev(clean)], "the row maps")


ENC_Q = (50, 80, 20)   # picture k's quality in the dense encodes


@functools.lru_cache(maxsize=None)
def _dense_sources():
    src = [himg_amd.synth("randtile", k + 1, S, S) for k in range(K)]
    enc = [np.frombuffer(ol.oracle_encode(src[k], ENC_Q[k], True), np.uint8).copy() for k in range(K)]
    return src, enc


def _dense_frames(batch):
    src, _ = _dense_sources()
    d_few = torch.from_numpy(np.stack(src)).cuda().reshape(K, FB)
    return d_few.index_select(0, torch.tensor([f % K for f in range(batch)], dtype=torch.int64, device="cuda"))


def test_dense_encode_q(eng):
    """encode_device_q of 258 frames of 2048 x 2048 x 4 (4.03 GiB of pixels; out_stride = max_packed_size,
    4.09 GiB of output), front = 1, row_tokens = 1: the benchmark's path.  Need: 29.2 GiB; measured:
    12.1 GiB in torch, 12.4 GiB of encode workspace."""
    _, enc = _dense_sources()
    batch = _dense_batch(FB)
    cap = himg_amd.max_packed_size(S, S, 4)
    assert cap % 256 == 0
    fm.assert_far([f * cap for f in range(batch)], whole_beyond=2)
    _require(fm.need_dense_encode(batch, FB, cap))
    eng.set_option("front", 1)
    eng.set_option("row_tokens", 1)
    d_frames = _dense_frames(batch)
    d_out = _sentinel(batch * cap)
    d_sizes = torch.full((batch,), POISON32, dtype=torch.int32, device="cuda")
    d_st = _status(batch)
    with _Meter("encode_device_q"):
        eng.encode_device_q(d_frames, batch, S, S, 4, 4, [ENC_Q[f % K] for f in range(batch)], True, d_out, cap, d_sizes, d_st)
    _ok(d_st, "encode_device_q", input=FB, output=cap)
    _sizes(d_sizes, [enc[f % K].size for f in range(batch)], "encode_device_q", input=FB, output=cap)
    wants = [_dev(s) for s in enc]
    fm.check_buffer(d_out, [(f * cap, wants[f % K]) for f in range(batch)], "encode_device_q", pitch=cap)


def test_dense_encode_sizes_and_sse(eng):
    """encode_sizes_device and encode_sse_device on the same 258 frames: every frame's exact size and
    distortion are the oracle's.  Need: 25.1 GiB; measured: 8.0 GiB in torch, 0.06 GiB more workspace for the
    distortion probe."""
    src, enc = _dense_sources()
    sse = []
    for k in range(K):
        rc, dec = ol.oracle_decode(enc[k], fix_t2=True)
        assert rc == 0
        sse.append(tgm.sse(src[k], dec.reshape(S, S, 4)))
    batch = _dense_batch(FB)
    _require(fm.need_dense_encode(batch, FB, 0))
    eng.set_option("front", 1)
    eng.set_option("row_tokens", 1)
    d_frames = _dense_frames(batch)
    quals = [ENC_Q[f % K] for f in range(batch)]
    d_sizes = torch.full((batch,), POISON32, dtype=torch.int32, device="cuda")
    d_st = _status(batch)
    with _Meter("encode_sizes_device"):
        eng.encode_sizes_device(d_frames, batch, S, S, 4, 4, quals, True, d_sizes, d_st)
    _ok(d_st, "encode_sizes_device", input=FB)
    _sizes(d_sizes, [enc[f % K].size for f in range(batch)], "encode_sizes_device", input=FB)
    d_sse = torch.full((batch,), -1, dtype=torch.int64, device="cuda")
    d_st = _status(batch)
    with _Meter("encode_sse_device"):
        eng.encode_sse_device(d_frames, batch, S, S, 4, 4, quals, True, d_sse, d_st)
    _ok(d_st, "encode_sse_device", input=FB)
    assert d_sse.cpu().tolist() == [sse[f % K] for f in range(batch)]
