"""GPU (-m gpu): the distortion probe (encode_sse_device) and the encode to a distortion target
(encode_target_device, its host forms, chimg -p) against the CPU oracle -- sse(q) is the squared
difference between the source and the oracle's fixed decode of the oracle's stream -- and the model
of the search (tests/target_model.py).  Bar: exact integers, bit-exact streams, the model's quality
and status for every frame."""
import functools
import subprocess

import numpy as np
import pytest

import himg_amd
from himg_amd import build as hb

import oracle_lib as ol
import target_model as tm

pytestmark = pytest.mark.gpu

# name, width, height, channels, pixel stride, options, use_ycbcr
CASES = [
    ("pix-one-wavefront", 64, 64, 4, 4, {}, True),
    ("ragged-last-wavefront", 200, 72, 4, 4, {}, True),
    ("front-tokens", 512, 64, 4, 4, {"front": 1, "row_tokens": 1}, True),
    ("front-tokens-spelled-out", 512, 64, 4, 4, {"front": 1, "row_tokens": 2}, True),
    ("three-channels", 264, 80, 3, 3, {}, True),
    ("one-channel", 264, 80, 1, 1, {}, True),
    ("not-multiples-of-8", 100, 52, 4, 4, {}, True),
    ("one-block-row", 64, 8, 4, 4, {}, True),
    ("rgb", 200, 72, 4, 4, {}, False),
    ("front-rgb", 512, 64, 4, 4, {"front": 1}, False),
    ("three-of-four-bytes", 264, 80, 3, 4, {}, True),
    ("one-tile", 8, 8, 4, 4, {}, True),
    ("one-ragged-tile", 9, 9, 4, 4, {}, True),
    ("run-time-strides", 4352, 16, 4, 4, {}, True),
]
IDS = [c[0] for c in CASES]
POISON64 = 0x5a5a5a5a5a5a5a5a
POISON32 = 0x5a5a5a5a


def _picture(kind, seed, w, h, stride=4):
    """(h, w, stride) bytes; the bytes behind the counted channels are the generator's own (not zero)."""
    if kind == "flat":
        img = np.full((h, w, 4), 77, np.uint8)
    else:
        img = himg_amd.synth(kind, seed, w, h)
    return np.ascontiguousarray(img[:, :, :stride])


@functools.lru_cache(maxsize=None)
def _stream(kind, seed, w, h, ch, stride, q, ycc):
    return ol.oracle_encode(_picture(kind, seed, w, h, stride), q, ycc, channels=ch, stride=stride)


@functools.lru_cache(maxsize=None)
def _sse(kind, seed, w, h, ch, stride, q, ycc):
    """The definition: the oracle's stream at q through the oracle's fixed decode, against the counted bytes."""
    rc, dec = ol.oracle_decode(_stream(kind, seed, w, h, ch, stride, q, ycc), fix_t2=True)
    assert rc == 0, (kind, seed, w, h, q, rc)
    return tm.sse(_picture(kind, seed, w, h, stride)[:, :, :ch], dec.reshape(h, w, ch))


def _curve(kind, seed, w, h, ch, stride, ycc):
    return [_sse(kind, seed, w, h, ch, stride, q, ycc) for q in range(101)]


def _engine(opts):
    eng = himg_amd.Engine(0)
    for k, v in opts.items():
        eng.set_option(k, v)
    return eng


def _probe(torch, eng, d_frames, B, w, h, ch, stride, quals, ycc):
    d_sse = torch.full((B + 2,), POISON64, dtype=torch.int64, device="cuda")
    d_st = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
    eng.encode_sse_device(d_frames, B, w, h, stride, ch, quals, ycc, d_sse, d_st)
    torch.cuda.synchronize()
    sse, st = d_sse.cpu().numpy(), d_st.cpu().numpy()
    assert (sse[B:] == POISON64).all() and (st[B:] == POISON32).all(), "canaries behind d_sse / d_status"
    assert not st[:B].any(), st[:B]
    return [int(x) for x in sse[:B]]


THREE = [("randtile", 1), ("gradn", 2), ("rand", 3)]


@pytest.mark.parametrize("name,w,h,ch,stride,opts,ycc", CASES, ids=IDS)
def test_sse_matches_the_oracle(name, w, h, ch, stride, opts, ycc):
    import torch
    eng = _engine(opts)
    d_frames = torch.from_numpy(np.stack([_picture(k, s, w, h, stride) for k, s in THREE])).cuda()
    for quals in ((10, 50, 90), (100, 0, 37)):
        want = [_sse(k, s, w, h, ch, stride, q, ycc) for (k, s), q in zip(THREE, quals)]
        got = _probe(torch, eng, d_frames, 3, w, h, ch, stride, quals, ycc)
        print(name, quals, "sse", got, "oracle", want)
        assert got == want, (name, quals, got, want)
    # a quality outside [0, 100] anywhere in the array: HIMG_ERR_ARG, nothing written
    for quals in ((50, 101, 50), (50, 50, -1)):
        d_sse = torch.full((3,), POISON64, dtype=torch.int64, device="cuda")
        d_st = torch.full((3,), POISON32, dtype=torch.int32, device="cuda")
        with pytest.raises(himg_amd.HimgError) as ei:
            eng.encode_sse_device(d_frames, 3, w, h, stride, ch, quals, ycc, d_sse, d_st)
        assert ei.value.code == himg_amd.HIMG_ERR_ARG
        torch.cuda.synchronize()
        assert (d_sse.cpu().numpy() == POISON64).all() and (d_st.cpu().numpy() == POISON32).all()
    eng.close()


SPREAD = (0, 14, 29, 43, 57, 71, 86, 100)


@pytest.mark.parametrize("name,w,h,ch,stride,opts,ycc", CASES, ids=IDS)
def test_sse_of_eight_frames_and_no_leak(name, w, h, ch, stride, opts, ycc):
    """Eight frames of one picture at qualities over 0 .. 100; an ordinary encode on the same context
    before and after keeps the oracle's bytes (no probe state leaks)."""
    import torch
    eng = _engine(opts)
    B = len(SPREAD)
    d_frames = torch.from_numpy(np.stack([_picture("randtile", 1, w, h, stride)] * B)).cuda()
    cap = himg_amd.max_packed_size(w, h, ch)
    want50 = _stream("randtile", 1, w, h, ch, stride, 50, ycc)

    def plain():
        d_out = torch.zeros((B * cap,), dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros((B,), dtype=torch.int32, device="cuda")
        d_st = torch.ones((B,), dtype=torch.int32, device="cuda")
        eng.encode_device(d_frames, B, w, h, stride, ch, 50, ycc, d_out, cap, d_sizes, d_st)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any()
        out = d_out.cpu().numpy()
        for f in range(B):
            assert int(d_sizes[f]) == want50.size and np.array_equal(out[f * cap: f * cap + want50.size], want50), (name, f)

    plain()
    got = _probe(torch, eng, d_frames, B, w, h, ch, stride, SPREAD, ycc)
    assert got == [_sse("randtile", 1, w, h, ch, stride, q, ycc) for q in SPREAD], name
    plain()
    eng.close()


def test_sse_of_a_flat_picture():
    import torch
    eng = himg_amd.Engine(0)
    w, h = 72, 40
    d_frames = torch.from_numpy(np.stack([_picture("flat", 0, w, h)] * 3)).cuda()
    quals = (0, 50, 100)
    assert _probe(torch, eng, d_frames, 3, w, h, 4, 4, quals, True) == [_sse("flat", 0, w, h, 4, 4, q, True) for q in quals]
    eng.close()


def test_sse_above_32_bits():
    """rand 1024 x 256 at quality 0: 5 232 949 770 on the oracle, more than a 32-bit sum holds."""
    import torch
    w, h = 1024, 256
    want = _sse("rand", 3, w, h, 4, 4, 0, True)
    assert want == 5232949770 and want > 1 << 32
    eng = himg_amd.Engine(0)
    d_frames = torch.from_numpy(np.stack([_picture("rand", 3, w, h)] * 2)).cuda()
    got = _probe(torch, eng, d_frames, 2, w, h, 4, 4, (0, 0), True)
    assert got == [want, want], got
    eng.close()


FORBIDDEN = ("k_tok", "k_tree", "k_span_bits", "k_sizes", "k_emit", "k_padfix", "k_lres_summary",
             # the decoder's
             "k_dec", "k_tile_inv", "k_lres_unpredict", "k_lres_spec", "k_lres_fix", "k_lres_write", "k_lres_finish",
             "k_lres_preview", "k_row_", "k_region")


@pytest.mark.parametrize("w,h,opts,front", [(512, 64, {"front": 1}, True), (200, 72, {}, False)], ids=["front", "three-kernels"])
def test_the_kernels_that_ran(w, h, opts, front):
    import torch
    eng = _engine(opts)
    d_frames = torch.from_numpy(np.stack([_picture("randtile", 1, w, h)] * 2)).cuda()
    _probe(torch, eng, d_frames, 2, w, h, 4, 4, (50, 50), True)   # (tables and workspace: not in the profile)
    eng.profile(True)
    eng.profile_reset()
    d_sse = torch.zeros((2,), dtype=torch.int64, device="cuda")
    eng.encode_sse_device(d_frames, 2, w, h, 4, 4, (30, 70), True, d_sse, None)
    torch.cuda.synchronize()
    stages = sorted(eng.profile_read())
    eng.profile(False)
    print(stages)
    assert any("k_sse" in s for s in stages), stages
    assert any("k_lres_predict" in s for s in stages), stages
    assert any("k_front" in s for s in stages) == front, stages
    assert any("k_lowres_avg" in s for s in stages) == (not front), stages
    for s in stages:
        assert not any(bad in s for bad in FORBIDDEN), (s, stages)
    assert [int(x) for x in d_sse.cpu().numpy()] == [_sse("randtile", 1, w, h, 4, 4, q, True) for q in (30, 70)]
    eng.close()


@pytest.mark.parametrize("name,w,h,ch,stride,opts,ycc", [CASES[i] for i in (0, 1, 4, 6, 9)], ids=[IDS[i] for i in (0, 1, 4, 6, 9)])
def test_cross_check_on_the_device(name, w, h, ch, stride, opts, ycc):
    """encode_device_q, decode_device with HIMG_OPT_FIX_T2 on, the squared difference in torch: d_sse."""
    import torch
    eng = _engine(opts)
    eng.set_option("fix_t2", 1)
    quals = (5, 50, 95)
    src = np.stack([_picture(k, s, w, h, stride) for k, s in THREE])
    d_frames = torch.from_numpy(src).cuda()
    cap = himg_amd.max_packed_size(w, h, ch)
    d_out = torch.zeros((3 * cap,), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros((3,), dtype=torch.int32, device="cuda")
    d_st = torch.ones((3,), dtype=torch.int32, device="cuda")
    eng.encode_device_q(d_frames, 3, w, h, stride, ch, quals, ycc, d_out, cap, d_sizes, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    d_pix = torch.zeros((3, h, w, ch), dtype=torch.uint8, device="cuda")
    eng.decode_device(d_out, cap, d_sizes.cpu().numpy().astype(np.uint32), 3, w, h, ch, d_pix, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    diff = d_frames[:, :, :, :ch].to(torch.int64) - d_pix.to(torch.int64)
    want = [int(x) for x in (diff * diff).sum(dim=(1, 2, 3)).cpu().numpy()]
    assert _probe(torch, eng, d_frames, 3, w, h, ch, stride, quals, ycc) == want, name
    eng.close()


def _eight_targets(s, qmax):
    return [s[10], s[50], s[90], s[qmax], s[qmax] - 1, min(s) - 1, 1 << 63, 0]


def _check_target_launch(torch, eng, pics, curves, targets, w, h, ch, stride, ycc, qmin, qmax, tag):
    """One encode_target_device launch against the model: frame f is picture pics[f] (kind, seed) with
    the oracle's curve curves[f] and the target targets[f]."""
    B = len(pics)
    want_q = [tm.search(lambda q, f=f: curves[f][q], targets[f], qmin, qmax)[0] for f in range(B)]
    d_frames = torch.from_numpy(np.stack([_picture(k, sd, w, h, stride) for k, sd in pics])).cuda()
    cap = himg_amd.max_packed_size(w, h, ch)
    d_out = torch.full((B * cap + 256,), 0xc3, dtype=torch.uint8, device="cuda")
    d_sizes = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
    d_st = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
    d_q = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
    d_sse = torch.full((B + 2,), POISON64, dtype=torch.int64, device="cuda")
    eng.encode_target_device(d_frames, B, w, h, stride, ch, qmin, qmax, ycc, targets, d_out, cap, d_sizes, d_q, d_sse, d_st)
    torch.cuda.synchronize()
    got_q, sizes, st = d_q.cpu().numpy(), d_sizes.cpu().numpy(), d_st.cpu().numpy()
    sse, out = d_sse.cpu().numpy(), d_out.cpu().numpy()
    print(tag, (qmin, qmax), "quality", [int(x) for x in got_q[:B]], "model", want_q)
    assert [int(x) for x in got_q[:B]] == want_q, (tag, qmin, qmax, got_q[:B], want_q)
    for a, p in ((got_q, POISON32), (sizes, POISON32), (st, POISON32), (sse, POISON64)):
        assert (a[B:] == p).all(), (tag, "canary behind a per-frame array")
    assert (out[B * cap:] == 0xc3).all(), (tag, "canary behind the last frame's out_stride")
    for f, (k, sd) in enumerate(pics):
        if want_q[f] < 0:
            assert int(sizes[f]) == 0 and int(st[f]) == himg_amd.HIMG_ERR_TARGET, (tag, f, sizes[f], st[f])
            continue
        want = _stream(k, sd, w, h, ch, stride, want_q[f], ycc)
        assert int(st[f]) == 0 and int(sizes[f]) == want.size, (tag, f, st[f], sizes[f], want.size)
        assert np.array_equal(out[f * cap: f * cap + want.size], want), (tag, f, want_q[f])
        assert int(sse[f]) == curves[f][want_q[f]] <= targets[f], (tag, f, int(sse[f]), curves[f][want_q[f]], targets[f])
    return want_q


@pytest.mark.parametrize("name,w,h,ch,stride,opts,ycc", CASES, ids=IDS)
def test_target_device(name, w, h, ch, stride, opts, ycc):
    import torch
    s = _curve("randtile", 1, w, h, ch, stride, ycc)
    eng = _engine(opts)
    pics = [("randtile", 1)] * 8
    for qmin, qmax in ((0, 100), (20, 80), (37, 37)):
        targets = _eight_targets(s, qmax)
        want_q = _check_target_launch(torch, eng, pics, [s] * 8, targets, w, h, ch, stride, ycc, qmin, qmax, name)
        # (from the model: the launch holds failures and results side by side)
        assert want_q[5] == -1 and want_q[7] == -1 and want_q[3] >= 0 and want_q[6] == qmin, want_q
    eng.close()


def test_target_more_frames_than_a_step_workgroup():
    """65 frames of 64 x 8, three pictures in turn, a target per frame from its own curve."""
    import torch
    w, h, B = 64, 8, 65
    eng = himg_amd.Engine(0)
    pics = [THREE[f % 3] for f in range(B)]
    curves = {p: _curve(p[0], p[1], w, h, 4, 4, True) for p in THREE}
    targets = [curves[pics[f]][(f * 7) % 101] - (1 if f % 5 == 4 else 0) for f in range(B)]
    targets[64] = min(curves[pics[64]]) - 1   # (the lane of the second workgroup fails)
    want_q = _check_target_launch(torch, eng, pics, [curves[p] for p in pics], targets, w, h, 4, 4, True, 0, 100, "65-frames")
    assert want_q[64] == -1 and len(set(want_q)) >= 8, want_q
    eng.close()


def test_target_host_forms():
    import ctypes as C
    w, h = 64, 64
    eng = himg_amd.Engine(0)
    s = _curve("gradn", 1, w, h, 4, 4, True)
    img = _picture("gradn", 1, w, h)
    pinned = himg_amd.pinned_empty(img.nbytes).reshape(img.shape)
    pinned[...] = img
    for src in (img, pinned):
        for t in (s[80], s[33] - 1, 1 << 63, s[100]):
            want_q = tm.search(lambda q: s[q], t, 0, 100)[0]
            stream, q, sse = eng.encode_target(src, t)
            assert q == want_q and sse == s[q] <= t, (t, q, want_q, sse)
            assert np.array_equal(stream, _stream("gradn", 1, w, h, 4, 4, q, True)), (t, q)
        stream, q, sse = eng.encode_target(src, s[50], qmin=40, qmax=60)
        assert q == tm.search(lambda x: s[x], s[50], 40, 60)[0] and sse == s[q]
        assert np.array_equal(stream, _stream("gradn", 1, w, h, 4, 4, q, True))
    with pytest.raises(himg_amd.HimgError) as ei:
        eng.encode_target(img, min(s) - 1)
    assert ei.value.code == himg_amd.HIMG_ERR_TARGET and ei.value.quality == -1 and ei.value.sse == s[100]
    with pytest.raises(himg_amd.HimgError) as ei:
        eng.encode_target(img, 1 << 40, qmin=60, qmax=40)
    assert ei.value.code == himg_amd.HIMG_ERR_ARG
    # a PSNR as the target
    t30 = himg_amd.psnr_to_sse(30.0, w, h, 4)
    stream, q, sse = eng.encode_target(img, t30)
    assert q == tm.search(lambda x: s[x], t30, 0, 100)[0] and sse == s[q] <= t30
    rc, dec = ol.oracle_decode(stream, fix_t2=True)
    assert rc == 0 and himg_amd.psnr(img, dec.reshape(img.shape)) >= 30.0
    # the capacity protocol: a too-small dst, then fetch_last
    L = himg_amd.lib()
    n, q, sse = C.c_size_t(), C.c_int(), C.c_uint64()
    small = np.zeros(16, np.uint8)
    rc = L.himg_hip_encode_target_to(eng._ctx, img.ctypes.data, w, h, 4, 4, 0, 100, 1, s[80], small.ctypes.data,
                                     small.nbytes, C.byref(n), C.byref(q), C.byref(sse))
    assert rc == himg_amd.HIMG_ERR_CAPACITY and q.value == tm.search(lambda x: s[x], s[80], 0, 100)[0]
    want = _stream("gradn", 1, w, h, 4, 4, q.value, True)
    assert n.value == want.size and not small.any() and sse.value == s[q.value]
    full = np.zeros(n.value, np.uint8)
    assert L.himg_hip_fetch_last(eng._ctx, full.ctypes.data, full.nbytes, C.byref(n)) == 0 and np.array_equal(full, want)
    # a batch of five of which one fails
    pics = [("randtile", 1), ("gradn", 1), ("rand", 3), ("gradn", 2), ("randtile", 2)]
    curves = [_curve(k, sd, w, h, 4, 4, True) for k, sd in pics]
    targets = [curves[0][20], curves[1][50] - 1, min(curves[2]) - 1, curves[3][80], 1 << 63]
    streams, quals, sses, rc = eng.encode_target_batch([_picture(k, sd, w, h) for k, sd in pics], targets)
    assert rc == himg_amd.HIMG_ERR_TARGET
    for i, (k, sd) in enumerate(pics):
        want_q = tm.search(lambda x, i=i: curves[i][x], targets[i], 0, 100)[0]
        assert quals[i] == want_q, (i, quals[i], want_q)
        if want_q < 0:
            assert i == 2 and streams[i].size == 0
        else:
            assert sses[i] == curves[i][want_q] <= targets[i], (i, sses[i])
            assert np.array_equal(streams[i], _stream(k, sd, w, h, 4, 4, want_q, True)), i
    eng.close()


def test_chimg_target(tmp_path):
    from test_cli import _freeimage_order, _write_pnm
    chimg = hb.build_cli()[0]
    w, h = 64, 64
    img = np.ascontiguousarray(himg_amd.synth("gradn", 1, w, h)[:, :, :3])
    src, dst = str(tmp_path / "in.ppm"), str(tmp_path / "o.himg")
    _write_pnm(src, img)
    fi = _freeimage_order(img)

    def curve(ycc):
        out = []
        for q in range(101):
            rc, dec = ol.oracle_decode(ol.oracle_encode(fi, q, ycc, channels=3, stride=3), fix_t2=True)
            assert rc == 0
            out.append(tm.sse(fi, dec.reshape(fi.shape)))
        return out

    for flags, qmax in (([], 100), (["-q", "60"], 60), (["-rgb"], 100)):
        ycc = "-rgb" not in flags
        s = curve(ycc)
        r = subprocess.run([chimg, *flags, "-p", "30", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert lines[-3].startswith("Quality: ") and lines[-2].startswith("PSNR: ") and lines[-1].startswith("Compressed size: "), r.stdout
        q = int(lines[-3].split()[1])
        assert q == tm.search(lambda x: s[x], himg_amd.psnr_to_sse(30.0, w, h, 3), 0, qmax)[0]
        want = ol.oracle_encode(fi, q, ycc, channels=3, stride=3)
        got = np.fromfile(dst, np.uint8)
        assert int(lines[-1].split()[2]) == got.size and np.array_equal(got, want)
        reached = 10.0 * np.log10(255.0 * 255.0 * fi.size / s[q])
        assert reached >= 30.0 and abs(float(lines[-2].split()[1]) - reached) <= 0.006, (lines[-2], reached)
    r = subprocess.run([chimg, "-p", "99", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "does not reach 99 dB" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([chimg, "-p", "30", "-b", "4000", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.startswith("-b and -p exclude each other\nUsage:")
