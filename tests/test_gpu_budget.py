"""GPU (-m gpu): a quality per frame (encode_device_q), the size-only pass (encode_sizes_device) and
the encode to a byte budget (encode_budget_device, its host forms, chimg -b) against the CPU oracle and
the model of the search (tests/budget_model.py).  Bar: bit-exact streams, exact sizes, the model's
quality for every frame."""
import functools
import subprocess

import numpy as np
import pytest

import himg_amd
from himg_amd import build as hb

import budget_model as bm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

# name, width, height, channels, options, use_ycbcr
CASES = [
    ("pix-one-wavefront", 64, 64, 4, {}, True),
    ("ragged-last-wavefront", 200, 72, 4, {}, True),
    ("front-tokens", 512, 64, 4, {"front": 1, "row_tokens": 1}, True),
    ("front-tokens-spelled-out", 512, 64, 4, {"front": 1, "row_tokens": 2}, True),
    ("three-channels", 264, 80, 3, {}, True),
    ("one-channel", 264, 80, 1, {}, True),
    ("not-multiples-of-8", 100, 52, 4, {}, True),
    ("one-block-row", 64, 8, 4, {}, True),
    ("rgb", 200, 72, 4, {}, False),
    ("front-rgb", 512, 64, 4, {"front": 1}, False),
]
IDS = [c[0] for c in CASES]


def _picture(kind, seed, w, h, ch=4):
    if kind == "flat":
        img = np.full((h, w, 4), 77, np.uint8)
    else:
        img = himg_amd.synth(kind, seed, w, h)
    return np.ascontiguousarray(img[:, :, :ch])


@functools.lru_cache(maxsize=None)
def _oracle(kind, seed, w, h, ch, q, ycc):
    return ol.oracle_encode(_picture(kind, seed, w, h, ch), q, ycc, channels=ch, stride=ch)


@functools.lru_cache(maxsize=None)
def _sizes(kind, seed, w, h, ycc, q0=0, q1=100):
    """The oracle's stream sizes for q0 .. q1 (a dict by quality)."""
    return {q: int(_oracle(kind, seed, w, h, 4, q, ycc).size) for q in range(q0, q1 + 1)}


def _engine(opts):
    eng = himg_amd.Engine(0)
    for k, v in opts.items():
        eng.set_option(k, v)
    return eng


def _buffers(torch, B, cap, fill=0):
    d_out = torch.full((B * cap + 256,), fill, dtype=torch.uint8, device="cuda")
    d_sizes = torch.full((B,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_st = torch.full((B,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    return d_out, d_sizes, d_st


THREE = [("randtile", 1), ("gradn", 2), ("rand", 3)]


@pytest.mark.parametrize("name,w,h,ch,opts,ycc", CASES, ids=IDS)
def test_quality_per_frame_matches_the_oracle(name, w, h, ch, opts, ycc):
    import torch
    eng = _engine(opts)
    frames = np.stack([_picture(k, s, w, h, ch) for k, s in THREE])
    d_frames = torch.from_numpy(frames).cuda()
    cap = himg_amd.max_packed_size(w, h, ch)
    for quals in ((10, 50, 90), (100, 0, 37)):
        d_out, d_sizes, d_st = _buffers(torch, 3, cap)
        eng.encode_device_q(d_frames, 3, w, h, ch, ch, quals, ycc, d_out, cap, d_sizes, d_st)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any(), (name, quals)
        sizes = d_sizes.cpu().numpy()
        out = d_out.cpu().numpy()
        for f, ((k, s), q) in enumerate(zip(THREE, quals)):
            want = _oracle(k, s, w, h, ch, q, ycc)
            assert int(sizes[f]) == want.size, (name, quals, f, int(sizes[f]), want.size)
            assert np.array_equal(out[f * cap: f * cap + want.size], want), (name, quals, f)
        assert not out[3 * cap:].any(), (name, "bytes behind the last frame's out_stride")
    # a quality outside [0, 100] anywhere in the array: HIMG_ERR_ARG, nothing written
    for quals in ((50, 101, 50), (50, 50, -1)):
        d_out, d_sizes, d_st = _buffers(torch, 3, cap, fill=0xa5)
        with pytest.raises(himg_amd.HimgError) as ei:
            eng.encode_device_q(d_frames, 3, w, h, ch, ch, quals, ycc, d_out, cap, d_sizes, d_st)
        assert ei.value.code == himg_amd.HIMG_ERR_ARG
        with pytest.raises(himg_amd.HimgError) as ei:
            eng.encode_sizes_device(d_frames, 3, w, h, ch, ch, quals, ycc, d_sizes, d_st)
        assert ei.value.code == himg_amd.HIMG_ERR_ARG
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0xa5).all() and (d_st.cpu().numpy() == 0x5a5a5a5a).all()
        assert (d_sizes.cpu().numpy() == 0x5a5a5a5a).all()
    eng.close()


SPREAD = (0, 14, 29, 43, 57, 71, 86, 100)


@pytest.mark.parametrize("name,w,h,ch,opts,ycc", CASES, ids=IDS)
def test_sizes_without_a_stream(name, w, h, ch, opts, ycc):
    """Eight frames of one picture at qualities over 0 .. 100: the exact sizes; and an ordinary encode
    on the same context before and after keeps the oracle's bytes (no probe state leaks)."""
    import torch
    eng = _engine(opts)
    B = len(SPREAD)
    one = _picture("randtile", 1, w, h, ch)
    d_frames = torch.from_numpy(np.stack([one] * B)).cuda()
    cap = himg_amd.max_packed_size(w, h, ch)
    want50 = _oracle("randtile", 1, w, h, ch, 50, ycc)

    def plain():
        d_out, d_sizes, d_st = _buffers(torch, B, cap)
        eng.encode_device(d_frames, B, w, h, ch, ch, 50, ycc, d_out, cap, d_sizes, d_st)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any()
        out = d_out.cpu().numpy()
        for f in range(B):
            assert int(d_sizes[f]) == want50.size and np.array_equal(out[f * cap: f * cap + want50.size], want50), (name, f)

    plain()
    d_sizes = torch.full((B + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_st = torch.full((B,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    eng.encode_sizes_device(d_frames, B, w, h, ch, ch, SPREAD, ycc, d_sizes, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    got = d_sizes.cpu().numpy()
    assert [int(x) for x in got[:B]] == [int(_oracle("randtile", 1, w, h, ch, q, ycc).size) for q in SPREAD], name
    assert (got[B:] == 0x5a5a5a5a).all()
    plain()
    eng.close()


SIX = [("randtile", 1), ("randtile", 2), ("gradn", 1), ("gradn", 2), ("rand", 3), ("flat", 0)]


def _six_budgets(w, h):
    """Per-frame budgets from the oracle's sizes: size(20), size(50) - 1, size(80), one at an inversion
    (of the second gradn frame), size(0) - 1 (fails), 2^30."""
    s = [_sizes(k, sd, w, h, True) for k, sd in SIX]
    inv = [q for q in bm.inversions([s[3][q] for q in range(101)]) if s[3][q] - 1 >= s[3][0]]
    assert inv, "the gradn frame has no inversion above its size at quality 0"
    q_inv = inv[len(inv) // 2]
    return s, [s[0][20], s[1][50] - 1, s[2][80], s[3][q_inv] - 1, s[4][0] - 1, 1 << 30]


@pytest.mark.parametrize("w,h,opts,qmin,qmax", [
    (64, 64, {}, 0, 100),
    (512, 64, {"front": 1, "row_tokens": 1}, 0, 100),
    (64, 64, {}, 50, 50),
    (64, 64, {}, 40, 60),
], ids=["64x64", "512x64-front-tokens", "one-probe", "range-40-60"])
def test_budget_device(w, h, opts, qmin, qmax):
    import torch
    s, budgets = _six_budgets(w, h)
    want_q = [bm.search(lambda q, f=f: s[f][q], budgets[f], qmin, qmax)[0] for f in range(6)]
    if (qmin, qmax) == (0, 100):
        # (from the model, before the GPU is looked at: otherwise the test shows nothing about per-frame state)
        assert len(set(want_q)) >= 4 and -1 in want_q, want_q
        assert want_q[4] == -1 and min(q for q in want_q if q >= 0) < max(want_q)
    assert -1 in want_q and max(want_q) >= 0, want_q
    eng = _engine(opts)
    B = 6
    frames = np.stack([_picture(k, sd, w, h) for k, sd in SIX])
    d_frames = torch.from_numpy(frames).cuda()
    cap = himg_amd.max_packed_size(w, h, 4)
    d_out, d_sizes, d_st = _buffers(torch, B, cap, fill=0xc3)
    d_q = torch.full((B + 4,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    eng.encode_budget_device(d_frames, B, w, h, 4, 4, qmin, qmax, True, budgets, d_out, cap, d_sizes, d_q, d_st)
    torch.cuda.synchronize()
    got_q = d_q.cpu().numpy()
    assert [int(x) for x in got_q[:B]] == want_q, (got_q, want_q)
    assert (got_q[B:] == 0x5a5a5a5a).all(), "canary behind d_quality"
    sizes, st, out = d_sizes.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy()
    assert (out[B * cap:] == 0xc3).all(), "canary behind the last frame's out_stride"
    for f, (k, sd) in enumerate(SIX):
        if want_q[f] < 0:
            assert int(sizes[f]) == 0 and int(st[f]) == himg_amd.HIMG_ERR_CAPACITY, (f, sizes[f], st[f])
            continue
        want = _oracle(k, sd, w, h, 4, want_q[f], True)
        assert int(st[f]) == 0 and int(sizes[f]) == want.size <= budgets[f], (f, st[f], sizes[f], want.size, budgets[f])
        assert np.array_equal(out[f * cap: f * cap + want.size], want), (f, want_q[f])
    eng.close()


def test_budget_host_forms():
    w, h = 64, 64
    s, budgets = _six_budgets(w, h)
    eng = himg_amd.Engine(0)
    # one frame, pageable and pinned
    img = _picture("gradn", 1, w, h)
    pinned = himg_amd.pinned_empty(img.nbytes).reshape(img.shape)
    pinned[...] = img
    for src in (img, pinned):
        for b in (s[2][80], s[2][33] - 1, 1 << 30, s[2][0]):
            want_q = bm.search(lambda q: s[2][q], b, 0, 100)[0]
            stream, q = eng.encode_budget(src, b)
            assert q == want_q and stream.size <= b and np.array_equal(stream, _oracle("gradn", 1, w, h, 4, q, True)), (b, q)
        stream, q = eng.encode_budget(src, s[2][50], qmin=40, qmax=60)
        assert q == bm.search(lambda x: s[2][x], s[2][50], 40, 60)[0]
        assert np.array_equal(stream, _oracle("gradn", 1, w, h, 4, q, True))
    with pytest.raises(himg_amd.HimgError) as ei:
        eng.encode_budget(img, s[2][0] - 1)
    assert ei.value.code == himg_amd.HIMG_ERR_CAPACITY and ei.value.quality == -1
    with pytest.raises(himg_amd.HimgError) as ei:
        eng.encode_budget(img, 1 << 20, qmin=60, qmax=40)
    assert ei.value.code == himg_amd.HIMG_ERR_ARG
    # the capacity protocol: a too-small dst, then fetch_last
    import ctypes as C
    L = himg_amd.lib()
    n, q = C.c_size_t(), C.c_int()
    small = np.zeros(16, np.uint8)
    rc = L.himg_hip_encode_budget_to(eng._ctx, img.ctypes.data, w, h, 4, 4, 0, 100, 1, s[2][80], small.ctypes.data,
                                     small.nbytes, C.byref(n), C.byref(q))
    want = _oracle("gradn", 1, w, h, 4, q.value, True)
    assert rc == himg_amd.HIMG_ERR_CAPACITY and q.value == bm.search(lambda x: s[2][x], s[2][80], 0, 100)[0]
    assert n.value == want.size and not small.any()
    full = np.zeros(n.value, np.uint8)
    assert L.himg_hip_fetch_last(eng._ctx, full.ctypes.data, full.nbytes, C.byref(n)) == 0 and np.array_equal(full, want)
    # a batch of five of which one fails
    five = [0, 1, 4, 2, 3]
    streams, quals, rc = eng.encode_budget_batch([_picture(*SIX[f], w, h) for f in five], [budgets[f] for f in five])
    assert rc == himg_amd.HIMG_ERR_CAPACITY
    for i, f in enumerate(five):
        want_q = bm.search(lambda x, f=f: s[f][x], budgets[f], 0, 100)[0]
        assert quals[i] == want_q, (i, f, quals[i], want_q)
        if want_q < 0:
            assert f == 4 and streams[i].size == 0
        else:
            assert np.array_equal(streams[i], _oracle(*SIX[f], w, h, 4, want_q, True)), (i, f)
    eng.close()


def test_batches_by_launch_size():
    """128 frames of 1024 x 512 (8192 block rows: the token stream and k_front by launch size), a
    quality per frame, then each frame within its own q50 size out of 40 .. 60."""
    import torch
    eng = himg_amd.Engine(0)
    w, h, B = 1024, 512, 128
    frames = np.stack([himg_amd.synth("randtile", sd, w, h) for sd in range(B)])
    d_frames = torch.from_numpy(frames).cuda()
    cap = himg_amd.max_packed_size(w, h, 4)
    d_out = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_st = torch.ones(B, dtype=torch.int32, device="cuda")
    quals = [(30, 50, 70, 90)[f % 4] for f in range(B)]
    check = (0, 1, B // 2, B - 1)
    eng.profile(True)
    eng.encode_device_q(d_frames, B, w, h, 4, 4, quals, True, d_out, cap, d_sizes, d_st)
    torch.cuda.synchronize()
    stages = eng.profile_read()
    assert "k_tok" in stages and "k_emit_tok" in stages, sorted(stages)
    eng.profile(False)
    assert not d_st.cpu().numpy().any()
    sizes = d_sizes.cpu().numpy()
    for f in check:
        want = ol.oracle_encode(frames[f], quals[f], True)
        assert int(sizes[f]) == want.size and np.array_equal(d_out[f, : want.size].cpu().numpy(), want), f
    # budgets: every frame's own size at quality 50
    eng.encode_sizes_device(d_frames, B, w, h, 4, 4, [50] * B, True, d_sizes, d_st)
    torch.cuda.synchronize()
    budgets = [int(x) for x in d_sizes.cpu().numpy()]
    d_q = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    eng.encode_budget_device(d_frames, B, w, h, 4, 4, 40, 60, True, budgets, d_out, cap, d_sizes, d_q, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    sizes, got_q = d_sizes.cpu().numpy(), d_q.cpu().numpy()
    assert (sizes <= np.array(budgets)).all() and (got_q >= 40).all() and (got_q <= 60).all()
    for f in check:
        streams = {q: ol.oracle_encode(frames[f], q, True) for q in range(40, 61)}
        assert budgets[f] == streams[50].size, f
        want_q = bm.search(lambda q: streams[q].size, budgets[f], 40, 60)[0]
        assert int(got_q[f]) == want_q, (f, int(got_q[f]), want_q)
        want = streams[want_q]
        assert int(sizes[f]) == want.size and np.array_equal(d_out[f, : want.size].cpu().numpy(), want), f
    eng.close()


def test_chimg_budget(tmp_path):
    from test_cli import _freeimage_order, _write_pnm
    chimg = hb.build_cli()[0]
    w, h = 64, 64
    img = np.ascontiguousarray(himg_amd.synth("gradn", 1, w, h)[:, :, :3])
    src, dst = str(tmp_path / "in.ppm"), str(tmp_path / "o.himg")
    _write_pnm(src, img)
    fi = _freeimage_order(img)
    sizes = {q: int(ol.oracle_encode(fi, q, True, channels=3, stride=3).size) for q in range(101)}
    for flags, qmax, budget in (([], 100, sizes[70]), (["-q", "60"], 60, sizes[70]), (["-rgb"], 100, None)):
        ycc = "-rgb" not in flags
        if budget is None:
            budget = int(ol.oracle_encode(fi, 40, False, channels=3, stride=3).size)
        r = subprocess.run([chimg, *flags, "-b", str(budget), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert lines[-2].startswith("Quality: ") and lines[-1].startswith("Compressed size: "), r.stdout
        q = int(lines[-2].split()[1])
        size_of = (lambda x: sizes[x]) if ycc else (lambda x: int(ol.oracle_encode(fi, x, False, channels=3, stride=3).size))
        assert q == bm.search(size_of, budget, 0, qmax)[0]
        want = ol.oracle_encode(fi, q, ycc, channels=3, stride=3)
        got = np.fromfile(dst, np.uint8)
        assert got.size <= budget and int(lines[-1].split()[2]) == got.size and np.array_equal(got, want)
    r = subprocess.run([chimg, "-b", str(sizes[0] - 1), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 255 and "does not fit" in r.stderr
