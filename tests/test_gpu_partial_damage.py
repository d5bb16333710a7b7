"""GPU (-m gpu): the decodes that promise to look at only part of a stream, on DAMAGED streams, against an
expectation the CPU oracle gives (tests/damage_model.py: the bytes a form sees respliced into a complete
stream) -- verdict and pixels, no tolerance.  The corpus is seeded (damage_model.streams): per base, payload
bit flips (P), a flipped bit in a row's size header (H) and, for the prefix decode, a flipped bit in the head
(C).  tests/test_damage_model_host.py proves the model's premises and counts what the corpus reaches.

Forms: decode_region (host), decode_region_device, decode_regions_device (an origin per frame; both count
kernels on the 256 x 72 base), the host batch, decode_scaled_regions_device at both scales,
decode_regions_tensor_device, decode_regions_into_device, decode_prefix_device and decode_prefix (host).
Every stream of a base, class and form goes in one device launch, between sentinels: a rejected frame's
neighbours are exactly their own expectation."""
import functools

import numpy as np
import pytest
import torch

import damage_model as dm
import himg_amd
import tensor_model as tm
from test_gpu_regions import _batch

pytestmark = pytest.mark.gpu

ST_SHORT = 5      # a frame's status word for a prefix below its first row header (HIMG_ERR_CAPACITY)
ST_UNSUPPORTED = 3
SENTINEL = 0x5A
PH = [(b.name, cls) for b in dm.BASES for cls in "PH" if not (cls == "H" and b.H <= 8)]
NAMES = [b.name for b in dm.BASES]
WAVES = {dm.BASES[0].name: (-1, 0, 1)}


@pytest.fixture
def eng(engine):
    def use(name):
        engine.set_option("fix_t2", int(dm.BASE[name].fix))
        return engine
    engine.set_option("count_wave", -1)
    yield use
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)


def _upload(streams):
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.zeros((n, stride), np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = s
    return torch.from_numpy(buf).cuda(), stride, [len(s) for s in streams]


def _outputs(n, frame_bytes):
    d_out = torch.full((n * frame_bytes + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    return d_out, d_st


def _fetch(d_out, d_st, n, frame_bytes):
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n * frame_bytes:] == SENTINEL).all()
    return d_st.cpu().numpy(), out[:n * frame_bytes].reshape(n, frame_bytes)


@functools.lru_cache(maxsize=None)
def _want(name, cls, which):
    """[(code, crop or None, X)] per stream: which = 'rects', 'origins' or 'one'."""
    b, m = dm.BASE[name], dm.good_model(name)
    ss = dm.streams(name, cls)
    if which == "rects":
        rr = dm.rects(name, cls)
    elif which == "origins":
        rr = [o + b.win for o in dm.origins(name, cls)]
    else:
        rr = [dm.one_rect(name)] * len(ss)
    return rr, [dm.expect_region(m.packed, s.bad, r, b.fix) for s, r in zip(ss, rr)]


def _judge_windows(want, st, out, shape, what):
    """Every frame of a launch against its expectation: the status, and an accepted frame's bytes."""
    n_acc = n_rej = 0
    for f, (code, crop, _) in enumerate(want):
        if code == dm.OK:
            assert st[f] == 0, (what, f, st[f])
            assert np.array_equal(out[f].reshape(shape), crop), (what, f)
            n_acc += 1
        else:
            assert st[f] & 15 == 4, (what, f, st[f])
            n_rej += 1
    assert n_acc >= 5 and n_rej >= 5, (what, n_acc, n_rej)


@pytest.mark.parametrize("name,cls", PH)
def test_region_host(eng, name, cls):
    e = eng(name)
    rr, want = _want(name, cls, "rects")
    n_acc = n_rej = 0
    for i, (s, r, (code, crop, _)) in enumerate(zip(dm.streams(name, cls), rr, want)):
        try:
            got, rc = e.decode_region(s.bad, *r), 0
        except himg_amd.HimgError as err:
            got, rc = None, err.code
        assert rc == code, (i, r, s.rows, rc, code)
        if code == dm.OK:
            assert np.array_equal(got, crop), (i, r, s.rows)
            n_acc += 1
        else:
            n_rej += 1
    assert n_acc >= 5 and n_rej >= 5, (n_acc, n_rej)


@pytest.mark.parametrize("name,cls", PH)
def test_region_device_one_rectangle(eng, name, cls):
    e, b = eng(name), dm.BASE[name]
    rr, want = _want(name, cls, "one")
    x, y, w, h = rr[0]
    d_in, stride, sizes = _upload([s.bad for s in dm.streams(name, cls)])
    n = len(sizes)
    for wave in WAVES.get(name, (-1,)):
        e.set_option("count_wave", wave)
        d_out, d_st = _outputs(n, h * w * b.C)
        e.decode_region_device(d_in, stride, sizes, n, b.W, b.H, b.C, x, y, w, h, d_out, d_st)
        st, out = _fetch(d_out, d_st, n, h * w * b.C)
        _judge_windows(want, st, out, (h, w, b.C), (name, cls, wave))


@pytest.mark.parametrize("name,cls", PH)
def test_regions_device_an_origin_per_frame(eng, name, cls):
    e, b = eng(name), dm.BASE[name]
    rr, want = _want(name, cls, "origins")
    w, h = b.win
    org = np.array([r[:2] for r in rr], np.int32)
    d_in, stride, sizes = _upload([s.bad for s in dm.streams(name, cls)])
    n = len(sizes)
    for wave in WAVES.get(name, (-1,)):
        e.set_option("count_wave", wave)
        d_out, d_st = _outputs(n, h * w * b.C)
        e.decode_regions_device(d_in, stride, sizes, n, b.W, b.H, b.C, org, w, h, d_out, d_st)
        st, out = _fetch(d_out, d_st, n, h * w * b.C)
        _judge_windows(want, st, out, (h, w, b.C), (name, cls, wave))


@pytest.mark.parametrize("name,cls", PH)
def test_host_batch(eng, name, cls):
    """himg_hip_decode_regions_batch: each frame's code is its own -- a rejected frame reports no geometry and
    stops nobody; the call returns the first error."""
    e, b = eng(name), dm.BASE[name]
    rr, want = _want(name, cls, "origins")
    rc, msg, dims, outs = _batch(e, [s.bad for s in dm.streams(name, cls)], rr)
    assert rc == himg_amd.HIMG_ERR_FORMAT, (rc, msg)
    for f, ((code, crop, _), r) in enumerate(zip(want, rr)):
        if code == dm.OK:
            assert dims[f] == (r[2], r[3], b.C), (f, dims[f])
            assert np.array_equal(outs[f].reshape(crop.shape), crop), f
        else:
            assert dims[f] == (0, 0, 0), (f, dims[f])
    assert sum(c == dm.OK for c, _, _ in want) >= 5


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("name,cls", PH)
def test_scaled_regions_device(eng, name, cls, scale):
    """The verdict is that of the covered full-resolution rectangle; the pixels are the crop of
    scaled_model.expected of the respliced stream."""
    e, b, m = eng(name), dm.BASE[name], dm.good_model(name)
    F = 1 << scale
    ws, hs = max(1, b.win[0] >> scale), max(1, b.win[1] >> scale)
    org = np.array([(x >> scale, y >> scale) for x, y in dm.origins(name, cls)], np.int32)
    ss = dm.streams(name, cls)
    want = []
    for s, (xs, ys) in zip(ss, org):
        y0, y1 = F * int(ys), min(F * int(ys) + F * hs, b.H)
        code, _, X = dm.expect_rows(m.packed, s.bad, range(y0 // 8, (y1 + 7) // 8), b.fix)
        crop = dm.scaled(X, scale, b.fix)[ys:ys + hs, xs:xs + ws] if code == dm.OK else None
        want.append((code, crop, X))
    d_in, stride, sizes = _upload([s.bad for s in ss])
    n = len(sizes)
    d_out, d_st = _outputs(n, hs * ws * b.C)
    e.decode_scaled_regions_device(d_in, stride, sizes, n, b.W, b.H, b.C, scale, org, ws, hs, d_out, d_st)
    st, out = _fetch(d_out, d_st, n, hs * ws * b.C)
    _judge_windows(want, st, out, (hs, ws, b.C), (name, cls, scale))


@pytest.mark.parametrize("name", NAMES)
def test_tensor_windows(eng, name):
    """decode_regions_tensor_device, class P: the region's verdict per frame, the crop through tensor_model."""
    e, b = eng(name), dm.BASE[name]
    rr, want = _want(name, "P", "origins")
    w, h = b.win
    desc = tm.imagenet(tm.F16, min(b.C, 3))
    co = desc.out_channels
    fb = co * h * w * tm.ELEM[tm.F16]
    d_in, stride, sizes = _upload([s.bad for s in dm.streams(name, "P")])
    n = len(sizes)
    d_out, d_st = _outputs(n, fb)
    e.decode_regions_tensor_device(d_in, stride, sizes, n, b.W, b.H, b.C, np.array([r[:2] for r in rr], np.int32), w, h,
                                   desc, d_out, d_st)
    st, out = _fetch(d_out, d_st, n, fb)
    bits = [(c, tm.expected(crop, desc) if c == dm.OK else None, X) for c, crop, X in want]
    _judge_windows(bits, st, out.view(np.uint16), (co, h, w), name)


@pytest.mark.parametrize("name", NAMES)
def test_pitched_windows(eng, name):
    """decode_regions_into_device, class P: padded rows, a wider pixel, an origin per destination picture.
    Nothing outside a window is written, a rejected frame's included."""
    e, b = eng(name), dm.BASE[name]
    rr, want = _want(name, "P", "origins")
    w, h = b.win
    ps = 2 if b.C == 1 else 4
    dw, dh = w + 5, h + 3
    pitch = dw * ps + 8
    dst = himg_amd.dst_desc(dw, dh, ps, pitch)
    rng = np.random.default_rng(dm.SEED + 9)
    dorg = np.stack([rng.integers(0, 6, len(rr)), rng.integers(0, 4, len(rr))], axis=1).astype(np.int32)
    d_in, stride, sizes = _upload([s.bad for s in dm.streams(name, "P")])
    n = len(sizes)
    d_out, d_st = _outputs(n, dh * pitch)
    e.decode_regions_into_device(d_in, stride, sizes, n, b.W, b.H, b.C, np.array([r[:2] for r in rr], np.int32), w, h,
                                 d_out, dst, dorg, d_st)
    st, out = _fetch(d_out, d_st, n, dh * pitch)
    n_rej = 0
    for f, (code, crop, _) in enumerate(want):
        pic = out[f].reshape(dh, pitch)
        dx, dy = (int(v) for v in dorg[f])
        mask = np.zeros((dh, pitch), bool)
        for c in range(b.C):
            mask[dy:dy + h, dx * ps + c:(dx + w) * ps:ps] = True
        if code == dm.OK:
            assert st[f] == 0, (f, st[f])
            assert np.array_equal(pic[mask].reshape(h, w, b.C), crop), f
        else:
            assert st[f] & 15 == 4, (f, st[f])
            n_rej += 1
        assert (pic[~mask] == SENTINEL).all(), f
    assert 5 <= n_rej <= n - 5


def _prefix(e, b, frames):
    """decode_prefix_device over frames [(stream, avail)]: frame f holds stream[:avail], junk behind.
    (status, rows, pictures)."""
    n = len(frames)
    stride = (max(max(a for _, a in frames), 4) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5, np.uint8)
    for f, (s, a) in enumerate(frames):
        buf[f, :a] = s[:a]
    fb = b.H * b.W * b.C
    d_out, d_st = _outputs(n, fb)
    d_rows = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    e.decode_prefix_device(torch.from_numpy(buf).cuda(), stride, [a for _, a in frames], n, b.W, b.H, b.C, d_out, d_rows, d_st)
    st, out = _fetch(d_out, d_st, n, fb)
    return st, d_rows.cpu().numpy(), out.reshape(n, b.H, b.W, b.C)


def _judge_prefix(f, want, st, rows, out, what):
    code, k, pic = want
    if code == dm.CAPACITY:
        assert st[f] == ST_SHORT and rows[f] == -1, (what, f, st[f], rows[f])
        assert (out[f] == SENTINEL).all(), (what, f)
    elif code == dm.FORMAT:
        assert st[f] & 15 == 4 and rows[f] == -1, (what, f, st[f], rows[f])
    else:
        assert st[f] == 0 and rows[f] == k, (what, f, st[f], rows[f], k)
        assert np.array_equal(out[f], pic), (what, f, k)


@pytest.mark.parametrize("name,cls", PH)
def test_prefix_device(eng, name, cls):
    e, b, m = eng(name), dm.BASE[name], dm.good_model(name)
    frames = [(s.bad, a) for s, av in zip(dm.streams(name, cls), dm.avails(name, cls)) for a in av]
    want = [dm.expect_prefix(m, s, a, b.fix) for s, a in frames]
    st, rows, out = _prefix(e, b, frames)
    for f in range(len(frames)):
        _judge_prefix(f, want[f], st, rows, out, (name, cls, frames[f][1]))
    codes = [c for c, _, _ in want]
    assert codes.count(dm.OK) >= 5 and codes.count(dm.FORMAT) >= 5


@pytest.mark.parametrize("name", NAMES)
def test_prefix_device_head_damage(eng, name):
    """Class C (damage_model.head_cases).  Where the engine answers HIMG_ERR_UNSUPPORTED to a prefix that holds
    the whole head (a tree with a branch deeper than 32: the one deviation include/himg_hip.h lists), the full
    decode of the stream must answer the same; those cases and the ones whose pixels are not judged stay
    below 20 % of the class."""
    e, b = eng(name), dm.BASE[name]
    frames, want = [], []
    for s, (rc, cases) in zip(dm.streams(name, "C"), dm.head_cases(name)):
        for a, kind, code, k, pic in cases:
            frames.append((s.bad, a))
            want.append((kind, code, k, pic))
    st, rows, out = _prefix(e, b, frames)
    loose = 0
    for f, (kind, code, k, pic) in enumerate(want):
        what = (name, f, frames[f][1], kind)
        if kind == "open":
            loose += 1
        elif kind == "fres" and code == dm.OK:
            assert st[f] == 0 and rows[f] == 0, (what, st[f], rows[f])
            loose += 1
        elif code != dm.CAPACITY and st[f] & 15 == ST_UNSUPPORTED:
            # (where the oracle accepts -- or, the tree being malformed further on, where the walk says FORMAT:
            # the engine reports the first failure in the order of the reference's tree walk)
            with pytest.raises(himg_amd.HimgError) as err:
                e.decode(frames[f][0])
            assert err.value.code == himg_amd.HIMG_ERR_UNSUPPORTED and rows[f] == -1, what
            loose += 1
        else:
            _judge_prefix(f, (code, k, pic), st, rows, out, what)
    assert 5 * loose <= len(want), (loose, len(want))


@pytest.mark.parametrize("name", NAMES)
def test_prefix_host_sample(eng, name):
    """decode_prefix on a host slice of exactly the bytes present, every seventh case of each class."""
    e, b, m = eng(name), dm.BASE[name], dm.good_model(name)
    cases = []
    for cls in "PH":
        cases += [(s.bad, a, dm.expect_prefix(m, s.bad, a, b.fix)) for s, av in zip(dm.streams(name, cls), dm.avails(name, cls)) for a in av]
    for s, (rc, cs) in zip(dm.streams(name, "C"), dm.head_cases(name)):
        cases += [(s.bad, a, (code, k, pic)) for a, kind, code, k, pic in cs if kind in ("walk", "head") or (kind == "model" and rc == 0)]
    codes = set()
    for bad, a, (code, k, pic) in cases[::7]:
        try:
            got, gk = e.decode_prefix(bad[:a].copy())
            rc = 0
        except himg_amd.HimgError as err:
            got, gk, rc = None, -1, err.code
        if rc == himg_amd.HIMG_ERR_UNSUPPORTED and code != dm.CAPACITY:   # (a tree deeper than 32, as above)
            with pytest.raises(himg_amd.HimgError) as err:
                e.decode(bad)
            assert err.value.code == rc
            continue
        assert rc == code and gk == k, (a, rc, code, gk, k)
        if code == dm.OK:
            assert np.array_equal(got, pic), (a, k)
        codes.add(code)
    assert codes == {dm.OK, dm.FORMAT, dm.CAPACITY}
