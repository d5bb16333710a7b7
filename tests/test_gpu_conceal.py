"""GPU (-m gpu): the concealing decode -- decode_conceal_device (a batch in HBM) and decode_conceal (a host
stream) -- against tests/conceal_model.py, byte for byte: status, d_concealed, the row map and the picture.
The corpus is damage_model's; tests/test_conceal_host.py proves the model's premises and asserts the floors
that keep these tests from being vacuous.  No tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conceal_model as cm
import damage_model as dm
import himg_amd
import oracle_lib as ol

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
ST_UNSUPPORTED = 3
PH = [(b.name, cls) for b in dm.BASES for cls in "PH" if not (cls == "H" and b.H <= 8)]
NAMES = [b.name for b in dm.BASES]


@pytest.fixture
def eng(engine):
    def use(name_or_fix):
        fix = dm.BASE[name_or_fix].fix if isinstance(name_or_fix, str) else name_or_fix
        engine.set_option("fix_t2", int(fix))
        return engine
    engine.set_option("count_wave", -1)
    yield use
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)


def _upload(streams, poison=None):
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    if poison is None:
        buf = np.zeros((n, stride), np.uint8)
    else:
        buf = np.random.default_rng(poison).integers(0, 256, (n, stride), dtype=np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = s
    return torch.from_numpy(buf).cuda(), stride, [len(s) for s in streams]


def _conceal(e, streams, W, H, Cn, rowmap=True, poison=None):
    """decode_conceal_device of one launch: (status, concealed, row maps or None, pictures)."""
    d_in, stride, sizes = _upload(streams, poison)
    n, rows, fb = len(streams), (H + 7) // 8, H * W * Cn
    d_out = torch.full((n * fb + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    d_cn = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    d_map = torch.full((n * rows + 16,), SENTINEL, dtype=torch.uint8, device="cuda") if rowmap else None
    e.decode_conceal_device(d_in, stride, sizes, n, W, H, Cn, d_out, d_cn, d_map, d_st)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n * fb:] == SENTINEL).all()
    maps = None
    if rowmap:
        maps = d_map.cpu().numpy()
        assert (maps[n * rows:] == SENTINEL).all()
        maps = maps[:n * rows].reshape(n, rows)
    return d_st.cpu().numpy(), d_cn.cpu().numpy(), maps, out[:n * fb].reshape(n, H, W, Cn)


def _full(e, streams, W, H, Cn):
    """decode_device of one launch: (status, pictures)."""
    d_in, stride, sizes = _upload(streams)
    n, fb = len(streams), H * W * Cn
    d_out = torch.full((n * fb,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    e.decode_device(d_in, stride, sizes, n, W, H, Cn, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy().reshape(n, H, W, Cn)


def _pic(model):
    return model.full.reshape(model.H, model.W, model.C)


def _judge(want, st, cn, maps, out, what):
    for f, (pic, rowmap) in enumerate(want):
        assert st[f] == 0 and cn[f] == int(rowmap.sum()), (what, f, st[f], cn[f], int(rowmap.sum()))
        if maps is not None:
            assert np.array_equal(maps[f], rowmap), (what, f, maps[f], rowmap)
        assert np.array_equal(out[f], pic.reshape(out[f].shape)), (what, f, rowmap)


def _with_good(name, cls):
    """The base's damaged streams with the good stream in every eighth slot: (streams, [(picture, rowmap)])."""
    m = dm.good_model(name)
    streams, want = [], []
    good = (_pic(m), np.zeros(m.rows, np.uint8))
    for s, w in zip(dm.streams(name, cls), cm.corpus(name, cls)):
        if len(streams) % 8 == 0:
            streams.append(m.packed)
            want.append(good)
        streams.append(s.bad)
        want.append(w)
    return streams, want


@pytest.mark.parametrize("name,cls", PH)
def test_corpus(eng, name, cls):
    e, b = eng(name), dm.BASE[name]
    streams, want = _with_good(name, cls)
    st, cn, maps, out = _conceal(e, streams, b.W, b.H, b.C)
    _judge(want, st, cn, maps, out, (name, cls))
    assert sum(int(w[1].sum()) > 0 for w in want) >= 40


@functools.lru_cache(maxsize=None)
def _clean(W, H):
    img = himg_amd.synth("randtile", 2, W, H)
    s = np.frombuffer(ol.oracle_encode(img, 50, True), np.uint8).copy()
    rc, pix = ol.oracle_decode(s, fix_t2=True)
    assert rc == 0
    return s, pix


def test_clean_bases_are_decode_device(eng):
    for name in NAMES:
        e, b, m = eng(name), dm.BASE[name], dm.good_model(name)
        st, cn, maps, out = _conceal(e, [m.packed] * 3, b.W, b.H, b.C)
        st0, out0 = _full(e, [m.packed] * 3, b.W, b.H, b.C)
        assert (st == 0).all() and (st0 == 0).all() and (cn == 0).all() and not maps.any(), (name, st, cn)
        assert np.array_equal(out, out0) and np.array_equal(out[0], _pic(m)), name


@pytest.mark.parametrize("W,H", [(4096, 16), (1920, 24), (256, 72), (16384, 16)])
def test_clean_row_kernel_forms_are_decode_device(eng, W, H):
    """The <512> and <240> row kernels, the generic one, and rows wider than the LDS.  (Frames this flat are
    smaller than a block row's symbols: trap T2, decoded under HIMG_OPT_FIX_T2.)"""
    e = eng(True)
    s, pix = _clean(W, H)
    st, cn, maps, out = _conceal(e, [s, s], W, H, 4)
    st0, out0 = _full(e, [s, s], W, H, 4)
    assert (st == 0).all() and (st0 == 0).all() and (cn == 0).all() and not maps.any(), (st, st0, cn)
    assert np.array_equal(out, out0) and np.array_equal(out[1], pix)


@pytest.mark.parametrize("wave", [-1, 0, 1])
def test_neighbours_in_the_persistent_row_kernel(eng, wave):
    """256 x 72, 320 frames -- more than the row kernel has workgroups: every third frame damaged.  (Both count
    kernels forced as well, on fewer frames.)"""
    name = "randtile256x72"
    e, b, m = eng(name), dm.BASE[name], dm.good_model(name)
    e.set_option("count_wave", wave)
    bad = [(s.bad, w) for cls in "PH" for s, w in zip(dm.streams(name, cls), cm.corpus(name, cls))]
    good = (_pic(m), np.zeros(m.rows, np.uint8))
    streams, want = [], []
    for f in range(320 if wave == -1 else 150):
        if f % 3 == 1:
            s, w = bad[(f // 3 * 7) % len(bad)]
            streams.append(s)
            want.append(w)
        else:
            streams.append(m.packed)
            want.append(good)
    assert sum(int(w[1].sum()) > 0 for w in want) >= (40 if wave == -1 else 20)
    st, cn, maps, out = _conceal(e, streams, b.W, b.H, b.C)
    assert (st == 0).all()
    _judge(want, st, cn, maps, out, name)


@pytest.mark.parametrize("name", NAMES)
def test_head_damage(eng, name):
    """Class C.  The oracle accepts: its picture, nothing concealed.  It rejects in a head stage: decode_device's
    status, concealed = -1.  It rejects in the FRES stage: the tree failed in the parse (decode_device's status,
    -1) or rows were rejected under an altered tree (status 0, at least one row concealed) -- pixels not judged.
    Those, and the engine's HIMG_ERR_UNSUPPORTED answers (a tree deeper than 32: include/himg_hip.h), stay
    below 20 % of the class."""
    e, b = eng(name), dm.BASE[name]
    streams = [s.bad for s in dm.streams(name, "C")]
    st, cn, maps, out = _conceal(e, streams, b.W, b.H, b.C)
    st0, _ = _full(e, streams, b.W, b.H, b.C)
    loose = n_acc = n_head = 0
    for f, s in enumerate(streams):
        rc, pix = ol.oracle_decode(s, fix_t2=b.fix)
        what = (name, f, rc, st[f], st0[f], cn[f])
        if st0[f] & 15 == ST_UNSUPPORTED:
            assert st[f] == st0[f] and cn[f] == -1, what
            loose += 1
        elif rc == 0:
            assert st[f] == 0 and st0[f] == 0 and cn[f] == 0 and not maps[f].any(), what
            assert np.array_equal(out[f], pix.reshape(out[f].shape)), what
            n_acc += 1
        elif -6 <= rc <= -1:
            assert st0[f] != 0 and st[f] == st0[f] and cn[f] == -1, what
            n_head += 1
        else:
            assert st0[f] != 0, what
            assert (st[f] == 0 and cn[f] >= 1 and cn[f] == int(maps[f].sum())) or (st[f] == st0[f] and cn[f] == -1), what
            loose += 1
    assert 5 * loose <= len(streams), (loose, len(streams))
    assert n_acc >= 20 and n_head >= 5, (n_acc, n_head)


@pytest.mark.parametrize("name,cls", [("randtile256x72", "P"), ("rand4096x24q100", "H"), ("randtile40x8", "P")])
def test_nothing_behind_a_stream_is_read(eng, name, cls):
    e, b = eng(name), dm.BASE[name]
    streams, want = _with_good(name, cls)
    a = _conceal(e, streams, b.W, b.H, b.C)
    p = _conceal(e, streams, b.W, b.H, b.C, poison=7)
    for x, y in zip(a, p):
        assert np.array_equal(x, y)
    _judge(want, *p, (name, cls, "poisoned"))


@pytest.mark.parametrize("name", ["gradn61x27", "randtile4352x24"])
def test_without_a_row_map(eng, name):
    e, b = eng(name), dm.BASE[name]
    streams, want = _with_good(name, "P")
    st, cn, maps, out = _conceal(e, streams, b.W, b.H, b.C, rowmap=False)
    assert maps is None
    _judge(want, st, cn, None, out, name)


def test_host_entry(eng):
    for name in ("randtile256x72", "gradn61x27", "grad40x40q0", "randtile40x8"):
        e, b, m = eng(name), dm.BASE[name], dm.good_model(name)
        for cls in "PH":
            for s, (pic, rowmap) in list(zip(dm.streams(name, cls), cm.corpus(name, cls)))[::40]:
                got, gmap = e.decode_conceal(s.bad)
                assert gmap.dtype == bool and np.array_equal(gmap, rowmap.astype(bool)), (name, cls, s.rows)
                assert np.array_equal(got, pic.reshape(got.shape)), (name, cls, s.rows)
        got, gmap = e.decode_conceal(m.packed)
        assert not gmap.any() and np.array_equal(got, e.decode(m.packed))
        # head damage: decode()'s error
        head = next(s.bad for s in dm.streams(name, "C") if -6 <= ol.oracle_decode(s.bad, fix_t2=b.fix)[0] <= -1)
        with pytest.raises(himg_amd.HimgError) as e0:
            e.decode(head)
        with pytest.raises(himg_amd.HimgError) as e1:
            e.decode_conceal(head)
        assert e1.value.code == e0.value.code
        assert str(e1.value).split(": ", 1)[1] == str(e0.value).split(": ", 1)[1]


def test_host_capacity_protocol_and_arguments(eng):
    name = "randtile256x72"
    e, b, m = eng(name), dm.BASE[name], dm.good_model(name)
    L, ctx = himg_amd.lib(), e._ctx
    i = next(i for i, (_, rowmap) in enumerate(cm.corpus(name, "P")) if 0 < rowmap.sum() < m.rows)
    s, (pic, rowmap) = dm.streams(name, "P")[i].bad, cm.corpus(name, "P")[i]
    w, h, c, n = C.c_int(), C.c_int(), C.c_int(), C.c_int(-7)
    geom = (C.byref(w), C.byref(h), C.byref(c))
    gmap = np.full(m.rows + 4, SENTINEL, np.uint8)
    # no destination: HIMG_ERR_CAPACITY with the geometry, the count and the map; fetch_last has the picture
    rc = L.himg_hip_decode_conceal_to(ctx, s.ctypes.data, s.nbytes, None, 0, *geom, gmap.ctypes.data, m.rows, C.byref(n))
    assert rc == himg_amd.HIMG_ERR_CAPACITY and (w.value, h.value, c.value) == (b.W, b.H, b.C)
    assert n.value == int(rowmap.sum()) and np.array_equal(gmap[:m.rows], rowmap) and (gmap[m.rows:] == SENTINEL).all()
    got, size = np.zeros(pic.size, np.uint8), C.c_size_t()
    assert L.himg_hip_fetch_last(ctx, got.ctypes.data, got.nbytes, C.byref(size)) == 0 and size.value == pic.size
    assert np.array_equal(got, pic.ravel())
    # a destination one byte short: the same
    rc = L.himg_hip_decode_conceal_to(ctx, s.ctypes.data, s.nbytes, got.ctypes.data, got.nbytes - 1, *geom, None, 0, C.byref(n))
    assert rc == himg_amd.HIMG_ERR_CAPACITY and n.value == int(rowmap.sum())
    # a NULL row map
    got[:] = 0
    rc = L.himg_hip_decode_conceal_to(ctx, s.ctypes.data, s.nbytes, got.ctypes.data, got.nbytes, *geom, None, 0, C.byref(n))
    assert rc == 0 and n.value == int(rowmap.sum()) and np.array_equal(got, pic.ravel())
    # a short row map: HIMG_ERR_CAPACITY, nothing written
    gmap[:] = SENTINEL
    rc = L.himg_hip_decode_conceal_to(ctx, s.ctypes.data, s.nbytes, got.ctypes.data, got.nbytes, *geom, gmap.ctypes.data,
                                      m.rows - 1, C.byref(n))
    assert rc == himg_amd.HIMG_ERR_CAPACITY and n.value == -1 and (gmap == SENTINEL).all()
    # null pointers
    ARG = himg_amd.HIMG_ERR_ARG
    assert L.himg_hip_decode_conceal_to(None, s.ctypes.data, s.nbytes, None, 0, *geom, None, 0, C.byref(n)) == ARG
    assert L.himg_hip_decode_conceal_to(ctx, None, s.nbytes, None, 0, *geom, None, 0, C.byref(n)) == ARG
    assert L.himg_hip_decode_conceal_to(ctx, s.ctypes.data, s.nbytes, None, 0, None, geom[1], geom[2], None, 0, C.byref(n)) == ARG
    assert L.himg_hip_decode_conceal_to(ctx, s.ctypes.data, s.nbytes, None, 0, *geom, None, 0, None) == ARG
    # the device entry
    d_in, stride, sizes = _upload([s])
    d_out = torch.full((pic.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((1,), -99, dtype=torch.int32, device="cuda")
    d_cn = torch.full((1,), -99, dtype=torch.int32, device="cuda")
    args = [d_in, stride, sizes, 1, b.W, b.H, b.C, d_out, d_cn, None, d_st]
    for k, v in ((0, None), (2, None), (7, None), (8, None), (10, None), (3, 0), (3, -1)):
        bad = list(args)
        bad[k] = v
        with pytest.raises(himg_amd.HimgError) as err:
            e.decode_conceal_device(*bad)
        assert err.value.code == ARG, k
    with pytest.raises(himg_amd.HimgError) as err:   # in_stride does not cover the stream
        e.decode_conceal_device(d_in, 256, [300], 1, b.W, b.H, b.C, d_out, d_cn, None, d_st)
    assert err.value.code == ARG
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all() and int(d_st[0]) == -99 and int(d_cn[0]) == -99   # nothing launched
