"""GPU (-m gpu): the extreme pictures of tests/extreme_pictures.py -- the saturating code +-127,
forward coefficients above the pixel stage's 8 192-entry magnitude table, chroma at 0 and 255, values
on the rounding boundary (what each kind reaches: tests/golden/extreme_reach.json, proved on the CPU by
tests/test_extreme_host.py) -- through every kernel form, against the CPU oracle and the numpy models
fed by the oracle's traces.  Bar: bit-exact; streams the reference rejects (trap T2) are tested for the
rejection and, with HIMG_OPT_FIX_T2, against the oracle's fixed mode."""
import functools
import os

import numpy as np
import pytest
import torch

import himg_amd
import extreme_pictures as xp
import oracle_lib as ol
import scaled_model as sm
import target_model as tgm
import tensor_model as tnm
from test_gpu_preview import expected as preview_expected
from test_gpu_region import _device as region_device
from test_gpu_regions import _upload
from test_gpu_tensor import _expected as tensor_expected, _regions_tensor, _same, _tensor

pytestmark = pytest.mark.gpu

# name, width, height, channels, pixel stride, options: the smallest shapes that select each form of the
# encoder's pixel stage (as in test_gpu_budget.py / test_gpu_target.py)
SHAPES = [
    ("pix-one-wavefront", 64, 64, 4, 4, {}),                           # k_pix_fwd, one wavefront
    ("ragged-last-wavefront", 200, 72, 4, 4, {}),
    ("front", 512, 64, 4, 4, {"front": 1}),                            # k_front
    ("front-tokens", 512, 64, 4, 4, {"front": 1, "row_tokens": 1}),
    ("three-channels", 136, 72, 3, 3, {}),                             # the generic k_tile_fwd
    ("ragged-tiles", 100, 52, 4, 4, {}),
    ("three-of-four-bytes", 264, 80, 3, 4, {}),
]
SHAPE_IDS = [s[0] for s in SHAPES]
MODES = [pytest.param(True, id="ycbcr"), pytest.param(False, id="rgb")]
QUALITIES = (100, 90, 50, 10, 0)
KINDS = xp.KINDS
MIXED = (100, 0, 50, 100, 90, 10)
POISON32 = 0x5a5a5a5a
POISON64 = 0x5a5a5a5a5a5a5a5a


@functools.lru_cache(maxsize=None)
def _picture(kind, w, h, stride):
    img = xp.picture(kind, w, h, stride)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _oracle(kind, w, h, ch, stride, q, ycc):
    """(the oracle's stream, its trace)."""
    packed, tr = ol.oracle_encode(_picture(kind, w, h, stride), q, ycc, channels=ch, stride=stride, trace=True)
    packed.setflags(write=False)
    return packed, tr


def _stream(kind, w, h, ch, stride, q, ycc):
    return _oracle(kind, w, h, ch, stride, q, ycc)[0]


@functools.lru_cache(maxsize=None)
def _decoded(kind, w, h, ch, stride, q, ycc):
    """(the reference's verdict, its pixels or None, the fixed mode's pixels)."""
    packed = _stream(kind, w, h, ch, stride, q, ycc)
    rc, pix = ol.oracle_decode(packed)
    rc_fix, pix_fix = ol.oracle_decode(packed, fix_t2=True)
    assert rc in (0, -7) and rc_fix == 0, (kind, w, h, q, ycc, rc, rc_fix)
    if rc == 0:
        assert np.array_equal(pix, pix_fix)
    return rc, pix, pix_fix


def _engine(opts=None, env=None):
    """A context of its own: options by set_option, knobs the context reads from the environment when it
    is created."""
    env = env or {}
    for k, v in env.items():
        os.environ[k] = v
    try:
        eng = himg_amd.Engine(0)
    finally:
        for k in env:
            del os.environ[k]
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    return eng


@pytest.fixture
def eng(engine):
    """The session's engine; HIMG_OPT_FIX_T2 back to the default behind every test."""
    yield engine
    engine.set_option("fix_t2", 0)


@pytest.fixture(scope="module")
def unfused_engine():
    """Block rows through the generic decode path (symbols via HBM, k_tile_inv)."""
    e = _engine(env={"HIMG_FORCE_UNFUSED": "1"})
    yield e
    e.close()


def _eq(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.size == want.size, "%s: size %d vs %d" % (what, got.size, want.size)
    d = np.flatnonzero(got != want)
    assert d.size == 0, "%s: %d mismatches, first at %d (engine %s, oracle %s)" % (what, d.size, d[0], got[d[0]], want[d[0]])


def _eq_symbols(got, want, tr, ch, what):
    """The FRES plane [rows][C][64][cols]: a mismatch names the channel, the coefficient and the tile."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.size == want.size, "%s: size %d vs %d" % (what, got.size, want.size)
    d = np.flatnonzero(got != want)
    if d.size:
        cols = tr["cols"]
        row, rem = divmod(int(d[0]), ch * 64 * cols)
        c, rem = divmod(rem, 64 * cols)
        k, u = divmod(rem, cols)
        raise AssertionError("%s: %d FRES symbols differ, first in channel %d, coefficient %d of the scan (block "
                             "position %d), tile column %d, block row %d: engine %d, oracle %d"
                             % (what, d.size, c, k, int(sm.SCAN[k]), u, row, int(got[d[0]].view(np.int8)),
                                int(want[d[0]].view(np.int8))))


# ---- encode ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("name,w,h,ch,stride,opts", SHAPES, ids=SHAPE_IDS)
def test_encode_stages_and_stream(name, w, h, ch, stride, opts, ycc):
    """Every intermediate product of the encoder, then the bytes."""
    e = _engine(opts)
    for q in QUALITIES:
        for kind in KINDS:
            what = "%s %s q%d %s" % (name, kind, q, "ycbcr" if ycc else "rgb")
            want, tr = _oracle(kind, w, h, ch, stride, q, ycc)
            got = e.encode(_picture(kind, w, h, stride), q, ycc, channels=ch, pixel_stride=stride)
            n_plane = ch * tr["rows"] * tr["cols"]
            _eq(e.debug_read("avg", 0, n_plane), tr["avg"], what + ": box averages")
            _eq(e.debug_read("lowres", 0, n_plane), tr["lowres"], what + ": low-res plane")
            _eq(e.debug_read("lres_sym", 0, tr["lres_sym"].size), tr["lres_sym"], what + ": LRES symbols")
            _eq_symbols(e.debug_read("fres_sym", 0, tr["fres_sym"].size), tr["fres_sym"], tr, ch, what)
            if opts.get("row_tokens"):
                _eq_symbols(e.debug_read("fres_tok_sym", 0, tr["fres_sym"].size), tr["fres_sym"], tr, ch,
                            what + " (token slots expanded)")
            _eq(e.debug_read("fres_hist", 0, 261 * 4, np.uint32), tr["fres_hist"], what + ": FRES histogram")
            _eq(got, want, what + ": stream")
    e.close()


def _rotations(t):
    return [t[k:] + t[:k] for k in range(len(t))]


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("name,w,h,ch,stride,opts", SHAPES, ids=SHAPE_IDS)
def test_quality_per_frame(name, w, h, ch, stride, opts, ycc):
    """The QI forms: the six kinds as one batch, a quality per frame, every kind at every quality of MIXED
    in turn -- streams (encode_device_q), sizes without a stream (encode_sizes_device) and the distortion
    probe (encode_sse_device: k_sse sends the encoder's +-127 symbols through its own inverse path)."""
    e = _engine(opts)
    B = len(KINDS)
    d_frames = torch.from_numpy(np.stack([_picture(k, w, h, stride) for k in KINDS])).cuda()
    cap = himg_amd.max_packed_size(w, h, ch)
    for quals in _rotations(MIXED):
        what = "%s %s %s" % (name, "ycbcr" if ycc else "rgb", quals)
        wants = [_stream(k, w, h, ch, stride, q, ycc) for k, q in zip(KINDS, quals)]
        d_out = torch.zeros((B * cap + 256,), dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
        d_st = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
        e.encode_device_q(d_frames, B, w, h, stride, ch, quals, ycc, d_out, cap, d_sizes, d_st)
        torch.cuda.synchronize()
        sizes, st, out = d_sizes.cpu().numpy(), d_st.cpu().numpy(), d_out.cpu().numpy()
        assert not st[:B].any() and (st[B:] == POISON32).all() and (sizes[B:] == POISON32).all(), (what, st, sizes)
        for f, want in enumerate(wants):
            assert int(sizes[f]) == want.size, (what, KINDS[f], int(sizes[f]), want.size)
            _eq(out[f * cap: f * cap + want.size], want, "%s: stream of %s" % (what, KINDS[f]))
        assert not out[B * cap:].any(), (what, "bytes behind the last frame's out_stride")

        d_sizes = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
        d_st = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
        e.encode_sizes_device(d_frames, B, w, h, stride, ch, quals, ycc, d_sizes, d_st)
        torch.cuda.synchronize()
        sizes, st = d_sizes.cpu().numpy(), d_st.cpu().numpy()
        assert not st[:B].any() and (st[B:] == POISON32).all() and (sizes[B:] == POISON32).all(), (what, st, sizes)
        assert [int(x) for x in sizes[:B]] == [x.size for x in wants], (what, "sizes")

        # the definition of test_gpu_target.py: the oracle's stream through the oracle's fixed decode
        want_sse = [tgm.sse(_picture(k, w, h, stride)[:, :, :ch], _decoded(k, w, h, ch, stride, q, ycc)[2].reshape(h, w, ch))
                    for k, q in zip(KINDS, quals)]
        d_sse = torch.full((B + 2,), POISON64, dtype=torch.int64, device="cuda")
        d_st = torch.full((B + 2,), POISON32, dtype=torch.int32, device="cuda")
        e.encode_sse_device(d_frames, B, w, h, stride, ch, quals, ycc, d_sse, d_st)
        torch.cuda.synchronize()
        sse, st = d_sse.cpu().numpy(), d_st.cpu().numpy()
        assert not st[:B].any() and (st[B:] == POISON32).all() and (sse[B:] == POISON64).all(), (what, st)
        assert [int(x) for x in sse[:B]] == want_sse, (what, "sse", [int(x) for x in sse[:B]], want_sse)
    e.close()


# ---- full decode ----------------------------------------------------------------------------------

# (width, height, channels, pixel stride of the source): the geometries of SHAPES
DECODE_SHAPES = sorted({(w, h, ch, stride) for _, w, h, ch, stride, _ in SHAPES})


def _check_full_decode(e, packed, rc, pix, what):
    if rc != 0:
        with pytest.raises(himg_amd.HimgError) as ei:
            e.decode(packed)
        assert ei.value.code == himg_amd.HIMG_ERR_FORMAT, (what, ei.value.code)
    else:
        _eq(e.decode(packed), pix, what)


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("w,h,ch,stride", DECODE_SHAPES)
def test_full_decode(eng, unfused_engine, w, h, ch, stride, ycc):
    """The oracle's streams, fused and generic row path: the reference's verdict and pixels; then with
    HIMG_OPT_FIX_T2 the fixed mode's pixels for every stream."""
    cases = [(kind, q) for q in QUALITIES for kind in KINDS]
    rejected = 0
    for fix in (0, 1):
        for e, path in ((eng, "fused"), (unfused_engine, "generic")):
            e.set_option("fix_t2", fix)
            for kind, q in cases:
                what = "%dx%dx%d %s q%d %s %s fix_t2=%d" % (w, h, ch, kind, q, "ycbcr" if ycc else "rgb", path, fix)
                rc, pix, pix_fix = _decoded(kind, w, h, ch, stride, q, ycc)
                rejected += rc != 0
                _check_full_decode(e, _stream(kind, w, h, ch, stride, q, ycc), 0 if fix else rc, pix_fix if fix else pix, what)
            e.set_option("fix_t2", 0)
    assert rejected, "no stream of these pictures is one the reference rejects"


@pytest.mark.parametrize("ycc", MODES)
def test_decode_stages(eng, unfused_engine, ycc):
    """The decoder's intermediate products on one shape (a stream the reference rejects: in the fixed mode)."""
    w, h, ch = 200, 72, 4
    for q in (100, 50, 0):
        for kind in KINDS:
            what = "%s q%d %s" % (kind, q, "ycbcr" if ycc else "rgb")
            packed = _stream(kind, w, h, ch, ch, q, ycc)
            fix = _decoded(kind, w, h, ch, ch, q, ycc)[0] != 0
            ol.oracle().himg_oracle_set_compat_fix(int(fix))
            try:
                rc, dt = ol.oracle_decode_trace(packed)
            finally:
                ol.oracle().himg_oracle_set_compat_fix(0)
            assert rc == 0
            for e in (eng, unfused_engine):
                e.set_option("fix_t2", int(fix))
            _eq(eng.decode(packed), dt["pixels"], what + ": pixels (fused)")
            _eq(eng.debug_read("lres_sym", 0, dt["lres_sym"].size, decoder=True), dt["lres_sym"], what + ": LRES symbols")
            _eq(eng.debug_read("lowres", 0, dt["lowres"].size, decoder=True), dt["lowres"], what + ": low-res plane")
            _eq(unfused_engine.decode(packed), dt["pixels"], what + ": pixels (generic)")
            _eq(unfused_engine.debug_read("fres_sym", 0, dt["fres_sym"].size, decoder=True), dt["fres_sym"], what + ": FRES symbols")
    unfused_engine.set_option("fix_t2", 0)


@pytest.mark.parametrize("persist", ["1", "0", "7"])
def test_row_kernel_forms(persist):
    """The row kernel with persistent workgroups (one per CU; seven) and with one workgroup per row
    (HIMG_PERSIST_ROWS, read when the context is created), on a device batch of every kind at three
    qualities and both colour modes: the reference's verdict per frame, then the fixed mode's pixels."""
    w, h, ch = 200, 72, 4
    e = _engine(env={"HIMG_PERSIST_ROWS": persist})
    keys = [(kind, q, ycc) for ycc in (True, False) for q in (100, 50, 0) for kind in KINDS]
    streams = [_stream(k, w, h, ch, ch, q, y) for k, q, y in keys]
    dec = [_decoded(k, w, h, ch, ch, q, y) for k, q, y in keys]
    assert any(d[0] != 0 for d in dec) and any(d[0] == 0 for d in dec)
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    B = len(streams)
    for fix in (0, 1):
        e.set_option("fix_t2", fix)
        d_pix = torch.full((B, h, w, ch), 0xA5, dtype=torch.uint8, device="cuda")
        d_st = torch.full((B,), -99, dtype=torch.int32, device="cuda")
        e.decode_device(d_in, stride, sizes, B, w, h, ch, d_pix, d_st)
        torch.cuda.synchronize()
        st, pix = d_st.cpu().numpy(), d_pix.cpu().numpy()
        for f, (rc, p, p_fix) in enumerate(dec):
            what = "persist=%s fix_t2=%d %s" % (persist, fix, keys[f])
            if fix or rc == 0:
                assert st[f] == 0, (what, st[f])
                _eq(pix[f], p_fix, what)
            else:
                assert st[f] != 0, (what, "accepted a stream the reference rejects")
    e.close()


# ---- the other decode forms: walsh, step and cube at q100 and q50 -----------------------------------

FORM_KINDS = ("walsh", "step", "cube")
FORM_QUALITIES = (100, 50)


def _form_streams(w, h, ch, ycc):
    """[(what, stream, fix)]: fix -- the reference rejects the stream (trap T2), so both sides decode it
    in the fixed mode (streams the reference accepts decode identically either way)."""
    out = []
    for q in FORM_QUALITIES:
        for kind in FORM_KINDS:
            rc = _decoded(kind, w, h, ch, ch, q, ycc)[0]
            out.append(("%dx%dx%d %s q%d %s" % (w, h, ch, kind, q, "ycbcr" if ycc else "rgb"),
                        _stream(kind, w, h, ch, ch, q, ycc), rc != 0, _decoded(kind, w, h, ch, ch, q, ycc)[2]))
    return out


@pytest.mark.parametrize("ycc", MODES)
def test_preview(eng, ycc):
    for w, h, ch in ((200, 72, 4), (100, 52, 4), (136, 72, 3)):
        for what, packed, fix, _ in _form_streams(w, h, ch, ycc):
            rc, want = preview_expected(packed)
            assert want is not None and (rc != 0) == fix, (what, rc)
            _eq(eng.preview(packed), want, what + ": preview")


def _crop(img, rect):
    x, y, w, h = rect
    return img[y:y + h, x:x + w]


# 4352 pixels of 4 channels are two column strips of the region kernel's LDS layout (520 tiles: the strips
# meet at x = 4160); the windows: inside one strip, across the strips, touching the right and bottom edges
REGION_CASES = [(4352, 24, 4, [(16, 3, 200, 17), (4100, 1, 130, 20), (4352 - 77, 24 - 13, 77, 13)]),
                (100, 52, 4, [(10, 5, 50, 30), (3, 9, 90, 40), (100 - 33, 52 - 21, 33, 21)]),
                (136, 72, 3, [(9, 8, 16, 8), (1, 1, 130, 70), (136 - 9, 72 - 9, 9, 9)])]


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("w,h,ch,rects", REGION_CASES, ids=["two-strips", "ragged", "three-channels"])
def test_region(eng, w, h, ch, rects, ycc):
    items = _form_streams(w, h, ch, ycc)
    for fix in sorted({it[2] for it in items}):
        eng.set_option("fix_t2", int(fix))
        group = [it for it in items if it[2] == fix]
        for rect in rects:
            for what, packed, _, full in group:
                _eq(eng.decode_region(packed, *rect), _crop(full, rect), "%s: region %s" % (what, rect))
            st, out = region_device(eng, [it[1] for it in group], w, h, ch, rect)
            assert (st == 0).all(), (rect, st)
            for i, (what, _, _, full) in enumerate(group):
                _eq(out[i], _crop(full, rect), "%s: region %s (device batch)" % (what, rect))


SCALED_REGION_CASES = [(4352, 24, 4, {1: [(8, 1, 100, 9), (2050, 0, 65, 12), (2176 - 39, 12 - 7, 39, 7)],
                                     2: [(4, 1, 50, 4), (1025, 0, 33, 6), (1088 - 19, 6 - 3, 19, 3)]}),
                       (100, 52, 4, {1: [(5, 2, 25, 15), (1, 3, 45, 20), (50 - 17, 26 - 11, 17, 11)],
                                     2: [(2, 1, 12, 7), (1, 1, 22, 10), (25 - 9, 13 - 5, 9, 5)]})]


@pytest.mark.parametrize("ycc", MODES)
def test_scaled(eng, ycc):
    """1/2 and 1/4 scale against the model of the definition, fed by the oracle's decode trace."""
    for w, h, ch in ((200, 72, 4), (100, 52, 4), (136, 72, 3)):
        for what, packed, fix, _ in _form_streams(w, h, ch, ycc):
            eng.set_option("fix_t2", int(fix))
            for s in (1, 2):
                rc, want = sm.expected(packed, s, fix)
                assert rc == 0
                _eq(eng.decode_scaled(packed, s), want, "%s: scale 1/%d" % (what, 1 << s))


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("w,h,ch,rects", SCALED_REGION_CASES, ids=["two-strips", "ragged"])
def test_scaled_region(eng, w, h, ch, rects, ycc):
    for what, packed, fix, _ in _form_streams(w, h, ch, ycc):
        eng.set_option("fix_t2", int(fix))
        for s in (1, 2):
            rc, want = sm.expected(packed, s, fix)
            assert rc == 0
            for rect in rects[s]:
                _eq(eng.decode_scaled_region(packed, s, *rect), _crop(want, rect), "%s: scale 1/%d window %s" % (what, 1 << s, rect))


@pytest.mark.parametrize("ycc", MODES)
@pytest.mark.parametrize("w,h,ch,origin,ww,wh", [(264, 40, 4, (13, 3), 200, 30), (100, 52, 3, (100 - 41, 52 - 27), 41, 27)],
                         ids=["row-kernel-store", "ragged-three-channels"])
def test_tensor(eng, w, h, ch, origin, ww, wh, ycc):
    """f32 / f16 / bf16 with the ImageNet scale and bias, the full frame and a window, against the
    model's bit patterns of the oracle's decode."""
    items = _form_streams(w, h, ch, ycc)
    fix = any(it[2] for it in items)
    eng.set_option("fix_t2", int(fix))
    streams = [it[1] for it in items]
    pics = [it[3].reshape(h, w, ch) for it in items]
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    n = len(streams)
    x, y = origin
    for dtype in tnm.DTYPES:
        desc = tnm.imagenet(dtype, ch)
        st, got = _tensor(eng, d_in, stride, sizes, w, h, ch, desc)
        assert (st == 0).all(), (dtype, st)
        _same(got, tensor_expected(pics, "imagenet", dtype, ch), "%dx%dx%d dtype %d" % (w, h, ch, dtype))
        st, got = _regions_tensor(eng, d_in, stride, sizes, w, h, ch, [origin] * n, ww, wh, desc)
        assert (st == 0).all(), (dtype, st)
        want = tensor_expected([p[y:y + wh, x:x + ww] for p in pics], "imagenet", dtype, ch)
        _same(got, want, "%dx%dx%d dtype %d window" % (w, h, ch, dtype))


# ---- round trip -----------------------------------------------------------------------------------

@pytest.mark.parametrize("ycc", MODES)
def test_round_trip(eng, ycc):
    """The engine's decode of the engine's own stream is the oracle's decode of it."""
    for w, h, ch in ((200, 72, 4), (100, 52, 4), (136, 72, 3)):
        for q in (100, 50, 0):
            for kind in KINDS:
                what = "%dx%dx%d %s q%d %s" % (w, h, ch, kind, q, "ycbcr" if ycc else "rgb")
                packed = eng.encode(_picture(kind, w, h, ch), q, ycc)
                rc, pix = ol.oracle_decode(packed)
                _check_full_decode(eng, packed, rc, pix, what + ": round trip")
                if rc != 0:
                    rc_fix, pix_fix = ol.oracle_decode(packed, fix_t2=True)
                    assert rc_fix == 0
                    eng.set_option("fix_t2", 1)
                    _eq(eng.decode(packed), pix_fix, what + ": round trip, fix_t2")
                    eng.set_option("fix_t2", 0)
