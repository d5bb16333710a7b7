"""GPU (-m gpu): the assembled streams of tests/assembled_cases.py -- valid streams that no encoder writes
(what each reaches is proved on the CPU by tests/test_assembler_host.py, where the oracle is pinned to
the real reference on every one of them) -- through the decoder's forms, bit-exact against the CPU oracle
and against scaled_model / tensor_model fed by the oracle's trace.  Streams the reference rejects (trap
T2, the one-leaf tree) are tested for the rejection by default and for the oracle's fixed-mode pixels with
HIMG_OPT_FIX_T2; a tree 33 deep is answered with HIMG_ERR_UNSUPPORTED by every entry point.

Which family runs where:
  A trees, B tokens   full decode at every shape of assembled_cases.SHAPES (row kernel <512>, <256>, <240>,
                      <-1>, <0> with three channels and ragged, rows wider than the LDS), each through the
                      fused and the unfused engine, count_wave 0 and 1, HIMG_PERSIST_ROWS 0 and 1; the
                      8192-row device batch (k_row_count_w); decoder stages; a mixed device batch
  C tables            the same full decodes (row kernels, k_tile_inv), region, scaled, scaled region, tensor
  D LRES, E fixed     decoder stages (lres_sym, lowres, fres_sym), preview, full decode; E also the full
                      decodes of A/B (row count kernels) and the region decode
  F container         at 64x24x4: every device form and the host forms (decode, preview_to by preview,
                      decode_batch); the host peeks are tested without a GPU in test_assembler_host.py"""
import functools
import os

import numpy as np
import pytest
import torch

import assembled_cases as ac
import himg_amd
import oracle_lib as ol
import scaled_model as sm
import tensor_model as tnm
from test_gpu_preview import expected as preview_expected
from test_gpu_region import _device as region_device
from test_gpu_regions import _upload
from test_gpu_tensor import _expected as tensor_expected, _regions_tensor, _same, _tensor

pytestmark = pytest.mark.gpu

# A frame's word in a device batch's status array for a tree more than 32 deep (kStUnsupported in
# himg_amd/csrc/kernels_dec.hip): what the host forms turn into HIMG_ERR_UNSUPPORTED.
ST_UNSUPPORTED = 3


@functools.lru_cache(maxsize=None)
def _judged(key):
    """(case, the reference's verdict, its pixels, the fixed mode's verdict, its pixels), by the oracle."""
    c = ac.case(*key)
    rc, pix = ol.oracle_decode(c.stream)
    rc_fix, pix_fix = ol.oracle_decode(c.stream, fix_t2=True)
    return c, rc, pix, rc_fix, pix_fix


def _trace(c, fix):
    ol.oracle().himg_oracle_set_compat_fix(int(fix))
    try:
        rc, dt = ol.oracle_decode_trace(c.stream)
    finally:
        ol.oracle().himg_oracle_set_compat_fix(0)
    assert rc == 0, (c.id, rc)
    return dt


def _engine(env):
    """A context of its own with knobs that it reads from the environment when it is created."""
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return himg_amd.Engine(0)
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture
def eng(engine):
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)
    yield engine
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)


@pytest.fixture(scope="module")
def forms(engine):
    """[(name, engine, count_wave)]: the fused row decode, the unfused one, persistent workgroups off and on."""
    made = [_engine({"HIMG_FORCE_UNFUSED": "1"}), _engine({"HIMG_PERSIST_ROWS": "0"}), _engine({"HIMG_PERSIST_ROWS": "1"})]
    yield [("fused count_wave=0", engine, 0), ("fused count_wave=1", engine, 1), ("unfused", made[0], -1),
           ("persist=0", made[1], -1), ("persist=1", made[2], -1)]
    engine.set_option("count_wave", -1)
    engine.set_option("fix_t2", 0)
    for e in made:
        e.close()


def _eq(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.size == want.size, "%s: size %d vs %d" % (what, got.size, want.size)
    d = np.flatnonzero(got != want)
    assert d.size == 0, "%s: %d mismatches, first at %d (engine %s, oracle %s)" % (what, d.size, d[0], got[d[0]], want[d[0]])


def _expect_error(fn, code, what):
    with pytest.raises(himg_amd.HimgError) as ei:
        fn()
    assert ei.value.code == code, (what, ei.value.code, code)


def _check_decode(e, key, fix, what):
    c, rc, pix, rc_fix, pix_fix = _judged(key)
    e.set_option("fix_t2", int(fix))
    want_rc, want = (rc_fix, pix_fix) if fix else (rc, pix)
    if c.expect == "unsupported":
        _expect_error(lambda: e.decode(c.stream), himg_amd.HIMG_ERR_UNSUPPORTED, what)
    elif want_rc != 0:
        _expect_error(lambda: e.decode(c.stream), himg_amd.HIMG_ERR_FORMAT, what)
    else:
        _eq(e.decode(c.stream), want, what)


# ---- full decode: every family with FRES content of its own, every row kernel form ------------------

FULL = {"A": ac.KINDS_A, "B": ac.KINDS_B, "C": ["C-" + k for k in ac.KINDS_C], "E": ac.KINDS_E}
SHAPE_IDS = ["%dx%dx%d" % s for s in ac.SHAPES]


@pytest.mark.parametrize("family", sorted(FULL))
@pytest.mark.parametrize("shape", ac.SHAPES, ids=SHAPE_IDS)
def test_full_decode(forms, shape, family):
    keys = [(k,) + shape for k in FULL[family] if (k,) + shape in ac.CASES]
    assert keys
    verdicts = set()
    for name, e, cw in forms:
        e.set_option("count_wave", cw)
        for key in keys:
            for fix in (0, 1):
                _check_decode(e, key, fix, "%s %s fix_t2=%d" % (ac.case_id(key), name, fix))
            verdicts.add(_judged(key)[1] == 0)
        e.set_option("fix_t2", 0)
    if family in ("A", "B"):
        assert verdicts == {True, False}, "both accepted and rejected streams"
    _judged.cache_clear()
    ac.case.cache_clear()


@pytest.mark.parametrize("key", [k for k in ac.CASES if k[0] in ac.KINDS_A_REJECTED], ids=ac.case_id)
def test_rejected_trees(forms, key):
    """Depth 33 (HIMG_ERR_UNSUPPORTED, the LRES tree and the FRES tree alike), a used leaf 300 and 262 leaves
    (HIMG_ERR_FORMAT) in every entry point, both modes."""
    c, rc, _, rc_fix, _ = _judged(key)
    code = himg_amd.HIMG_ERR_UNSUPPORTED if c.expect == "unsupported" else himg_amd.HIMG_ERR_FORMAT
    assert c.expect == "unsupported" or (rc != 0 and rc_fix != 0)
    W, H, C = key[1:]
    for name, e, cw in forms:
        e.set_option("count_wave", cw)
        for fix in (0, 1):
            e.set_option("fix_t2", fix)
            what = "%s %s fix_t2=%d" % (c.id, name, fix)
            _expect_error(lambda: e.decode(c.stream), code, what)
            _expect_error(lambda: e.decode_region(c.stream, 8, 3, 24, 9), code, what + " region")
            _expect_error(lambda: e.decode_scaled(c.stream, 1), code, what + " scaled")
            _expect_error(lambda: e.decode_scaled_region(c.stream, 1, 2, 1, 9, 5), code, what + " scaled region")
            if "lres" in c.name:
                _expect_error(lambda: e.preview(c.stream), code, what + " preview")
            d_in, stride = _upload([c.stream])
            for desc in (None, tnm.imagenet(tnm.DTYPES[0], C)):
                d_st = torch.full((1,), -99, dtype=torch.int32, device="cuda")
                if desc is None:
                    e.decode_device(d_in, stride, [c.stream.size], 1, W, H, C, torch.zeros((1, H, W, C), dtype=torch.uint8, device="cuda"), d_st)
                    torch.cuda.synchronize()
                    st = d_st.cpu().numpy()
                else:
                    st, _ = _tensor(e, d_in, stride, [c.stream.size], W, H, C, desc)
                if c.expect == "unsupported":
                    assert st[0] == ST_UNSUPPORTED, (what, st[0])
                else:
                    assert st[0] not in (0, ST_UNSUPPORTED), (what, st[0])
        e.set_option("fix_t2", 0)


# ---- device batches -----------------------------------------------------------------------------------

def _batch(e, keys, fix):
    """decode_device over the cases (one geometry), poisoned output: (status, pixels)."""
    W, H, C = keys[0][1:]
    streams = [_judged(k)[0].stream for k in keys]
    d_in, stride = _upload(streams)
    B = len(keys)
    e.set_option("fix_t2", int(fix))
    d_pix = torch.full((B, H, W, C), 0xA5, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    e.decode_device(d_in, stride, [len(s) for s in streams], B, W, H, C, d_pix, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_pix.cpu().numpy()


@pytest.mark.parametrize("shape", [(64, 24, 4), (2048, 16, 4)], ids=["64x24x4", "2048x16x4"])
def test_mixed_device_batch(forms, shape):
    """Accepted and rejected streams side by side: every frame's status and pixels are its own."""
    keys = [(k,) + shape for k in ac.KINDS_A + ac.KINDS_A_REJECTED + ac.KINDS_B + ac.KINDS_E + ["C-fmap-random", "C-nibbles-0"]]
    if shape == (64, 24, 4):
        keys += [("F-" + k,) + shape for k in ac.KINDS_F]
    dec = [_judged(k) for k in keys]
    assert any(d[1] != 0 for d in dec) and any(d[1] == 0 for d in dec)
    for name, e, cw in forms:
        e.set_option("count_wave", cw)
        for fix in (0, 1):
            st, pix = _batch(e, keys, fix)
            for f, (c, rc, p, rc_fix, p_fix) in enumerate(dec):
                what = "%s %s fix_t2=%d frame %d" % (c.id, name, fix, f)
                want_rc, want = (rc_fix, p_fix) if fix else (rc, p)
                if c.expect == "unsupported":
                    assert st[f] == ST_UNSUPPORTED, (what, st[f])
                elif want_rc != 0:
                    assert st[f] not in (0, ST_UNSUPPORTED), (what, st[f])
                else:
                    assert st[f] == 0, (what, st[f])
                    _eq(pix[f], want, what)
        e.set_option("fix_t2", 0)
    _judged.cache_clear()
    ac.case.cache_clear()


@pytest.mark.parametrize("kind", ac.BATCH_KINDS)
def test_batch_of_8192_rows(eng, kind):
    """One 64x512x4 stream 128 times: 8192 block rows in one launch (k_row_count_w)."""
    key = (kind,) + ac.BATCH_SHAPE
    c, rc, pix, _, _ = _judged(key)
    assert rc == 0
    st, got = _batch(eng, [key] * 128, 0)
    assert (st == 0).all(), st
    assert (got == pix[None]).all(), "%s: %d of 128 frames differ" % (c.id, int((got != pix[None]).any(axis=(1, 2, 3)).sum()))


# ---- the decoder's stages, the preview ----------------------------------------------------------------

STAGE_KEYS = [k for k in ac.CASES if k[0] not in ac.KINDS_A_REJECTED and
              (k[0][0] == "D" or "lres" in k[0] or (k[0] in ("A-comb32", "A-deeper-17", "E-5", "E-7")
                                                   and k[1:] in ((64, 24, 4), (100, 52, 4), (4096, 16, 4))))]


@pytest.mark.parametrize("key", STAGE_KEYS, ids=ac.case_id)
def test_decoder_stages_and_preview(eng, forms, key):
    c, rc, pix, rc_fix, pix_fix = _judged(key)
    fix = rc != 0
    dt = _trace(c, fix)
    unfused = forms[2][1]
    for e in (eng, unfused):
        e.set_option("fix_t2", int(fix))
    _eq(eng.decode(c.stream), dt["pixels"], c.id + ": pixels")
    _eq(eng.debug_read("lres_sym", 0, dt["lres_sym"].size, decoder=True), dt["lres_sym"], c.id + ": LRES symbols")
    _eq(eng.debug_read("lowres", 0, dt["lowres"].size, decoder=True), dt["lowres"], c.id + ": low-res plane")
    _eq(unfused.decode(c.stream), dt["pixels"], c.id + ": pixels (unfused)")
    _eq(unfused.debug_read("fres_sym", 0, dt["fres_sym"].size, decoder=True), dt["fres_sym"], c.id + ": FRES symbols")
    unfused.set_option("fix_t2", 0)
    prc, want = preview_expected(c.stream, fix)
    assert want is not None
    _eq(eng.preview(c.stream), want, c.id + ": preview")
    _judged.cache_clear()
    ac.case.cache_clear()


# ---- region, scaled, scaled region, tensor: the tables (C), the fixed-length codes (E) ---------------

def _crop(img, rect):
    x, y, w, h = rect
    return img[y:y + h, x:x + w]


def _form_cases(shape, kinds):
    """[(case, fix, the pixels)]: fix -- the reference rejects the stream, so both sides decode it fixed."""
    out = []
    for k in kinds:
        c, rc, pix, _, pix_fix = _judged((k,) + shape)
        out.append((c, rc != 0, pix_fix))
    return out


C_KINDS = ["C-" + k for k in ac.KINDS_C]
# 4352 pixels of 4 channels are two column strips of the region kernel's LDS layout (they meet at x = 4160)
REGION_CASES = [((4352, 16, 4), [(16, 3, 200, 11), (4100, 1, 130, 14), (4352 - 77, 16 - 13, 77, 13)]),
                ((100, 52, 4), [(10, 5, 50, 30), (3, 9, 90, 40), (100 - 33, 52 - 21, 33, 21)]),
                ((72, 16, 3), [(9, 8, 16, 8), (1, 1, 70, 14), (72 - 9, 16 - 9, 9, 9)])]


@pytest.mark.parametrize("shape,rects", REGION_CASES, ids=["two-strips", "ragged", "three-channels"])
def test_region(eng, shape, rects):
    W, H, C = shape
    items = _form_cases(shape, C_KINDS + ([k for k in ac.KINDS_E if (k,) + shape in ac.CASES]))
    for fix in sorted({it[1] for it in items}):
        eng.set_option("fix_t2", int(fix))
        group = [it for it in items if it[1] == fix]
        for rect in rects:
            for c, _, full in group:
                _eq(eng.decode_region(c.stream, *rect), _crop(full, rect), "%s: region %s" % (c.id, rect))
            st, out = region_device(eng, [it[0].stream for it in group], W, H, C, rect)
            assert (st == 0).all(), (rect, st)
            for i, (c, _, full) in enumerate(group):
                _eq(out[i], _crop(full, rect), "%s: region %s (device batch)" % (c.id, rect))
    _judged.cache_clear()
    ac.case.cache_clear()


SCALED_REGION_CASES = [((4352, 16, 4), {1: [(8, 1, 100, 6), (2050, 0, 65, 8), (2176 - 39, 8 - 7, 39, 7)],
                                        2: [(4, 1, 50, 3), (1025, 0, 33, 4), (1088 - 19, 4 - 3, 19, 3)]}),
                       ((100, 52, 4), {1: [(5, 2, 25, 15), (1, 3, 45, 20), (50 - 17, 26 - 11, 17, 11)],
                                       2: [(2, 1, 12, 7), (1, 1, 22, 10), (25 - 9, 13 - 5, 9, 5)]})]


@pytest.mark.parametrize("shape", [(64, 24, 4), (100, 52, 4), (72, 16, 3), (2048, 16, 4)], ids=["64x24x4", "100x52x4", "72x16x3", "2048x16x4"])
def test_scaled(eng, shape):
    """1/2 and 1/4 scale against the model of the definition, fed by the oracle's decode trace."""
    for c, fix, _ in _form_cases(shape, C_KINDS):
        eng.set_option("fix_t2", int(fix))
        for s in (1, 2):
            rc, want = sm.expected(c.stream, s, fix)
            assert rc == 0
            _eq(eng.decode_scaled(c.stream, s), want, "%s: scale 1/%d" % (c.id, 1 << s))
    _judged.cache_clear()
    ac.case.cache_clear()


@pytest.mark.parametrize("shape,rects", SCALED_REGION_CASES, ids=["two-strips", "ragged"])
def test_scaled_region(eng, shape, rects):
    for c, fix, _ in _form_cases(shape, C_KINDS):
        eng.set_option("fix_t2", int(fix))
        for s in (1, 2):
            rc, want = sm.expected(c.stream, s, fix)
            assert rc == 0
            for rect in rects[s]:
                _eq(eng.decode_scaled_region(c.stream, s, *rect), _crop(want, rect), "%s: scale 1/%d window %s" % (c.id, 1 << s, rect))
    _judged.cache_clear()
    ac.case.cache_clear()


@pytest.mark.parametrize("shape,stage,origin,ww,wh", [((4096, 16, 4), "k_dec_row_fused_t<512>", (13, 3), 200, 11),
                                                     ((100, 52, 4), "k_dec_row_fused_t<0>", (100 - 41, 52 - 27), 41, 27)],
                         ids=["row-kernel-store", "ragged"])
def test_tensor(eng, shape, stage, origin, ww, wh):
    """f32 / f16 / bf16 with the ImageNet scale and bias, the full frame and a window, against the model's
    bit patterns of the oracle's decode; the profiler's stage name says that the tensor kernel ran."""
    W, H, C = shape
    items = _form_cases(shape, C_KINDS)
    assert not any(it[1] for it in items)
    streams = [it[0].stream for it in items]
    pics = [it[2].reshape(H, W, C) for it in items]
    d_in, stride = _upload(streams)
    sizes = [len(s) for s in streams]
    n = len(streams)
    x, y = origin
    for dtype in tnm.DTYPES:
        desc = tnm.imagenet(dtype, C)
        eng.profile(True)
        eng.profile_reset()
        st, got = _tensor(eng, d_in, stride, sizes, W, H, C, desc)
        stages = eng.profile_read()
        eng.profile(False)
        assert (st == 0).all(), (dtype, st)
        assert stage in stages, (stage, sorted(stages))
        _same(got, tensor_expected(pics, "imagenet", dtype, C), "%dx%dx%d dtype %d" % (W, H, C, dtype))
        st, got = _regions_tensor(eng, d_in, stride, sizes, W, H, C, [origin] * n, ww, wh, desc)
        assert (st == 0).all(), (dtype, st)
        want = tensor_expected([p[y:y + wh, x:x + ww] for p in pics], "imagenet", dtype, C)
        _same(got, want, "%dx%dx%d dtype %d window" % (W, H, C, dtype))
    _judged.cache_clear()
    ac.case.cache_clear()


# ---- the container (F): every form at 64x24x4, host forms against device forms ------------------------

@pytest.mark.parametrize("kind", ac.KINDS_F)
def test_container(eng, forms, kind):
    key = ("F-" + kind, 64, 24, 4)
    c, rc, pix, _, _ = _judged(key)
    assert rc == 0
    W, H, C = key[1:]
    dt = _trace(c, False)
    for name, e, cw in forms:
        e.set_option("count_wave", cw)
        _eq(e.decode(c.stream), pix, "%s %s" % (c.id, name))
    _eq(eng.debug_read("lres_sym", 0, dt["lres_sym"].size, decoder=True), dt["lres_sym"], c.id + ": LRES symbols")
    _eq(eng.debug_read("lowres", 0, dt["lowres"].size, decoder=True), dt["lowres"], c.id + ": low-res plane")
    _eq(eng.decode_batch([c.stream, c.stream])[1], pix, c.id + ": decode_batch")
    st, got = _batch(eng, [key, key], 0)
    assert (st == 0).all() and (got == pix[None]).all(), c.id + ": decode_device"
    _, want = preview_expected(c.stream)
    _eq(eng.preview(c.stream), want, c.id + ": preview")
    _eq(eng.preview_batch([c.stream])[0], want, c.id + ": preview_batch")
    for rect in ((10, 5, 40, 13), (0, 0, 64, 24), (64 - 9, 24 - 9, 9, 9)):
        _eq(eng.decode_region(c.stream, *rect), _crop(pix, rect), "%s: region %s" % (c.id, rect))
        st, out = region_device(eng, [c.stream], W, H, C, rect)
        assert (st == 0).all()
        _eq(out[0], _crop(pix, rect), "%s: region %s (device)" % (c.id, rect))
    for s in (1, 2):
        _, want = sm.expected(c.stream, s, False)
        _eq(eng.decode_scaled(c.stream, s), want, "%s: scale 1/%d" % (c.id, 1 << s))
        rect = (1, 1, 9, 4) if s == 1 else (1, 1, 5, 3)
        _eq(eng.decode_scaled_region(c.stream, s, *rect), _crop(want, rect), "%s: scale 1/%d window" % (c.id, 1 << s))
    d_in, stride = _upload([c.stream])
    for dtype in tnm.DTYPES:
        desc = tnm.imagenet(dtype, C)
        st, got = _tensor(eng, d_in, stride, [c.stream.size], W, H, C, desc)
        assert (st == 0).all()
        _same(got, tensor_expected([pix.reshape(H, W, C)], "imagenet", dtype, C), "%s dtype %d" % (c.id, dtype))
        st, got = _regions_tensor(eng, d_in, stride, [c.stream.size], W, H, C, [(7, 3)], 30, 11, desc)
        assert (st == 0).all()
        _same(got, tensor_expected([pix.reshape(H, W, C)[3:14, 7:37]], "imagenet", dtype, C), "%s dtype %d window" % (c.id, dtype))
