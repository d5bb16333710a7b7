"""Host (no GPU): the tensor decode's descriptor rules through himg_hip_tensor_bytes, tensor_desc's
mean / std arithmetic, the exported symbols, and the properties of the numpy model
(tests/tensor_model.py) the GPU tests compare against."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import himg_amd
import tensor_model as tm


def _bytes_rc(desc, channels, w, h):
    n = C.c_size_t(12345)
    rc = himg_amd.lib().himg_hip_tensor_bytes(C.byref(desc), channels, w, h, C.byref(n))
    return rc, n.value


def test_symbols_exported():
    L = himg_amd.lib()
    for name in ("himg_hip_tensor_bytes", "himg_hip_decode_tensor_device", "himg_hip_decode_regions_tensor_device"):
        assert hasattr(L, name), name
    assert (himg_amd.HIMG_DT_F32, himg_amd.HIMG_DT_F16, himg_amd.HIMG_DT_BF16) == (0, 1, 2)
    assert C.sizeof(himg_amd.TensorDesc) == 40


@pytest.mark.parametrize("dtype,elem", [(tm.F32, 4), (tm.F16, 2), (tm.BF16, 2)])
def test_tensor_bytes_sizes(dtype, elem):
    for channels, co, w, h in [(4, 3, 4096, 4096), (4, 4, 203, 21), (3, 1, 100, 37), (1, 1, 67, 19), (2, 2, 1000, 16)]:
        assert himg_amd.tensor_bytes(tm.imagenet(dtype, co), channels, w, h) == co * w * h * elem
    for tdt in (torch.float32, torch.float16, torch.bfloat16):
        d = himg_amd.tensor_desc(tdt, 3)
        assert himg_amd.tensor_bytes(d, 4, 8, 8) == 3 * 64 * torch.empty(0, dtype=tdt).element_size()


def test_tensor_bytes_rejects():
    ok = tm.imagenet(tm.F16, 3)
    assert _bytes_rc(ok, 4, 64, 32) == (0, 3 * 64 * 32 * 2)
    for dtype in (-1, 3):
        d = tm.imagenet(tm.F16, 3)
        d.dtype = dtype
        assert _bytes_rc(d, 4, 64, 32) == (himg_amd.HIMG_ERR_ARG, 12345), dtype
    for channels, co in [(4, 0), (4, 5), (3, 4), (1, 2), (4, -1)]:
        d = tm.identity(tm.F32, 1)
        d.out_channels = co
        assert _bytes_rc(d, channels, 64, 32)[0] == himg_amd.HIMG_ERR_ARG, (channels, co)
    for field in ("scale", "bias"):
        for bad in (math.nan, math.inf, -math.inf):
            for slot in range(3):
                d = tm.imagenet(tm.BF16, 3)
                getattr(d, field)[slot] = bad
                assert _bytes_rc(d, 4, 64, 32)[0] == himg_amd.HIMG_ERR_ARG, (field, bad, slot)
            # an ignored slot may hold anything
            d = tm.imagenet(tm.BF16, 3)
            getattr(d, field)[3] = bad
            assert _bytes_rc(d, 4, 64, 32) == (0, 3 * 64 * 32 * 2), (field, bad)
    with pytest.raises(himg_amd.HimgError) as e:
        himg_amd.tensor_bytes(tm.identity(tm.F32, 4), 3, 8, 8)
    assert e.value.code == himg_amd.HIMG_ERR_ARG
    assert _bytes_rc(ok, 4, 0, 32)[0] == himg_amd.HIMG_ERR_ARG


def test_tensor_desc_mean_std():
    d = himg_amd.tensor_desc(torch.float16, 3, mean=tm.IMAGENET_MEAN, std=tm.IMAGENET_STD)
    assert (d.dtype, d.out_channels) == (himg_amd.HIMG_DT_F16, 3)
    for c in range(3):
        m, s = float(tm.IMAGENET_MEAN[c]), float(tm.IMAGENET_STD[c])
        assert d.scale[c] == float(np.float32(1.0 / (255.0 * s))), c
        assert d.bias[c] == float(np.float32(-m / s)), c
    assert d.scale[3] == 0.0 and d.bias[3] == 0.0
    e = himg_amd.tensor_desc(himg_amd.HIMG_DT_BF16, 2, scale=(2.0, -0.5), bias=(1.0, 3.0))
    assert (e.dtype, list(e.scale)[:2], list(e.bias)[:2]) == (2, [2.0, -0.5], [1.0, 3.0])
    i = himg_amd.tensor_desc(torch.float32, 4)
    assert list(i.scale) == [1.0] * 4 and list(i.bias) == [0.0] * 4
    with pytest.raises(ValueError):
        himg_amd.tensor_desc(torch.float64, 3)
    with pytest.raises(ValueError):
        himg_amd.tensor_desc(torch.float32, 3, mean=tm.IMAGENET_MEAN, scale=(1, 1, 1))


@pytest.mark.parametrize("name", sorted(tm.DESCS))
def test_model_tables(name):
    tdt = {tm.F32: torch.float32, tm.F16: torch.float16, tm.BF16: torch.bfloat16}
    f16_min_normal, bf16_min_normal = 2.0 ** -14, 2.0 ** -126
    for dtype in tm.DTYPES:
        desc = tm.DESCS[name](dtype, 4)
        assert himg_amd.tensor_bytes(desc, 4, 8, 8) == 4 * 64 * tm.ELEM[dtype]
        t = tm.tables(desc)   # (asserts that every entry's double is the exact real value)
        assert t.shape == (4, 256) and t.dtype == tm.BITS[dtype]
        for c in range(4):
            x32 = tm.f32_table(desc.scale[c], desc.bias[c])
            # the conversion against torch's on the CPU, bit for bit
            want = torch.from_numpy(x32).to(tdt[dtype])
            want = want.view(torch.int32 if dtype == tm.F32 else torch.int16).numpy().view(tm.BITS[dtype])
            assert np.array_equal(t[c], want), (name, dtype, c)
            # zero or normal in every type: no result depends on how denormals are treated
            a = np.abs(x32.astype(np.float64))
            lim = {tm.F32: 2.0 ** -126, tm.F16: f16_min_normal, tm.BF16: bf16_min_normal}[dtype]
            assert ((a == 0) | (a >= lim)).all() and np.isfinite(x32).all(), (name, dtype, c)
            if dtype == tm.F16:   # ... and so is the converted value
                v = t[c].view(np.float16).astype(np.float64)
                assert ((v == 0) | (np.abs(v) >= f16_min_normal)).all() and np.isfinite(v).all(), (name, c)
    # the identity table is the byte value itself
    assert np.array_equal(tm.f32_table(1.0, 0.0), np.arange(256, dtype=np.float32))
    # bfloat16 rounds to nearest even: 2 v - 1 at v = 255 is 509 -> 508 (tie to even), never truncation alone
    assert tm.bf16_bits(np.array([509.0, 511.0, 1.0], np.float32)).tolist() == [0x43FE, 0x4400, 0x3F80]


def test_model_expected_layout():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    d = tm.mix(tm.F32, 3)
    e = tm.expected(img, d)
    assert e.shape == (3, 5, 7) and e.dtype == np.uint32
    for c in range(3):
        want = np.float32(np.float64(img[:, :, c]) * float(d.scale[c]) + float(d.bias[c]))
        assert np.array_equal(e[c].view(np.float32), want), c
