"""CPU: the opened-streams handle's host-only parts -- himg_hip_opened_bytes against the formula of
include/himg_hip.h, its argument errors, the new symbols in the ABI -- and a model check, with the oracle alone,
that the independence cases test_gpu_opened_streams.py splits into two calls are not vacuous."""
import ctypes as C

import pytest

import himg_amd
import damage_model as dm
import stream_region_cases as sc


def _r256(x):
    return (x + 255) // 256 * 256


def formula(W, H, Cn, n):
    rows, cols = (H + 7) // 8, (W + 7) // 8
    terms = [n * 1616, n * 4176, n * 32768, n * 16384, n * 16384, n * rows * 8, n * _r256(Cn * rows * cols),
             n * rows * (2 * 1024 + 72) * 4, (n * (rows + 1) * 8 + n * 4 + n * rows * 8) * 4, n * 12]
    return sum(_r256(t) for t in terms)


@pytest.mark.parametrize("W,H,Cn,n", [(96, 72, 4, 2), (50, 41, 3, 1), (33, 9, 1, 5), (16384, 16384, 4, 1), (4096, 4096, 4, 128),
                                      (8192, 64, 4, 65535)])
def test_opened_bytes_is_the_formula(W, H, Cn, n):
    got = himg_amd.opened_bytes(W, H, Cn, n)
    assert got == formula(W, H, Cn, n)
    rows = (H + 7) // 8
    assert got > n * rows * 8480 and got % 256 == 0   # the records: [rows][2 * 1024 + 72] words per stream


def test_opened_bytes_argument_errors():
    L = himg_amd.lib()
    b = C.c_size_t(7)
    for args in [(0, 72, 4, 1), (96, 0, 4, 1), (96, 72, 0, 1), (96, 72, 5, 1), (96, 72, 4, 0), (96, 72, 4, 65536), (96, 72, 4, -1)]:
        assert L.himg_hip_opened_bytes(*args, C.byref(b)) == himg_amd.HIMG_ERR_ARG, args
        assert b.value == 7
        with pytest.raises(himg_amd.HimgError) as e:
            himg_amd.opened_bytes(*args)
        assert e.value.code == himg_amd.HIMG_ERR_ARG
    assert L.himg_hip_opened_bytes(96, 72, 4, 1, None) == himg_amd.HIMG_ERR_ARG


def test_abi_has_the_opened_entries():
    L = himg_amd.lib()
    for name in ["himg_hip_opened_bytes", "himg_hip_open_streams_device", "himg_hip_open_stream_host",
                 "himg_hip_opened_regions_device", "himg_hip_opened_regions_to", "himg_hip_opened_info",
                 "himg_hip_close_streams"]:
        assert hasattr(L, name), name
    for name in ["open_streams_device", "open_stream"]:
        assert callable(getattr(himg_amd.Engine, name))
    for name in ["regions_device", "regions", "info", "close", "__enter__", "__exit__"]:
        assert callable(getattr(himg_amd.OpenedStreams, name))
    # host-only refusals need no context
    assert L.himg_hip_opened_info(None, None, None, None, None, None, None) == himg_amd.HIMG_ERR_ARG
    o = C.c_void_p(1)
    assert L.himg_hip_open_stream_host(None, None, 0, C.byref(o)) == himg_amd.HIMG_ERR_ARG and not o.value
    assert L.himg_hip_opened_regions_device(None, None, None, None, 1, 1, 1, None, None, None) == himg_amd.HIMG_ERR_ARG
    L.himg_hip_close_streams(None, None)


@pytest.mark.parametrize("name", ["payload", "header", "cut", "surplus", "head"])
def test_split_calls_are_not_vacuous(name):
    """Each case has at least one window that fails and one that passes: both of the two calls it is split into
    hold windows, and the damaged stream's windows are in both unless its head fails all of them."""
    so, _ = sc.windows()
    codes = [c for c, _ in sc.expected(name)]
    assert dm.FORMAT in codes and dm.OK in codes, codes
    assert all(c == dm.OK for c, s in zip(codes, so) if s == 1)
    if name != "head":
        codes0 = [c for c, s in zip(codes, so) if s == 0]
        assert dm.FORMAT in codes0 and dm.OK in codes0
