"""CPU: the C entry points of the per-frame region decode -- himg_hip_decode_regions_device (a
window per frame of a batch in HBM) and himg_hip_decode_regions_batch (host streams, a rectangle
each) are exported and declared, and refuse a NULL context."""
import ctypes as C
import glob
import os
import re

import numpy as np

import himg_amd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "*.himg")))
HEADER = os.path.join(os.path.dirname(HERE), "include", "himg_hip.h")
ENTRIES = ("himg_hip_decode_regions_device", "himg_hip_decode_regions_batch")


def test_entries_exported_and_declared():
    L = himg_amd.lib()
    head = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\(" % name, head), name
    assert "const int32_t *h_origins" in head and "const int32_t *rects" in head


def test_null_context_is_arg_error():
    L = himg_amd.lib()
    b = np.frombuffer(open(GOLDEN[0], "rb").read(), np.uint8)
    sizes = np.array([b.nbytes], np.uint32)
    org = np.zeros(2, np.int32)
    dst = np.zeros(64, np.uint8)
    assert L.himg_hip_decode_regions_device(None, b.ctypes.data, 256, sizes.ctypes.data, 1, 64, 64, 4, org.ctypes.data,
                                            1, 1, dst.ctypes.data, dst.ctypes.data, None) == himg_amd.HIMG_ERR_ARG
    src = (C.c_void_p * 1)(b.ctypes.data)
    szs = (C.c_size_t * 1)(b.nbytes)
    rects = np.array([0, 0, 1, 1], np.int32)
    dsts = (C.c_void_p * 1)(dst.ctypes.data)
    caps = (C.c_size_t * 1)(dst.nbytes)
    ws, hs, cs = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    assert L.himg_hip_decode_regions_batch(None, src, szs, 1, rects.ctypes.data, dsts, caps, ws, hs,
                                           cs) == himg_amd.HIMG_ERR_ARG


def test_python_bindings_are_declared():
    for name in ("decode_regions", "decode_regions_device"):
        assert callable(getattr(himg_amd.Engine, name, None)), name
