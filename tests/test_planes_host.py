"""CPU (-m "not gpu"): the host side of the planes decode -- the model (tests/planes_model.py) checked
against the oracle's own full decode, the argument rules of himg_hip_planes_bytes, himg_hip_peek_format
on the golden streams and on a rewritten one, the exported symbols and their declarations, and
dhimg -g's argument clashes, which are refused before the file is read or a device is opened."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_util as gu
import himg_amd
import oracle_lib as ol
import planes_model as pm
from test_cli import _run, tools  # noqa: F401  (tools: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("himg_hip_planes_bytes", "himg_hip_peek_format", "himg_hip_decode_planes_device",
           "himg_hip_decode_planes_to")


def _picture(kind, w, h, c, seed=0):
    if kind == "binary":   # 0 / 255 noise: every clamp of the colour inverse is met
        return np.random.default_rng(seed).choice(np.array([0, 255], np.uint8), size=(h, w, c))
    return np.ascontiguousarray(himg_amd.synth(kind, seed, w, h)[:, :, :c])


MODEL_SHAPES = [(8, 8, 3), (9, 8, 4), (13, 21, 4), (100, 37, 3), (203, 21, 4), (264, 40, 4)]


@pytest.mark.parametrize("w,h,c", MODEL_SHAPES)
def test_model_recombines_to_the_oracles_decode(w, h, c):
    """This checks the model, not the feature: the planes taken from the rewritten streams, sent through
    ycbcr.cpp:54-82 in numpy, are the oracle's full decode byte for byte, and the alpha plane is the
    full decode's alpha -- in the reference's mode wherever the T2 rule lets the stream through, and in
    the fixed mode always."""
    passed = 0
    for q in (50, 90):
        for kind in ("randtile", "binary"):
            s = ol.oracle_encode(_picture(kind, w, h, c, seed=q), q, True)
            assert pm.header(s) == (w, h, c, 1)
            for fix in (False, True):
                rc, full = ol.oracle_decode(s, fix_t2=fix)
                rc_p, pl = pm.planes(s, fix_t2=fix)
                assert rc_p == rc, (q, kind, fix, rc, rc_p)   # the FRES chunk keeps its size: the same T2 verdict
                if rc:
                    assert not fix, "the fixed mode accepts every stream of the oracle's encoder"
                    continue
                assert pl.shape == (c, h, w)
                assert np.array_equal(pm.to_picture(pl, 1), full.reshape(h, w, c)), (q, kind, fix)
                if c == 4:
                    assert np.array_equal(pl[3], full.reshape(h, w, c)[:, :, 3])
                passed += 1
    assert passed >= 4   # (every fixed-mode case at least)


def test_model_without_a_colour_inverse_is_the_decode_itself():
    for c, ycbcr in [(1, True), (2, True), (3, False), (4, False)]:
        s = ol.oracle_encode(_picture("randtile", 40, 72, c), 50, ycbcr)
        assert pm.header(s)[3] == 0
        rc, pl = pm.planes(s, fix_t2=True)
        assert rc == 0 and np.array_equal(pl.transpose(1, 2, 0), ol.oracle_decode(s, fix_t2=True)[1].reshape(72, 40, c))
        assert np.array_equal(pm.select(pl, 1 << (c - 1))[0], pl[c - 1])


def test_planes_bytes_rules():
    for c in range(1, 5):
        for mask in range(1, 1 << c):
            assert himg_amd.planes_bytes(c, mask, 13, 21) == bin(mask).count("1") * 13 * 21
    assert himg_amd.planes_bytes(4, 0xF, 16384, 16384) == 4 << 28
    bad = [(4, 0, 8, 8), (4, 0x10, 8, 8), (4, 0x11, 8, 8), (3, 0x8, 8, 8), (3, 0xF, 8, 8), (1, 0x2, 8, 8), (2, 0x4, 8, 8),
           (4, 0x80000000, 8, 8), (0, 1, 8, 8), (5, 1, 8, 8), (-1, 1, 8, 8), (4, 1, 0, 8), (4, 1, 8, 0), (4, 1, -3, 8),
           (4, 1, 8, -1)]
    for args in bad:
        with pytest.raises(himg_amd.HimgError) as e:
            himg_amd.planes_bytes(*args)
        assert e.value.code == himg_amd.HIMG_ERR_ARG, args
    assert himg_amd.lib().himg_hip_planes_bytes(4, 1, 8, 8, None) == himg_amd.HIMG_ERR_ARG


def test_peek_format():
    seen = set()
    for name, rec in sorted(gu.GOLDEN.items()):
        if "fixture" not in rec:
            continue
        b = gu.fixture(rec)
        cs = 1 if rec["ycbcr"] and rec["channels"] >= 3 else 0
        assert himg_amd.peek_format(b) == (rec["width"], rec["height"], rec["channels"], cs), name
        assert pm.header(b) == himg_amd.peek_format(b)
        seen.add(cs)
        if cs:
            for chroma in (False, True):
                assert himg_amd.peek_format(pm.rewrite(b, chroma)) == (rec["width"], rec["height"], rec["channels"], 0)
    assert 1 in seen
    s = ol.oracle_encode(_picture("randtile", 24, 16, 3), 50, False)
    assert himg_amd.peek_format(s) == (24, 16, 3, 0)
    # what himg_hip_peek refuses, it refuses: no RIFF file, a truncated one
    bad = s.copy()
    bad[0] ^= 1
    for broken in (bad, s[:20]):
        with pytest.raises(himg_amd.HimgError) as e:
            himg_amd.peek_format(broken)
        assert e.value.code == himg_amd.HIMG_ERR_FORMAT
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    assert himg_amd.lib().himg_hip_peek_format(s.ctypes.data, s.nbytes, C.byref(w), C.byref(h), C.byref(c), None) == himg_amd.HIMG_ERR_ARG


def test_symbols_exported_and_declared():
    L = himg_amd.lib()
    header = open(os.path.join(ROOT, "include", "himg_hip.h")).read()
    for name in SYMBOLS:
        assert getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    for name in ("planes_bytes", "peek_format"):
        assert callable(getattr(himg_amd, name))
    for name in ("decode_planes", "decode_planes_device"):
        assert callable(getattr(himg_amd.Engine, name))
    # what the entry points refuse before they look at a device
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    assert L.himg_hip_decode_planes_to(None, b"RIFF", 4, 1, None, 0, C.byref(w), C.byref(h), C.byref(c)) == himg_amd.HIMG_ERR_ARG
    assert L.himg_hip_decode_planes_device(None, None, 0, None, 1, 8, 8, 4, 1, None, None, None) == himg_amd.HIMG_ERR_ARG


def test_dhimg_g_argument_clashes(tools, tmp_path):
    """-g stands alone, like -m and -c: with another option it is a bad argument (usage, exit 0) whatever
    the order, and nothing is read or written -- the input does not even exist."""
    _, dhimg = tools
    src, out = str(tmp_path / "missing.himg"), str(tmp_path / "o.pgm")
    clashes = [["-g", "-s2"], ["-s4", "-g"], ["-g", "-t"], ["-t", "-g"], ["-g", "-m"], ["-m", "-g"], ["-c", "-g"],
               ["-g", "-c"], ["-g", "-r", "0,0,4,4"], ["-r", "0,0,4,4", "-g"], ["-g", "-g"]]
    for flags in clashes:
        r = _run(dhimg, *flags, src, out)
        assert r.returncode == 0 and r.stdout == "Usage: %s image outfile\n" % dhimg, (flags, r.stdout)
        assert not os.listdir(str(tmp_path)), flags
    r = _run(dhimg, "-g", src, out)
    assert r.returncode == 255 and r.stdout == "Unable to read file %s\n" % src
