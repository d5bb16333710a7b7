"""CPU (-m "not gpu"): the host side of the pyramid decode -- himg_hip_pyramid_size against
himg_hip_scaled_size and the preview's geometry, the exported symbols and their declarations, and
dhimg -m's argument clashes, which are refused before the file is read or a device is opened."""
import ctypes as C
import os
import re

import pytest

import himg_amd
from test_cli import _run, tools  # noqa: F401  (tools: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("himg_hip_pyramid_size", "himg_hip_decode_pyramid_device", "himg_hip_decode_pyramid_to")


def test_pyramid_size():
    for w in range(1, 41):
        for h in range(1, 41):
            assert himg_amd.pyramid_size(w, h, 0) == (w, h)
            assert himg_amd.pyramid_size(w, h, 1) == himg_amd.scaled_size(w, h, 1)
            assert himg_amd.pyramid_size(w, h, 2) == himg_amd.scaled_size(w, h, 2)
            assert himg_amd.pyramid_size(w, h, 3) == ((w + 7) // 8, (h + 7) // 8)
    for w, h in [(4096, 4096), (16384, 16383), (2147483647, 5)]:
        for k in range(4):
            f = 1 << k
            assert himg_amd.pyramid_size(w, h, k) == ((w + f - 1) // f, (h + f - 1) // f)


def test_pyramid_size_argument_errors():
    for bad in [(8, 8, -1), (8, 8, 4), (0, 8, 1), (8, 0, 2), (-4, 8, 0), (8, -1, 3)]:
        with pytest.raises(himg_amd.HimgError) as e:
            himg_amd.pyramid_size(*bad)
        assert e.value.code == himg_amd.HIMG_ERR_ARG, bad
    ow, oh = C.c_int(), C.c_int()
    assert himg_amd.lib().himg_hip_pyramid_size(8, 8, 1, None, C.byref(oh)) == himg_amd.HIMG_ERR_ARG
    assert himg_amd.lib().himg_hip_pyramid_size(8, 8, 1, C.byref(ow), None) == himg_amd.HIMG_ERR_ARG


def test_symbols_exported_and_declared():
    L = himg_amd.lib()
    header = open(os.path.join(ROOT, "include", "himg_hip.h")).read()
    for name in SYMBOLS:
        assert getattr(L, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"typedef\s+struct\s+himg_hip_pyramid\s*\{[^}]*void\s*\*\s*level\s*\[\s*4\s*\]", header)
    for name in ("pyramid_size", "pyramid_desc"):
        assert callable(getattr(himg_amd, name))
    for name in ("decode_pyramid", "decode_pyramid_device"):
        assert callable(getattr(himg_amd.Engine, name))
    # the descriptor is four pointers, as the header lays it out
    assert C.sizeof(himg_amd.PyramidDesc) == 4 * C.sizeof(C.c_void_p)
    d = himg_amd.pyramid_desc(None, 0x1000, None, 0x2000)
    assert [d.level[k] for k in range(4)] == [None, 0x1000, None, 0x2000]


def test_pyramid_to_without_a_context_or_a_level():
    """What himg_hip_decode_pyramid_to refuses before it looks at a device."""
    L = himg_amd.lib()
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    dst, cap = (C.c_void_p * 4)(), (C.c_size_t * 4)()
    assert L.himg_hip_decode_pyramid_to(None, b"RIFF", 4, dst, cap, C.byref(w), C.byref(h), C.byref(c)) == himg_amd.HIMG_ERR_ARG
    assert L.himg_hip_decode_pyramid_device(None, None, 0, None, 1, 8, 8, 4, None, None, None) == himg_amd.HIMG_ERR_ARG


def test_dhimg_m_argument_clashes(tools, tmp_path):
    """-m stands alone: with a scale, a rectangle or -t it is a bad argument (usage, exit 0) whatever the
    order, and nothing is read or written -- the input does not even exist."""
    _, dhimg = tools
    src, out = str(tmp_path / "missing.himg"), str(tmp_path / "o.pam")
    clashes = [["-m", "-s2"], ["-s2", "-m"], ["-m", "-s4"], ["-s4", "-m"], ["-m", "-t"], ["-t", "-m"],
               ["-m", "-r", "0,0,4,4"], ["-r", "0,0,4,4", "-m"], ["-s2", "-r", "0,0,4,4", "-m"], ["-m", "-m"]]
    for flags in clashes:
        r = _run(dhimg, *flags, src, out)
        assert r.returncode == 0 and r.stdout == "Usage: %s image outfile\n" % dhimg, (flags, r.stdout)
        assert not os.listdir(str(tmp_path)), flags
    # -m on its own gets as far as the file
    r = _run(dhimg, "-m", src, out)
    assert r.returncode == 255 and r.stdout == "Unable to read file %s\n" % src
