"""GPU (-m gpu): dhimg -m writes the picture pyramid from one decode -- the full picture where dhimg
writes it, levels 1 to 3 beside it as out.L1.ext, out.L2.ext, out.L3.ext -- and each file is what
dhimg, dhimg -s2 and dhimg -s4 write for the same stream (level 3: the engine's preview)."""
import numpy as np
import pytest

import golden_util as gu
from test_cli import _freeimage_order, _read_pnm, _run, tools  # noqa: F401  (tools: the fixture)

pytestmark = pytest.mark.gpu


def test_dhimg_pyramid(tools, engine, tmp_path):
    _, dhimg = tools
    b = gu.fixture(gu.GOLDEN["randtile_s0_64x64_q50"])
    src = str(tmp_path / "in.himg")
    b.tofile(src)
    out = str(tmp_path / "pyr.pam")
    r = _run(dhimg, "-m", src, out)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines() == ["File size: %d" % b.size]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.himg", "pyr.L1.pam", "pyr.L2.pam", "pyr.L3.pam", "pyr.pam"]
    for flags, name in [([], "pyr.pam"), (["-s2"], "pyr.L1.pam"), (["-s4"], "pyr.L2.pam")]:
        one = str(tmp_path / ("one" + name))
        r = _run(dhimg, *flags, src, one)
        assert r.returncode == 0, (flags, r.stdout)
        want, got = _read_pnm(one), _read_pnm(str(tmp_path / name))
        assert got.shape == want.shape and np.array_equal(got, want), (flags, name)
    assert _read_pnm(out).shape[:2] == (64, 64) and _read_pnm(str(tmp_path / "pyr.L1.pam")).shape[:2] == (32, 32)
    assert _read_pnm(str(tmp_path / "pyr.L2.pam")).shape[:2] == (16, 16)
    low = _read_pnm(str(tmp_path / "pyr.L3.pam"))
    assert low.shape[:2] == (8, 8)
    assert np.array_equal(_freeimage_order(low), engine.preview(b))
    # an output name without an extension: the level goes behind it
    r = _run(dhimg, "-m", src, str(tmp_path / "plain"))
    assert r.returncode == 0 and (tmp_path / "plain.L3").exists() and (tmp_path / "plain").exists()
    # a damaged stream: the decoder's message, no files
    bad = b.copy()
    bad[0] ^= 0x01
    bad.tofile(str(tmp_path / "bad.himg"))
    r = _run(dhimg, "-m", str(tmp_path / "bad.himg"), str(tmp_path / "bad.pam"))
    assert r.returncode == 255 and r.stdout.splitlines()[-1] == "Unable to decode image."
    assert not (tmp_path / "bad.pam").exists() and not (tmp_path / "bad.L1.pam").exists()
