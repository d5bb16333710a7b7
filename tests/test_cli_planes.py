"""GPU (-m gpu): dhimg -g writes plane 0 of the stream -- the codec's own luma for a colour-space-1
stream -- as a PGM: the model's plane 0 (tests/planes_model.py), its rows flipped as dhimg flips every
picture it writes."""
import numpy as np
import pytest

import golden_util as gu
import oracle_lib as ol
import planes_model as pm
from test_cli import _read_pnm, _run, tools  # noqa: F401  (tools: the fixture)

pytestmark = pytest.mark.gpu


def test_dhimg_grey(tools, tmp_path):
    _, dhimg = tools
    b = gu.fixture(gu.GOLDEN["randtile_s0_64x64_q50"])
    assert pm.header(b) == (64, 64, 4, 1) and ol.oracle_decode(b)[0] == 0
    src, out = str(tmp_path / "in.himg"), str(tmp_path / "luma.pgm")
    b.tofile(src)
    r = _run(dhimg, "-g", src, out)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines() == ["File size: %d" % b.size]
    assert open(out, "rb").read(2) == b"P5"
    got = _read_pnm(out)
    rc, model = pm.planes(b)
    assert rc == 0 and got.shape == (64, 64, 1)
    assert np.array_equal(got[:, :, 0], model[0][::-1])
    # not the luma recomputed from anything behind the colour inverse: the full decode's first channel differs
    full = str(tmp_path / "full.pam")
    assert _run(dhimg, src, full).returncode == 0
    assert not np.array_equal(_read_pnm(full)[:, :, 0], got[:, :, 0])
    # a damaged stream: the decoder's message, no file
    bad = b.copy()
    bad[0] ^= 0x01
    bad.tofile(str(tmp_path / "bad.himg"))
    r = _run(dhimg, "-g", str(tmp_path / "bad.himg"), str(tmp_path / "bad.pgm"))
    assert r.returncode == 255 and r.stdout.splitlines()[-1] == "Unable to decode image."
    assert not (tmp_path / "bad.pgm").exists()
