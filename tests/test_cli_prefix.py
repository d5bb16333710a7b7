"""GPU (-m gpu): dhimg -t decodes a truncated file -- the block rows that are whole, the rest from the
low-res plane -- and says how many rows it had; without -t the same file is rejected as before."""
import numpy as np
import pytest

import golden_util as gu
import prefix_model as pm
from test_cli import _freeimage_order, _read_pnm, _run, tools  # noqa: F401  (tools: the fixture)

pytestmark = pytest.mark.gpu


def test_dhimg_truncated_file(tools, tmp_path):
    _, dhimg = tools
    b = gu.fixture(gu.GOLDEN["randtile_s0_64x64_q50"])
    m = pm.Model(b)
    avail = b.size * 6 // 10
    code, k, want = m.expect(avail)
    assert code == 0 and 0 < k < 8
    cut, out = str(tmp_path / "cut.himg"), str(tmp_path / "cut.pam")
    b[:avail].tofile(cut)
    r = _run(dhimg, "-t", cut, out)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines() == ["File size: %d" % avail, "block rows %d of 8" % k]
    assert np.array_equal(_freeimage_order(_read_pnm(out)), want)
    # without -t: today's behaviour and message
    r = _run(dhimg, cut, str(tmp_path / "no.pam"))
    assert r.returncode == 255
    assert r.stdout.splitlines() == ["File size: %d" % avail, "Not a RIFF HIMG file.", "Unable to decode image."]
    assert not (tmp_path / "no.pam").exists()
    # the whole file through -t: the full decode
    whole, out2 = str(tmp_path / "whole.himg"), str(tmp_path / "whole.pam")
    b.tofile(whole)
    r = _run(dhimg, "-t", whole, out2)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "block rows 8 of 8"
    assert np.array_equal(_freeimage_order(_read_pnm(out2)), m.full)
    # a file that ends before the first block row: an error, no picture
    short = str(tmp_path / "short.himg")
    b[:100].tofile(short)
    r = _run(dhimg, "-t", short, str(tmp_path / "short.pam"))
    assert r.returncode == 255 and r.stdout.splitlines()[-1] == "Unable to decode image."
    assert not (tmp_path / "short.pam").exists()
