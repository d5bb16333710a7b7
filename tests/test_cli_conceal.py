"""GPU (-m gpu): dhimg -c decodes a damaged file -- the block rows the decoder accepts, the others from the
low-res plane -- and names the concealed rows on stderr; without -c the same file is rejected as before; a
clean file through -c is the plain decode."""
import numpy as np
import pytest

import conceal_model as cm
import damage_model as dm
from test_cli import _freeimage_order, _read_pnm, _run, tools  # noqa: F401  (tools: the fixture)

pytestmark = pytest.mark.gpu

NAME = "randtile256x72"


def test_dhimg_damaged_file(tools, tmp_path):
    _, dhimg = tools
    m = dm.good_model(NAME)
    i = next(i for i, (_, rowmap) in enumerate(cm.corpus(NAME, "P")) if 0 < rowmap.sum() < m.rows)
    bad, (want, rowmap) = dm.streams(NAME, "P")[i].bad, cm.corpus(NAME, "P")[i]
    src, out = str(tmp_path / "bad.himg"), str(tmp_path / "bad.pam")
    bad.tofile(src)
    r = _run(dhimg, "-c", src, out)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.splitlines() == ["File size: %d" % bad.size]
    err = r.stderr.splitlines()
    k = err.index("concealed %d of %d block rows" % (rowmap.sum(), m.rows))
    assert err[k + 1] == " ".join(str(v) for v in np.flatnonzero(rowmap))
    assert np.array_equal(_freeimage_order(_read_pnm(out)), want)
    # without -c: today's behaviour
    r = _run(dhimg, src, str(tmp_path / "no.pam"))
    assert r.returncode == 255
    assert r.stdout.splitlines()[0] == "File size: %d" % bad.size and r.stdout.splitlines()[-1] == "Unable to decode image."
    assert not (tmp_path / "no.pam").exists()
    # a clean file through -c: byte-identical to the plain decode
    good, a, b = str(tmp_path / "good.himg"), str(tmp_path / "a.pam"), str(tmp_path / "b.pam")
    m.packed.tofile(good)
    r = _run(dhimg, "-c", good, a)
    assert r.returncode == 0 and "concealed 0 of %d block rows" % m.rows in r.stderr.splitlines()
    assert _run(dhimg, good, b).returncode == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    # -c is on its own: with another option it is a bad argument, as -m is
    for extra in (["-s2", "-c"], ["-c", "-r", "0,0,8,8"], ["-t", "-c"], ["-m", "-c"], ["-c", "-m"]):
        r = _run(dhimg, *extra, good, str(tmp_path / "x.pam"))
        assert r.returncode == 0 and r.stdout.startswith("Usage: "), extra
        assert not (tmp_path / "x.pam").exists()
