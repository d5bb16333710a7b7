"""The reference's own `benchmark` main RUNS against the engine ("missing" #3).

oracle/_ref/ref_benchmark is the reference's src/benchmark.cpp, compiled where it lies
and unchanged by oracle/Makefile (himg_amd.build.build_ref_benchmark()) at build time, linked
against libhimg_hip.so (himg::Decoder) and a test-only FreeImage link stub whose loaders
fail -- so the only branch of that main that can work is the one a .himg file takes:
IsHimg -> himg::Decoder::Decode, 30 iterations (src/benchmark.cpp:21,108-126), then the
Min / Max / Average lines (src/benchmark.cpp:150-154).  The binary travels to the GPU
machine with the rest of oracle/_ref/; the reference sources do not, and nothing here reads them."""
import os
import re
import subprocess

import numpy as np
import pytest

import himg_amd
from himg_amd import build as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exe():
    exe = hb.build_ref_benchmark()
    if not exe or not os.path.exists(exe):
        pytest.skip("ref_benchmark not built (no reference sources at build time)")
    return exe


def test_ref_benchmark_binary_is_the_reference_main():
    """CPU side: the binary exists after build() and needs the engine's Decoder symbols."""
    exe = _exe()
    out = subprocess.run(["nm", "-C", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    assert "himg::Decoder::Decode(unsigned char const*, int)" in out
    assert "himg::Decoder::Decoder(int)" in out
    # no FreeImage left undefined: the stub satisfies the link
    assert "FreeImage_" not in out


@pytest.mark.gpu
def test_reference_benchmark_decodes_a_himg_file(tmp_path):
    exe = _exe()
    eng = himg_amd.Engine(0)
    img = himg_amd.synth("randtile", 3, 1024, 512)
    packed = eng.encode(img, 50, True)
    eng.close()
    path = str(tmp_path / "frame.himg")
    np.asarray(packed, np.uint8).tofile(path)
    r = subprocess.run([exe, "-d", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "File size: %d" % packed.size in out
    assert "Unable to decode image." not in out
    # 30 iterations, each through himg::Decoder::Decode (src/benchmark.cpp:21,111-126)
    assert out.count("Iteration ") == 30 and "Iteration 30/30" in out
    vals = {}
    for key in ("Min", "Max", "Average"):
        m = re.search(r"^\s*%s: ([0-9.eE+-]+) ms$" % key, out, re.M)
        assert m, out[-400:]
        vals[key] = float(m.group(1))
    assert 0.0 < vals["Min"] <= vals["Average"] <= vals["Max"]


@pytest.mark.gpu
def test_reference_benchmark_rejects_what_the_reference_rejects(tmp_path):
    """A stream the reference decoder refuses (T2: the pure gradient compresses below one
    block row) makes the reference main print its failure line and exit with -1."""
    exe = _exe()
    golden = os.path.join(ROOT, "tests", "golden", "grad_s0_64x64_q50.himg")
    r = subprocess.run([exe, "-d", golden], capture_output=True, text=True, timeout=300)
    assert "Unable to decode image." in r.stdout
    assert r.returncode != 0
