"""Encode to a distortion target, the parts that need no GPU: himg_hip_psnr_to_sse against its
formula, the exported symbols, the definition of sse(q) on the oracle (the fixed decode is the picture
a stream defines), its inversions, the model's search and the pinned example of the header."""
import ctypes as C
import functools
import math
import subprocess

import numpy as np
import pytest

import himg_amd
from himg_amd import build as hb

import budget_model as bm
import oracle_lib as ol
import target_model as tm

# kind, seed, width, height, channels, use_ycbcr
PICTURES = [
    ("randtile", 1, 64, 64, 4, True),
    ("gradn", 1, 64, 64, 4, True),
    ("rand", 3, 64, 64, 4, True),
    ("grad", 0, 64, 64, 4, True),
    ("gradn", 2, 64, 64, 4, False),
    ("randtile", 2, 40, 24, 3, True),
    ("gradn", 1, 40, 24, 1, True),
    ("randtile", 1, 100, 52, 4, True),
]


def picture(kind, seed, w, h, ch):
    return np.ascontiguousarray(himg_amd.synth(kind, seed, w, h)[:, :, :ch])


@functools.lru_cache(maxsize=None)
def curve(kind, seed, w, h, ch, ycc):
    """(sse(q) for q = 0 .. 100 from the fixed decode, the number of streams the unfixed decode rejects);
    asserts what the definition rests on along the way."""
    img = picture(kind, seed, w, h, ch)
    out, rejected = [], 0
    for q in range(101):
        stream = ol.oracle_encode(img, q, ycc, channels=ch, stride=ch)
        rc, dec = ol.oracle_decode(stream, fix_t2=True)
        assert rc == 0, (kind, seed, q, rc)
        rc_ref, dec_ref = ol.oracle_decode(stream)
        if rc_ref != 0:
            rejected += 1
        else:
            assert np.array_equal(dec, dec_ref), (kind, seed, q)
        out.append(tm.sse(img, dec.reshape(img.shape)))
    return tuple(out), rejected


def test_symbols_are_exported():
    L = C.CDLL(himg_amd.LIB)
    for name in ("himg_hip_encode_sse_device", "himg_hip_encode_target_device", "himg_hip_encode_target_to",
                 "himg_hip_encode_target_batch", "himg_hip_psnr_to_sse"):
        assert hasattr(L, name), name
    assert himg_amd.HIMG_ERR_TARGET == -6
    for name in ("encode_sse_device", "encode_target_device", "encode_target", "encode_target_batch"):
        assert hasattr(himg_amd.Engine, name), name


def test_psnr_to_sse():
    for w, h, ch in ((8, 8, 1), (64, 64, 4), (100, 52, 3), (4096, 4096, 4), (16384, 16384, 4), (1, 1, 1)):
        for db in (0.0, 1.0, 20.0, 30.0, 33.3, 40.0, 48.13, 60.0, 99.0, 150.0, 400.0):
            want = int(math.floor(255.0 * 255.0 * (float(w) * float(h) * float(ch)) / math.pow(10.0, db / 10.0)))
            got = himg_amd.psnr_to_sse(db, w, h, ch)
            assert got == want, (w, h, ch, db, got, want)
            if got > 0:
                # himg_amd.psnr's formula at SSE = got: the target is at least the dB asked for
                reached = 10.0 * np.log10(255.0 * 255.0 / (got / (float(w) * h * ch)))
                assert reached >= db - 1e-9, (w, h, ch, db, reached)
    assert himg_amd.psnr_to_sse(400.0, 64, 64, 4) == 0   # (allowed: it asks for a lossless result)
    out = C.c_uint64(7)
    L = himg_amd.lib()
    for bad in ((float("nan"), 64, 64, 4), (float("inf"), 64, 64, 4), (-0.5, 64, 64, 4), (-float("inf"), 64, 64, 4),
                (30.0, 0, 64, 4), (30.0, 64, -1, 4), (30.0, 64, 64, 0), (30.0, 64, 64, 5)):
        assert L.himg_hip_psnr_to_sse(*bad, C.byref(out)) == himg_amd.HIMG_ERR_ARG, bad
        assert out.value == 7
        with pytest.raises(himg_amd.HimgError):
            himg_amd.psnr_to_sse(*bad)
    assert L.himg_hip_psnr_to_sse(30.0, 64, 64, 4, None) == himg_amd.HIMG_ERR_ARG


def test_the_fixed_decode_defines_the_picture():
    """Every stream decodes with the fix; where the unfixed decode accepts one, its pixels are the
    same (asserted in curve()); and the unfixed decode does reject streams of the encoder's own."""
    rejected = [curve(*p)[1] for p in PICTURES]
    assert max(rejected) > 0, rejected


def test_sse_is_not_monotone():
    for p in PICTURES:
        inv = tm.inversions(curve(*p)[0])
        assert inv, (p, "sse(q + 1) <= sse(q) everywhere: the header's remark would be wrong")


def test_model_on_the_oracles_curves():
    for p in PICTURES:
        s = curve(*p)[0]
        inv = tm.inversions(s)
        targets = [0, min(s) - 1, min(s), s[100] - 1, s[100], s[50], s[50] - 1, s[0], s[0] - 1, 1 << 63]
        targets += [s[q] for q in inv] + [s[q + 1] - 1 for q in inv]
        for qmin, qmax in ((0, 100), (20, 80), (37, 37), (0, 1), (99, 100), (0, 86)):
            want = bm.probe_count(qmin, qmax)
            assert himg_amd.lib().himg_hip_budget_probes(qmin, qmax) == want
            for t in targets:
                q, probes = tm.search(lambda x: s[x], t, qmin, qmax)
                assert len(probes) <= want, (p, qmin, qmax, t)
                assert (q == -1) == (s[qmax] > t), (p, qmin, qmax, t)
                if q >= 0:
                    assert qmin <= q <= qmax and s[q] <= t, (p, qmin, qmax, t, q)
                    assert q == qmin or s[q - 1] > t or q - 1 not in probes, (p, qmin, qmax, t, q)


def test_probe_lists_never_exceed_the_count():
    for qmin in range(0, 101, 7):
        for qmax in range(qmin, 101):
            want = himg_amd.budget_probes(qmin, qmax)
            # the hardest frame -- nothing below qmax meets the target, so that the bisection keeps the
            # larger (upper) half every time -- takes exactly that many
            hardest = lambda q, qmax=qmax: 0 if q == qmax else 1 << 40
            assert len(tm.search(hardest, 10, qmin, qmax)[1]) == (want if qmax > qmin else 1), (qmin, qmax)
            for other in (lambda q: 0, lambda q: 1 << 40, lambda q, qmin=qmin: 1 << 40 if q == qmin else 0):
                assert len(tm.search(other, 10, qmin, qmax)[1]) <= want, (qmin, qmax)


def test_pinned_example():
    """rand, seed 3, 64 x 64 RGBA YCbCr: the minimum 47 717 at q = 86, 66 146 at q = 100 -- a target of
    50 000 fails for 0 .. 100 and succeeds for 0 .. 86."""
    s = curve("rand", 3, 64, 64, 4, True)[0]
    assert s[100] == 66146 and s[86] == 47717 and min(s) == 47717
    assert tm.search(lambda q: s[q], 50000, 0, 100)[0] == -1
    q = tm.search(lambda q: s[q], 50000, 0, 86)[0]
    assert 0 <= q <= 86 and s[q] <= 50000


def test_chimg_target_arguments():
    chimg = hb.build_cli()[0]
    run = lambda *a: subprocess.run([chimg, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    r = run()
    assert r.returncode == 0 and " -p <dB>      Reach at least this PSNR" in r.stdout
    r = run("-p", "x7", "a", "b")
    assert r.returncode == 0 and r.stdout.startswith("Invalid number: x7\nUsage: %s [options] image outfile\n" % chimg)
    r = run("-p", "-5", "a", "b")
    assert r.returncode == 0 and r.stdout.startswith("Invalid PSNR: -5\nUsage:")
    r = run("-p", "30", "-b", "1000", "a", "b")
    assert r.returncode == 0 and r.stdout.startswith("-b and -p exclude each other\nUsage:")
    r = run("a", "b", "-p")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
