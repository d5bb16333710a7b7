"""Encode to a byte budget, the parts that need no GPU: the probe count against the model, the
exported symbols, the model's search on the oracle's sizes (with the inversions the header speaks
of), and the command line of chimg -b."""
import ctypes as C
import functools
import subprocess

import pytest

import himg_amd
from himg_amd import build as hb

import budget_model as bm
import oracle_lib as ol

KINDS = [("randtile", 1), ("gradn", 1), ("rand", 3)]


@functools.lru_cache(maxsize=None)
def oracle_sizes(kind, seed, w, h, ycc):
    img = himg_amd.synth(kind, seed, w, h)
    return tuple(int(ol.oracle_encode(img, q, ycc).size) for q in range(101))


def test_probe_count_matches_the_model():
    L = himg_amd.lib()
    for qmin in range(101):
        for qmax in range(qmin, 101):
            want = bm.probe_count(qmin, qmax)
            n = L.himg_hip_budget_probes(qmin, qmax)
            assert n == want == himg_amd.budget_probes(qmin, qmax), (qmin, qmax, n, want)
            # no frame takes more probes than that; the hardest one -- everything below qmax fits, so
            # that the bisection keeps the larger half every time -- takes exactly that many
            hardest = lambda q, qmax=qmax: 1 << 40 if q == qmax else 0
            assert len(bm.search(hardest, 10, qmin, qmax)[1]) == (want if qmax > qmin else 1), (qmin, qmax)
            for other in (lambda q: 0, lambda q: 1 << 40, lambda q, qmin=qmin: 0 if q == qmin else 1 << 40):
                assert len(bm.search(other, 10, qmin, qmax)[1]) <= want, (qmin, qmax)
    assert L.himg_hip_budget_probes(0, 100) == 9
    for bad in ((-1, 50), (0, 101), (60, 40), (-5, -5), (101, 101)):
        assert L.himg_hip_budget_probes(*bad) == himg_amd.HIMG_ERR_ARG, bad
        with pytest.raises(himg_amd.HimgError):
            himg_amd.budget_probes(*bad)


def test_symbols_are_exported():
    L = C.CDLL(himg_amd.LIB)
    for name in ("himg_hip_encode_device_q", "himg_hip_encode_sizes_device", "himg_hip_budget_probes",
                 "himg_hip_encode_budget_device", "himg_hip_encode_budget_to", "himg_hip_encode_budget_batch"):
        assert hasattr(L, name), name


def test_model_on_the_oracles_sizes():
    """For every budget the result fits or is -1, -1 exactly when the stream at qmin does not fit;
    and the size is not monotone in the quality (what the header says about the search's result)."""
    any_inversion = False
    for kind, seed in KINDS:
        for ycc in (True, False):
            s = oracle_sizes(kind, seed, 64, 64, ycc)
            inv = bm.inversions(s)
            any_inversion = any_inversion or bool(inv)
            budgets = [s[0] - 1, s[0], s[50] - 1, s[50], s[100], 1 << 30]
            budgets += [s[q] - 1 for q in inv] + [s[q + 1] for q in inv]
            for qmin, qmax in ((0, 100), (40, 60), (50, 50), (0, 1), (99, 100)):
                for b in budgets:
                    q, probes = bm.search(lambda x: s[x], b, qmin, qmax)
                    assert len(probes) <= bm.probe_count(qmin, qmax)
                    assert (q == -1) == (s[qmin] > b), (kind, ycc, qmin, qmax, b)
                    if q >= 0:
                        assert qmin <= q <= qmax and s[q] <= b, (kind, ycc, qmin, qmax, b, q)
                        assert q == qmax or s[q + 1] > b or q + 1 not in probes, (kind, ycc, qmin, qmax, b, q)
    assert any_inversion, "none of the pictures has size(q + 1) < size(q): the header's remark would be wrong"


def test_chimg_budget_arguments():
    chimg = hb.build_cli()[0]
    run = lambda *a: subprocess.run([chimg, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    r = run()
    assert r.returncode == 0 and " -b <bytes>   Fit the file into a byte budget" in r.stdout
    r = run("-b", "x7", "a", "b")
    assert r.returncode == 0 and r.stdout.startswith("Invalid integer expression: x7\nUsage: %s [options] image outfile\n" % chimg)
    r = run("-b", "-5", "a", "b")
    assert r.returncode == 0 and r.stdout.startswith("Invalid byte budget: -5\nUsage:")
    r = run("a", "b", "-b")
    assert r.returncode == 0 and r.stdout.startswith("Usage:")
