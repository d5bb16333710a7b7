"""CPU: scaled windows on an opened-streams handle -- the two entries in the ABI and their host-only refusals; a
model check, with the oracle alone, that the cases of test_gpu_opened_scaled.py are not vacuous (which of the
independence windows fail at each scale, the row arithmetic of the shared-counts test); and
OpenedRows::pending (himg_amd/csrc/opened_plan.h) fed the rectangles R^ of scaled windows, driven by
tools/micro/opened_scaled_plan_check.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import himg_amd
import damage_model as dm
import opened_scaled_cases as oc
import stream_region_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = himg_amd.HIMG_ERR_ARG


def test_abi_has_the_scaled_entries():
    L = himg_amd.lib()
    for name in ["himg_hip_opened_scaled_regions_device", "himg_hip_opened_scaled_regions_to"]:
        assert hasattr(L, name), name
        assert name in open(os.path.join(ROOT, "include", "himg_hip.h")).read()
    for name in ["scaled_regions_device", "scaled_regions"]:
        assert callable(getattr(himg_amd.OpenedStreams, name))


def test_null_handle_or_context_is_an_argument_error():
    """Refused on the host, without a device: no context, no handle, and a handle that no context owns."""
    L = himg_amd.lib()
    so, org = np.zeros(1, np.int32), np.zeros(2, np.int32)
    st = np.full(1, 7, np.int32)
    dst = np.full(64, 0x77, np.uint8)
    wo, ho, co = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    for s in (0, 1, 2, 3, 4, -1):
        for ctx, h in [(None, None), (None, C.c_void_p(8)), (C.c_void_p(0), C.c_void_p(8))]:
            assert L.himg_hip_opened_scaled_regions_device(ctx, h, s, so.ctypes.data, org.ctypes.data, 1, 1, 1, dst.ctypes.data,
                                                           st.ctypes.data, None) == ARG, (s, ctx, h)
            assert L.himg_hip_opened_scaled_regions_to(ctx, h, s, 1, so.ctypes.data, org.ctypes.data, 1, 1, dst.ctypes.data,
                                                       dst.nbytes, st.ctypes.data, C.byref(wo), C.byref(ho),
                                                       C.byref(co)) == ARG, (s, ctx, h)
    assert (dst == 0x77).all() and st[0] == 7 and (wo.value, ho.value, co.value) == (-1, -1, -1)


@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("name", ["payload", "header", "cut", "surplus", "head"])
def test_independence_cases_are_not_vacuous(name, s):
    """At each scale some windows fail and some pass, and -- unless the head fails all of them -- both kinds are
    among the damaged stream's windows: each of the two calls the GPU test splits them into holds windows."""
    so, org = oc.windows(s)
    w, h = oc.WIN[s]
    ow, oh = oc.size(sc.W, sc.H, s)
    assert (ow, oh) == himg_amd.scaled_size(sc.W, sc.H, s)
    assert all(0 <= x and x + w <= ow and 0 <= y and y + h <= oh for x, y in org)
    # the scaled windows touch the block rows of the full-resolution windows they come from
    assert [oc.rows_of(s, int(y), h) for _, y in org] == [oc.rows_of(0, int(y), sc.WIN[1]) for _, y in sc.windows()[1]]
    codes = [c for c, _ in oc.expected(name, s)]
    assert dm.FORMAT in codes and dm.OK in codes, codes
    assert all(c == dm.OK for c, k in zip(codes, so) if k == 1)
    codes0 = [c for c, k in zip(codes, so) if k == 0]
    if name == "head":
        assert all(c == dm.FORMAT for c in codes0)
    else:
        assert dm.FORMAT in codes0 and dm.OK in codes0
        for (c, crop), k in zip(oc.expected(name, s), so):
            assert (crop is not None and crop.shape == (h, w, sc.C)) == (c == dm.OK)


def test_scale_3_windows_lie_inside_the_low_res_picture():
    w, h = oc.WIN[3]
    cols, rows = oc.size(sc.W, sc.H, 3)
    assert (cols, rows) == ((sc.W + 7) // 8, (sc.H + 7) // 8)
    assert all(0 <= x and x + w <= cols and 0 <= y and y + h <= rows for x, y in oc.windows(3)[1])


def test_row_arithmetic_of_the_shared_counts():
    """The steps of the shared-counts test touch the rows they say, inside their pictures, and a model of the
    bitmap gives the launches and rows_counted they expect."""
    counted = set()
    for s, (x, y), (w, h), rows, launches, total in oc.COUNT_STEPS:
        ow, oh = oc.size(sc.W, sc.H, s)
        assert 0 <= x and x + w <= ow and 0 <= y and y + h <= oh
        new = set()
        if s != 3:
            assert oc.rows_of(s, y, h) == rows
            new = set(range(*rows)) - counted
        assert (1 if new else 0) == launches
        counted |= new
        assert len(counted) == total
    assert [r for _, _, _, r, _, _ in oc.COUNT_STEPS] == [(2, 5), (2, 5), (3, 7), None, (2, 7)]


# ---- OpenedRows::pending fed R^ ---------------------------------------------------------------------------

def _build(tmp_path, *flags):
    exe = str(tmp_path / "opened_scaled_plan_check")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "himg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "micro", "opened_scaled_plan_check.cpp"), "-o", exe], check=True)
    return exe


def _sequences():
    """(n_streams, rows, H, [(scale, h, [(stream, x, y)])]): single windows of every y mod S and height, then mixed calls."""
    rng = np.random.default_rng(43)
    out = []
    for n_streams, rows in [(1, 9), (3, 9), (2, 2), (4, 300)]:
        H = 8 * rows - int(rng.integers(0, 8))
        calls = []
        for _ in range(40):
            s = int(rng.integers(0, 3))
            oh = oc.size(1, H, s)[1]
            h = int(rng.integers(1, min(oh, 60) + 1))
            n = 1 if rng.integers(0, 2) else int(rng.integers(2, 20))
            calls.append((s, h, [(int(rng.integers(0, n_streams)), int(rng.integers(0, 50)), int(rng.integers(0, oh - h + 1)))
                                 for _ in range(n)]))
        out.append((n_streams, rows, H, calls))
    # one fresh handle per single window: the run IS the window's rows, [y / S, ceil((y + h) / S))
    H = 72
    for s in (1, 2):
        S, oh = 8 >> s, oc.size(1, H, s)[1]
        for y in list(range(2 * S + 1)) + [oh - 1, oh - S - 1]:
            for h in (1, 2, S - 1 or 1, S, S + 1, oh - y):
                if 1 <= h and y + h <= oh:
                    out.append((2, 9, H, [(s, h, [(1, 3, y)])]))
    return out


def _run_and_compare(exe, seqs):
    text = []
    for n_streams, rows, H, calls in seqs:
        text.append("H %d %d" % (n_streams, rows))
        for s, h, wins in calls:
            text.append("C %d %d %d " % (s, len(wins), h) + " ".join("%d %d %d" % w for w in wins))
    r = subprocess.run([exe], input="\n".join(text) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = iter(r.stdout.splitlines())
    singles = 0
    for n_streams, rows, H, calls in seqs:
        counted = set()
        for s, h, wins in calls:
            v = [int(x) for x in next(lines).split()]
            got = [tuple(v[2 + 3 * i:5 + 3 * i]) for i in range((len(v) - 2) // 3)]
            touched = set()
            for k, _, y in wins:
                r0, r1 = oc.rows_of(s, y, h)
                assert 0 <= r0 < r1 <= rows
                touched |= {(k, r) for r in range(r0, r1)}
            new = sorted(touched - counted)
            assert sorted((k, r) for k, a, b in got for r in range(a, b)) == new, (s, h, wins[:4], got[:4])
            counted |= touched
            assert v[0] == len(new) and v[1] == len(counted)
            if len(calls) == 1 and len(wins) == 1:   # exactly the window's rows, as one run
                k, _, y = wins[0]
                assert got == [(k,) + oc.rows_of(s, y, h)], (s, h, y, got)
                singles += 1
    assert next(lines, None) is None and singles > 40


def test_pending_of_scaled_windows_is_their_rows(tmp_path):
    _run_and_compare(_build(tmp_path), _sequences())


def test_pending_of_scaled_windows_sanitized(tmp_path):
    """The same program under AddressSanitizer and UBSan (a stand-alone host program)."""
    _run_and_compare(_build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), _sequences())
