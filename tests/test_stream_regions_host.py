"""CPU: himg_hip_stream_regions_peek -- every window's plan is region_peek's, the ranges are the sorted,
disjoint union of the head and the windows' rows -- its error codes, and a model check, with the oracle alone,
that the independence cases test_gpu_stream_regions.py runs are not vacuous."""
import ctypes as C

import numpy as np
import pytest

import himg_amd
import damage_model as dm
import stream_region_cases as sc


def _union(ranges):
    out = []
    for a, e in sorted(ranges):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([a, e])
    return [tuple(r) for r in out]


@pytest.mark.parametrize("kind,W,H,Cn,q,win", [("randtile", 96, 72, 4, 50, (24, 17)), ("gradn", 50, 41, 3, 90, (24, 17)),
                                               ("randtile", 96, 72, 4, 50, (1, 1)), ("gradn", 50, 41, 3, 90, (50, 41))])
def test_plans_are_region_peeks_and_ranges_their_union(kind, W, H, Cn, q, win):
    s = sc.stream(kind, W, H, Cn, q)
    org = [tuple(int(v) for v in o) for o in sc.origins12(W, H, *win, np.random.default_rng(3))]
    assert len(org) == 12
    plans, ranges = himg_amd.stream_regions_peek(s, org, *win)
    want = [himg_amd.region_peek(s, x, y, *win) for x, y in org]
    assert plans == want
    assert all(a < e for a, e in ranges) and all(ranges[i][1] < ranges[i + 1][0] for i in range(len(ranges) - 1))
    assert ranges == _union([(0, want[0]["head_bytes"])] + [(p["rows_begin"], p["rows_end"]) for p in want])
    assert ranges[-1][1] <= len(s)


def test_error_codes():
    s = sc.stream()
    L = himg_amd.lib()
    # a bad rectangle: that window alone has no plan
    plans, ranges = himg_amd.stream_regions_peek(s, [(0, 0), (sc.W - 23, 0), (5, 55)], *sc.WIN)
    assert plans[1] == himg_amd.HIMG_ERR_ARG and plans[0] == himg_amd.region_peek(s, 0, 0, *sc.WIN)
    assert plans[2] == himg_amd.region_peek(s, 5, 55, *sc.WIN)
    org = np.array([(0, 0), (sc.W - 23, 0)], np.int32)
    pl = (himg_amd.RegionPlan * 2)()
    rng = np.zeros(6, np.uintp)
    n = C.c_int(-1)
    rc = L.himg_hip_stream_regions_peek(s.ctypes.data, s.nbytes, 0, 2, org.ctypes.data, 24, 17, pl, rng.ctypes.data, C.byref(n))
    assert rc == himg_amd.HIMG_ERR_ARG and n.value == 1   # (the first failing window's code; window 0's rows start where the head ends)
    assert L.himg_hip_stream_regions_peek(s.ctypes.data, s.nbytes, 0, 0, org.ctypes.data, 24, 17, pl, rng.ctypes.data,
                                          C.byref(n)) == himg_amd.HIMG_ERR_ARG
    assert L.himg_hip_stream_regions_peek(None, 0, 0, 2, org.ctypes.data, 24, 17, pl, rng.ctypes.data,
                                          C.byref(n)) == himg_amd.HIMG_ERR_ARG
    # a header chain that breaks at row 5: the windows with r1 <= 5 keep their plans, the others are FORMAT
    bad = sc.header_overruns(s.copy(), 5)
    so, org = sc.windows()
    org = org[so == 0]
    plans, ranges = himg_amd.stream_regions_peek(bad, org, *sc.WIN)
    r1 = [(int(y) + sc.WIN[1] + 7) // 8 for _, y in org]
    assert any(r <= 5 for r in r1) and any(r > 5 for r in r1)
    for p, (x, y), r in zip(plans, org, r1):
        if r <= 5:
            assert p == himg_amd.region_peek(s, int(x), int(y), *sc.WIN)
        else:
            assert p == himg_amd.HIMG_ERR_FORMAT
    good = [p for p in plans if isinstance(p, dict)]
    assert ranges == _union([(0, good[0]["head_bytes"])] + [(p["rows_begin"], p["rows_end"]) for p in good])
    # a stream that is none: every window FORMAT, no range
    plans, ranges = himg_amd.stream_regions_peek(np.zeros(64, np.uint8), org, *sc.WIN)
    assert plans == [himg_amd.HIMG_ERR_FORMAT] * len(org) and ranges == []


@pytest.mark.parametrize("name", ["payload", "header", "cut", "surplus"])
def test_independence_cases_are_not_vacuous(name):
    """By the model alone: within the damaged stream some windows fail and some pass, and the clean stream's all pass."""
    so, org = sc.windows()
    exp = sc.expected(name)
    codes0 = [c for (c, _), s in zip(exp, so) if s == 0]
    assert dm.FORMAT in codes0 and dm.OK in codes0, codes0
    assert all(c == dm.OK for (c, _), s in zip(exp, so) if s == 1)
    # what each case is meant to hit
    r = [(int(y) // 8, (int(y) + sc.WIN[1] + 7) // 8) for (_, y), s in zip(org, so) if s == 0]
    fails = [c == dm.FORMAT for c in codes0]
    rule = {"payload": lambda a, b: a <= 4 < b, "header": lambda a, b: b > 5, "cut": lambda a, b: b > 6,
            "surplus": lambda a, b: b == sc.ROWS}[name]
    assert fails == [rule(a, b) for a, b in r], (name, r, fails)


def test_head_case_fails_in_a_head_stage():
    assert all(c == dm.FORMAT for (c, _), s in zip(sc.expected("head"), sc.windows()[0]) if s == 0)
