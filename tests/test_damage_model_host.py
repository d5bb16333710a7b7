"""Host: the premises of tests/damage_model.py, proved with the oracle alone on every base of
test_gpu_partial_damage.py, and the host peeks against the model's walk over the whole corpus.

1. Identity: a stream respliced with its own payloads is itself, byte for byte, for every k and every span.
2. Row independence: the oracle accepts a stream damaged in rows J exactly when it accepts each stream
   damaged in one row of J alone, and the accepted picture is the good picture with each row of J taken from
   its single-row decode.  Rows outside J are the good stream's.
3. The oracle's compat fix changes nothing but trap T2 on these bases (damage_model.judge leans on that).
4. Where oracle/_ref is built, the REAL reference gives the oracle's verdict and pixels on a sample of
   respliced streams (whole tiles, no fix: what the reference defines).
5. himg_hip_prefix_peek is prefix_model.walk on every (damaged stream, avail) of the corpus -- the host
   peek's fuzz -- and himg_hip_region_peek says HIMG_ERR_FORMAT exactly where walk_rows does.
6. The corpus reaches what it is for.  Counts by the model alone (damage_model.outcomes, .head_cases), with
   the floors asserted below: 20 per outcome on a base of at least 3 block rows, 5 on a smaller one, where
   the outcome exists (a frame of one block row has no size header, so no class H).

       base             | P: damaged rejected outside same | H: walk past unseen | C: walk head model fres open (not judged)
       randtile256x72   |        182      873    1092    0 |    1051   99    975 |     420  128   716   45    9  (33 + 9)
       gradn61x27       |        351      749    1026    0 |    1146  104    847 |     474   32   808   45    5  (33 + 5)
       rand64x16c1      |        502      647     954    0 |    1243   94    702 |     500   16   793   38    8  (27 + 8)
       randtile4352x24  |         83      522     459    0 |     584   86    372 |     178  116   356    8    0  (6 + 0)
       rand4096x24q100  |        397      191     469    0 |     550   97    394 |     208   68   396    5    1  (4 + 1)
       grad40x40q0      |         55     1018    1003   33 |    1351   67    672 |     495   70   754    8    2  (6 + 2)
       randtile40x8     |        168      312     358    0 |       -    -      - |     261    4   378   24    0  (18 + 0)

   Class C, not judged: the k = 0 prefixes of a stream that fails in the FRES stage (accepted, pixels not
   judged) plus the prefixes left open -- at most 20 % of the class, asserted below.
"""
import numpy as np
import pytest

import damage_model as dm
import himg_amd
import oracle_lib as ol
import prefix_model as pm

NAMES = [b.name for b in dm.BASES]
KEYS = ("width", "height", "num_channels", "rows", "rows_complete", "packed_size", "head_bytes", "used_bytes",
        "next_bytes")


def _payloads(stream, fix):
    b = dm._bytes(stream)
    return [b[o:o + n] for o, n in dm.rows_of(b, fix)[1]]


@pytest.mark.parametrize("name", NAMES)
def test_identity_resplice(name):
    b, m = dm.BASE[name], dm.good_model(name)
    g = m.packed.tobytes()
    assert dm.resplice(g, _payloads(g, b.fix), b.fix) == g
    for k in range(1, m.rows + 1):          # a prefix of k whole rows
        code, img, X = dm.expect_rows(g, g, range(k), b.fix, avail=m.row_ends()[k])
        assert code == dm.OK and X == g and np.array_equal(img, m.full), k
    for r0 in range(m.rows):                # every span of a region
        for r1 in range(r0 + 1, m.rows + 1):
            code, img, X = dm.expect_rows(g, g, range(r0, r1), b.fix)
            assert code == dm.OK and X == g, (r0, r1)


@pytest.mark.parametrize("name", NAMES)
def test_row_independence(name):
    b, m = dm.BASE[name], dm.good_model(name)
    g = m.packed.tobytes()
    good_rows = _payloads(g, b.fix)
    n_acc = n_rej = 0
    for s in dm.streams(name, "P"):
        bad = s.bad.tobytes()
        bad_rows = _payloads(bad, b.fix)                                   # (payload damage moves no header)
        assert dm.resplice(g, bad_rows, b.fix) == bad
        assert [r for r in range(m.rows) if bad_rows[r] != good_rows[r]] == list(s.rows)
        rc, img = dm.judge(bad, b.fix)
        want, ok = m.full.copy(), True
        for r in s.rows:
            rc1, img1 = dm.judge(dm.resplice(g, [bad_rows[i] if i == r else good_rows[i] for i in range(m.rows)], b.fix), b.fix)
            ok = ok and rc1 == 0
            if rc1 == 0:
                assert np.array_equal(img1[:8 * r], m.full[:8 * r]) and np.array_equal(img1[8 * r + 8:], m.full[8 * r + 8:])
                want[8 * r:8 * r + 8] = img1[8 * r:8 * r + 8]
        assert (rc == 0) == ok, s.rows
        if ok:
            assert np.array_equal(img, want), s.rows
            n_acc += 1
        else:
            n_rej += 1
    assert n_acc >= 5 and n_rej >= 5, (n_acc, n_rej)


@pytest.mark.parametrize("name", [b.name for b in dm.BASES if not b.fix])
def test_fix_changes_nothing_else(name):
    m = dm.good_model(name)
    streams = [m.packed] + [s.bad for s in dm.streams(name, "P")[:60]] + [s.bad for s in dm.streams(name, "H")[:60]]
    for s in streams:
        rc0, img0 = ol.oracle_decode(s, fix_t2=False)
        rc1, img1 = ol.oracle_decode(s, fix_t2=True)
        assert (rc0 == 0) == (rc1 == 0)
        if rc0 == 0:
            assert np.array_equal(img0, img1)


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref is not built")
@pytest.mark.parametrize("name", [b.name for b in dm.BASES if not b.fix and b.W % 8 == 0 and b.H % 8 == 0])
def test_reference_judges_respliced_streams_alike(name):
    b, m = dm.BASE[name], dm.good_model(name)
    n_acc = n_rej = 0
    for cls in "PH":
        ss = dm.streams(name, cls)
        for i, rect in dm.region_cases(name, cls)[:len(ss)][::8]:
            code, img, X = dm.expect_rows(m.packed, ss[i].bad, range(rect[1] // 8, (rect[1] + rect[3] + 7) // 8), b.fix)
            if X is None:
                continue
            rrc, rimg = ol.ref_decode(np.frombuffer(X, np.uint8))
            assert (rrc == 0) == (code == dm.OK), (cls, i, rrc, code)
            if code == dm.OK:
                assert np.array_equal(rimg, img), (cls, i)
                n_acc += 1
            else:
                n_rej += 1
    assert n_acc >= 5 and n_rej >= 5, (n_acc, n_rej)


def _peek(bad, avail, fix):
    try:
        return 0, himg_amd.prefix_peek(bad, avail, fix)
    except himg_amd.HimgError as e:
        return e.code, e.plan


@pytest.mark.parametrize("name", NAMES)
def test_prefix_peek_is_the_walk(name):
    b = dm.BASE[name]
    codes = set()
    cases = [(s.bad, a) for cls in "PH" for s, av in zip(dm.streams(name, cls), dm.avails(name, cls)) for a in av]
    cases += [(s.bad, c[0]) for s, (_, cs) in zip(dm.streams(name, "C"), dm.head_cases(name)) for c in cs]
    for bad, a in cases:
        code, plan = _peek(bad, a, b.fix)
        mcode, mplan = pm.walk(bad, a, b.fix)
        if code == himg_amd.HIMG_ERR_UNSUPPORTED:
            # FRMT's fields are read behind a damaged chunk header: a geometry outside the engine's limits,
            # which the walk does not know
            assert (mplan["width"], mplan["height"], mplan["num_channels"]) != (b.W, b.H, b.C)
            continue
        assert code == mcode, (a, code, mcode)
        codes.add(code)
        if code == 0:
            assert {k: plan[k] for k in KEYS} == {k: mplan[k] for k in KEYS}, a
        else:
            for k in ("packed_size", "width", "height", "num_channels", "head_bytes"):
                assert plan[k] == mplan[k], (a, k)
    assert codes == {dm.OK, dm.FORMAT, dm.CAPACITY}


@pytest.mark.parametrize("name", NAMES)
def test_region_peek_rejects_where_the_walk_does(name):
    b = dm.BASE[name]
    n_rej = 0
    for cls in "PH":
        ss = dm.streams(name, cls)
        for i, (x, y, w, h) in dm.region_cases(name, cls):
            r0, r1 = y // 8, (y + h + 7) // 8
            code, ranges, _ = dm.walk_rows(ss[i].bad, r1, None, b.fix)
            try:
                p = himg_amd.region_peek(ss[i].bad, x, y, w, h, b.fix)
            except himg_amd.HimgError as e:
                assert e.code == himg_amd.HIMG_ERR_FORMAT and code == dm.FORMAT, (cls, i, e.code, code)
                n_rej += 1
                continue
            assert code == dm.OK, (cls, i)
            assert (p["row0"], p["row1"]) == (r0, r1) and p["rows_end"] == sum(ranges[r1 - 1]), (cls, i)
    assert n_rej >= 5 or not dm.streams(name, "H")


@pytest.mark.parametrize("name", NAMES)
def test_outcome_floors(name):
    m = dm.good_model(name)
    floor = 20 if m.rows >= 3 else 5
    cnt = dm.outcomes(name)
    print(name, cnt)
    for key in ("damaged", "rejected", "outside"):
        assert cnt[key] >= floor, (key, cnt)
    if dm.streams(name, "H"):
        for key in ("walk", "past", "unseen"):
            assert cnt[key] >= floor, (key, cnt)
    # class C: the cases whose pixels are not judged are at most 20 % (the engine's UNSUPPORTED answers
    # come on top, on the GPU: test_gpu_partial_damage.py counts them against the same limit)
    kinds = [c[1] for _, cs in dm.head_cases(name) for c in cs]
    n_open = kinds.count("open")
    n_k0 = sum(c[1] == "fres" and c[2] == dm.OK for _, cs in dm.head_cases(name) for c in cs)
    print(name, {k: kinds.count(k) for k in sorted(set(kinds))}, "k = 0, pixels not judged:", n_k0)
    assert 5 * (n_open + n_k0) <= len(kinds), (n_open, n_k0, len(kinds))
    for k in ("walk", "model"):
        assert kinds.count(k) >= 20, (k, kinds.count(k))
