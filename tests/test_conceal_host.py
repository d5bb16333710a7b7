"""Host: the concealing decode's interface and the premises of tests/conceal_model.py, proved with the oracle
alone on every base of damage_model, and the floors that keep tests/test_gpu_conceal.py from being vacuous.

1. The two entry points are exported by the library and declared in include/himg_hip.h; the Python entry
   points exist.
2. Premises: a stream the oracle accepts conceals nothing and the model's picture is the oracle's; a class-P
   stream the oracle rejects conceals at least one row; every unconcealed row of a class-P stream is the good
   stream's row or the single-row decode of test_damage_model_host.py's test_row_independence, and only a
   damaged row is ever concealed.
3. Floors, counted by the model alone (minimum over the bases, the base that has it, the floor asserted):

       quantity                                          | scope                 | min | base             | floor
       frames with a concealed row                       | class P               |  44 | rand4096x24q100  |  40
       partly concealed frames                           | P, bases of >= 2 rows |  44 | rand4096x24q100  |  40
       accepted rows with other pixels than the good one | class P               |  23 | grad40x40q0      |  20
       header walks that stop short                      | class H               |  85 | rand4096x24q100  |  80

   randtile40x8 has one row: 78 of its 120 class-P frames are concealed whole, and it has no class H.
4. Class C: the streams the oracle rejects in the FRES stage, whose pixels test_gpu_conceal.py does not
   judge, are at most 20 % of the class.
"""
import os
import re

import numpy as np
import pytest

import conceal_model as cm
import damage_model as dm
import himg_amd
import oracle_lib as ol

NAMES = [b.name for b in dm.BASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_declared():
    lib = himg_amd.lib()
    header = open(os.path.join(ROOT, "include", "himg_hip.h")).read()
    for name in ("himg_hip_decode_conceal_device", "himg_hip_decode_conceal_to"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
        assert re.search(r"\bint %s\(himg_hip_ctx \*ctx," % name, header), name
    assert len(lib.himg_hip_decode_conceal_device.argtypes) == 13
    assert len(lib.himg_hip_decode_conceal_to.argtypes) == 11


def test_python_entry_points():
    assert callable(getattr(himg_amd.Engine, "decode_conceal", None))
    assert callable(getattr(himg_amd.Engine, "decode_conceal_device", None))


@pytest.mark.parametrize("name", NAMES)
def test_good_stream_conceals_nothing(name):
    b, m = dm.BASE[name], dm.good_model(name)
    pic, rowmap = cm.expect(m, m.packed, b.fix)
    assert not rowmap.any() and np.array_equal(pic, m.full)


@pytest.mark.parametrize("name", NAMES)
def test_premises_class_p(name):
    b, m = dm.BASE[name], dm.good_model(name)
    g = m.packed.tobytes()
    good_rows = [g[o:o + n] for o, n in dm.rows_of(g, b.fix)[1]]
    n_acc = n_rej = 0
    for s, (pic, rowmap) in zip(dm.streams(name, "P"), cm.corpus(name, "P")):
        rc, img = dm.judge(s.bad.tobytes(), b.fix)
        if rc == 0:   # the oracle accepts: nothing concealed, the oracle's picture
            assert not rowmap.any() and np.array_equal(pic, img), s.rows
            n_acc += 1
        else:
            assert rowmap.any(), s.rows
            n_rej += 1
        bad = s.bad.tobytes()
        bad_rows = [bad[o:o + n] for o, n in dm.rows_of(bad, b.fix)[1]]   # (payload damage moves no header)
        for r in range(m.rows):
            rows = slice(8 * r, 8 * r + 8)
            if r not in s.rows:
                assert not rowmap[r] and np.array_equal(pic[rows], m.full[rows]), (s.rows, r)
            elif rowmap[r]:
                assert np.array_equal(pic[rows], m.fill[rows]), (s.rows, r)
            else:
                one = dm.resplice(g, [bad_rows[i] if i == r else good_rows[i] for i in range(m.rows)], b.fix)
                rc1, img1 = dm.judge(one, b.fix)
                assert rc1 == 0 and np.array_equal(pic[rows], img1[rows]), (s.rows, r)
    assert n_acc >= 5 and n_rej >= 5, (n_acc, n_rej)


@pytest.mark.parametrize("name", NAMES)
def test_floors(name):
    b, m = dm.BASE[name], dm.good_model(name)
    P = cm.corpus(name, "P")
    n_any = sum(bool(rowmap.any()) for _, rowmap in P)
    n_part = sum(0 < int(rowmap.sum()) < m.rows for _, rowmap in P)
    n_other = sum(1 for pic, rowmap in P for r in range(m.rows)
                  if not rowmap[r] and not np.array_equal(pic[8 * r:8 * r + 8], m.full[8 * r:8 * r + 8]))
    n_short = 0
    for s in dm.streams(name, "H"):
        code, ranges, _ = dm.walk_rows(s.bad, None, None, b.fix)
        n_short += code != dm.OK and len(ranges) < m.rows
    print("%-16s | rows %d | P: concealed %3d  partly %3d  accepted with other pixels %3d | H: walks that stop short %3d"
          % (name, m.rows, n_any, n_part, n_other, n_short))
    assert n_any >= 40, n_any
    assert n_other >= 20, n_other
    if m.rows >= 2:
        assert n_part >= 40, n_part
    if dm.streams(name, "H"):
        assert n_short >= 80, n_short
    # the H corpus conceals, too: every frame whose walk stops short has a concealed row
    for (pic, rowmap), s in zip(cm.corpus(name, "H"), dm.streams(name, "H")):
        code, ranges, _ = dm.walk_rows(s.bad, None, None, b.fix)
        if code != dm.OK and len(ranges) < m.rows:
            assert rowmap[len(ranges):].all()


@pytest.mark.parametrize("name", NAMES)
def test_class_c_unjudged_share(name):
    b = dm.BASE[name]
    rcs = [ol.oracle_decode(s.bad, fix_t2=b.fix)[0] for s in dm.streams(name, "C")]
    n_fres = sum(rc not in (0, -1, -2, -3, -4, -5, -6) for rc in rcs)
    print(name, "class C: accepted %d, head %d, FRES stage (not judged) %d" % (rcs.count(0), len(rcs) - rcs.count(0) - n_fres, n_fres))
    assert 5 * n_fres <= len(rcs), (n_fres, len(rcs))
    assert rcs.count(0) >= 20 and len(rcs) - rcs.count(0) - n_fres >= 5
