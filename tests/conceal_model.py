"""The concealing decode (himg_hip_decode_conceal_*) as its definition in include/himg_hip.h, on top of
damage_model and prefix_model: the walk gives k, each row below k is judged ON ITS OWN by the oracle (the
good stream with that one row's payload as the damaged stream's header chain delimits it), a rejected row
and every row from k on is the low-res fill.  For damage at or after head_bytes.

Test infrastructure only.
"""
import functools

import numpy as np

import damage_model as dm


def expect(model, bad, fix):
    """(picture, rowmap as a uint8 array) of the stream `bad`; model = prefix_model.Model(good)."""
    code, ranges, plan = dm.walk_rows(bad, None, None, fix)
    assert plan["head_bytes"] != 0, "the head must have passed"
    rows = model.rows
    k = rows if code == dm.OK else len(ranges)   # (a failure behind the last row: every row is delimited)
    out, rowmap = model.fill.copy(), np.ones(rows, np.uint8)
    for r in range(k):
        if r + 1 < rows:
            rcode, img, _ = dm.expect_rows(model.packed, bad, range(r, r + 1), fix)
        else:
            # The last row's own verdict: expect_rows would walk on to the end of the chunk, and what fails
            # behind the last row conceals nothing.  The same splice from the ranges of the walk above.
            g, b = dm._bytes(model.packed), dm._bytes(bad)
            pay = [g[o:o + n] for o, n in dm.rows_of(g, fix)[1]]
            pay[r] = b[ranges[r][0]:ranges[r][0] + ranges[r][1]]
            rc, img = dm.judge(dm.resplice(g, pay, fix), fix)
            rcode = dm.OK if rc == 0 else dm.FORMAT
        if rcode == dm.OK:
            out[8 * r:8 * r + 8] = img[8 * r:8 * r + 8]
            rowmap[r] = 0
    return out, rowmap


@functools.lru_cache(maxsize=None)
def corpus(name, cls):
    """[(picture, rowmap)] of damage_model.streams(name, cls), classes P and H."""
    b, m = dm.BASE[name], dm.good_model(name)
    return [expect(m, s.bad, b.fix) for s in dm.streams(name, cls)]
