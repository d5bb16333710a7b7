"""Host: himg_hip_prefix_peek against the model's plain Python walk (tests/prefix_model.py) at every
prefix length of the small goldens and on a stream with 4-byte row headers; its error codes; and the
model's definition of the rows that have not arrived, pinned against the oracle decoder itself on
streams whose rows from k on are all zero."""
import numpy as np
import pytest

import assembled_cases as ac
import golden_util as gu
import himg_amd
import oracle_lib as ol
import prefix_model as pm
import stream_assembler as sa

KEYS = ("width", "height", "num_channels", "rows", "rows_complete", "packed_size", "head_bytes", "used_bytes",
        "next_bytes")


def _peek(b, avail, fix_t2=False):
    try:
        return 0, himg_amd.prefix_peek(b, avail, fix_t2)
    except himg_amd.HimgError as e:
        return e.code, e.plan


def _same(b, avail, fix_t2=False):
    code, plan = _peek(b, avail, fix_t2)
    mcode, mplan = pm.walk(b, avail, fix_t2)
    assert code == mcode, (avail, code, mcode)
    if code == 0:
        assert {k: plan[k] for k in KEYS} == {k: mplan[k] for k in KEYS}, avail
    else:   # what the walk had reached
        for k in ("packed_size", "width", "height", "num_channels", "head_bytes"):
            assert plan[k] == mplan[k], (avail, k)
    return code, plan


@pytest.mark.parametrize("name", [n for n in gu.cases(max_pixels=64 * 64) if "fixture" in gu.GOLDEN[n]])
def test_peek_every_prefix_length(name):
    b = gu.fixture(gu.GOLDEN[name])
    for fix in (False, True):
        ks = []
        for avail in range(b.size + 1):
            # (a slice of exactly avail bytes: nothing behind it exists)
            code, plan = _same(b[:avail].copy(), avail, fix)
            if code == 0:
                ks.append(plan["rows_complete"])
                assert plan["used_bytes"] <= avail < plan["next_bytes"] or plan["rows_complete"] == plan["rows"]
        full_code, full = _peek(b, b.size, fix)
        if full_code == 0:   # (the grad stream: trap T2 without the fix)
            assert ks == sorted(ks) and ks[0] == 0 and ks[-1] == 8
            assert full["next_bytes"] == b.size and full["used_bytes"] == b.size


def _wide():
    """4096 x 16 rand q100: both rows' payloads take a 4-byte size header."""
    b = ac._base(4096, 16, 4, True)["packed"]
    return np.frombuffer(bytes(b), np.uint8).copy()


def test_peek_four_byte_headers():
    b = _wide()
    m = pm.Model(b)
    ends = m.row_ends()
    assert len(ends) == 3 and ends[1] - ends[0] > 0x8000 + 4
    for k in (0, 1):
        h = ends[k]   # the header of row k starts here: cut after 0, 1, 2 and 3 of its 4 bytes
        for cut, nxt in ((0, h + 2), (1, h + 2), (2, h + 4), (3, h + 4)):
            code, plan = _same(b, h + cut)
            assert code == 0 and plan["rows_complete"] == k and plan["next_bytes"] == nxt and plan["used_bytes"] == h
        code, plan = _same(b, h + 4)
        assert code == 0 and plan["rows_complete"] == k and plan["next_bytes"] == ends[k + 1]
        _same(b, ends[k + 1] - 1)
    code, plan = _same(b, b.size)
    assert plan["rows_complete"] == 2 and plan["next_bytes"] == b.size


def test_peek_error_codes():
    b = gu.fixture(gu.GOLDEN["randtile_s0_64x64_q50"])
    T = b.size
    head = himg_amd.region_peek(b, 0, 0, 64, 64)["head_bytes"]
    # below the first row header: HIMG_ERR_CAPACITY; head_bytes only once the tree's length is known
    for avail in (0, 11, 12, 40, head - 1):
        code, plan = _same(b, avail)
        assert code == himg_amd.HIMG_ERR_CAPACITY, avail
    assert _peek(b, 11)[1]["packed_size"] == 0 and _peek(b, 12)[1]["packed_size"] == T
    assert _peek(b, head - 1)[1]["width"] == 64
    code, plan = _same(b, head)
    assert code == 0 and plan["rows_complete"] == 0 and plan["head_bytes"] == head == plan["used_bytes"]
    # more bytes than the RIFF header declares
    longer = np.concatenate((b, np.zeros(4, np.uint8)))
    assert _same(longer, T + 1)[0] == himg_amd.HIMG_ERR_FORMAT
    # damage that is present: the magic, a chunk size beyond T, a row header beyond the chunk
    for off, val in ((0, 0x51), (8, 0x51), (19, 0x7f)):
        d = b.copy()
        d[off] = val
        assert _same(d, T)[0] == himg_amd.HIMG_ERR_FORMAT, off
        assert _same(d, 64)[0] == himg_amd.HIMG_ERR_FORMAT, off
    d = b.copy()
    d[head + 1] = 0x7f      # row 0's length: far beyond the chunk's end
    assert _same(d, head + 1)[0] == 0 and _same(d, head + 2)[0] == himg_amd.HIMG_ERR_FORMAT
    # the same damage behind the bytes present is not seen
    assert _same(d, head)[0] == 0
    # trap T2 is the decoder's: the grad golden fails without the fix, passes with it
    g = gu.fixture(gu.GOLDEN["grad_s0_64x64_q50"])
    assert _same(g, g.size, False)[0] == himg_amd.HIMG_ERR_FORMAT
    assert _same(g, g.size, True)[0] == 0
    # an unsupported geometry is reported as himg_hip_peek reports it, as soon as FRMT is there
    d = b.copy()
    d[21:25] = (0xff, 0xff, 0xff, 0x7f)
    assert _peek(d, T)[0] == himg_amd.HIMG_ERR_UNSUPPORTED
    # FRMT's fields are untrusted: a channel count of 0 is an unsupported geometry, as for himg_hip_peek
    # (the walk itself goes on past FRMT and would pass)
    d = b.copy()
    assert d[29] == 4
    d[29] = 0
    import ctypes as C
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    assert himg_amd.lib().himg_hip_peek(d.ctypes.data, T, C.byref(w), C.byref(h), C.byref(c)) == himg_amd.HIMG_ERR_UNSUPPORTED
    for avail in (T, head, 64):
        assert _peek(d, avail)[0] == himg_amd.HIMG_ERR_UNSUPPORTED, avail
    assert _peek(d, 24)[0] == himg_amd.HIMG_ERR_CAPACITY    # FRMT's fields have not arrived
    # arguments
    assert himg_amd.lib().himg_hip_prefix_peek(None, 4, 0, None) == himg_amd.HIMG_ERR_ARG
    for avail in (-1, T + 1):   # not a length of this buffer
        with pytest.raises(ValueError):
            himg_amd.prefix_peek(b, avail)


@pytest.mark.parametrize("W,H,C,ycc,k", [(64, 64, 4, True, 3), (100, 45, 3, True, 0), (37, 19, 1, False, 2)])
def test_model_fill_is_the_decoders(W, H, C, ycc, k):
    """Rows >= k all zero, in a stream with the same head: the oracle decodes them to the model's fill."""
    base = ac._base(W, H, C, ycc)
    rows, n = (H + 7) // 8, ((W + 7) // 8) * 64 * C
    tree = sa.balanced(range(261))   # holds every literal and every run symbol
    fres = [sa.encoder_tokens(r if v < k else np.zeros(n, np.uint8)) for v, r in enumerate(base["fres_rows"])]
    parts = {p: base[p] for p in ("lmap", "lres_tree", "lres_tokens", "shift_luma", "shift_chroma", "fmap")}
    zs = sa.assemble(W, H, C, ycc, fres_tree=tree, fres_row_tokens=fres, **parts)
    rc, got = ol.oracle_decode(zs, fix_t2=True)
    assert rc == 0
    m = pm.Model(np.frombuffer(bytes(base["packed"]), np.uint8), fix_t2=True)
    assert rows == m.rows
    assert np.array_equal(got[8 * k:], m.fill[8 * k:])
    assert np.array_equal(got[:8 * k], m.full[:8 * k])
    assert np.array_equal(got, m.picture(k))
    if k == 0:   # the low-res plane as a picture is not flat
        assert m.fill.std() > 1
