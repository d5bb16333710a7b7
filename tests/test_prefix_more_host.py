"""Host: the resumed row walk.  tests/prefix_more_model.py's walk_from against the walk from scratch
(prefix_model.walk) from every predecessor state along a chain of row ends, and himg_hip_prefix_peek_from
against that model field for field; the states the rules refuse."""
import functools

import numpy as np
import pytest

import assembled_cases as ac
import golden_util as gu
import himg_amd
import oracle_lib as ol
import prefix_model as pm
import prefix_more_model as mm

KEYS = ("width", "height", "num_channels", "rows", "rows_complete", "packed_size", "head_bytes", "used_bytes",
        "next_bytes")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, the avails to look at).  Every prefix length for the small streams; for the wide one every
    length up to the first row header and within 8 bytes of a row's header or end -- the cuts inside the
    4-byte headers among them --, and every 1009th between."""
    if name == "randtile64":
        m = pm.Model(gu.fixture(gu.GOLDEN["randtile_s0_64x64_q50"]))
        return m, range(m.T + 1)
    if name == "onerow":
        img = himg_amd.synth("randtile", 3, 40, 8)
        m = pm.Model(np.frombuffer(ol.oracle_encode(img, 90, True), np.uint8).copy(), True)
        assert m.rows == 1
        return m, range(m.T + 1)
    m = pm.Model(np.frombuffer(bytes(ac._base(4096, 16, 4, True)["packed"]), np.uint8).copy())
    ends = m.row_ends()
    assert len(ends) == 3 and ends[1] - ends[0] > 0x8000 + 4
    av = set(range(ends[0] + 9)) | set(range(ends[0], m.T + 1, 1009)) | {m.T}
    for e in ends:
        av |= set(range(e - 8, min(e + 9, m.T + 1)))
    return m, sorted(av)


def _chain_states(m):
    """The state behind a call at each row end, reached link by link from a fresh one."""
    st, out = mm.state(), []
    for k, e in enumerate(m.row_ends()):
        code, got_k, written, st = mm.step(m, st, e)
        assert code == 0 and got_k == k and st == mm.state(1, k, e, e), (k, e, st)
        assert written == ((0, m.rows) if k == 0 else (k - 1, k))
        out.append(st)
    return out


CASES = ["randtile64", "onerow", "wide"]


@pytest.mark.parametrize("name", CASES)
def test_model_resumed_walk_is_the_walk_from_scratch(name):
    m, avails = _case(name)
    b = m.packed.tobytes()
    states = _chain_states(m)
    if name == "wide":   # a state may also stand between the two halves of a header: nothing was passed
        states.append(mm.step(m, states[1], m.row_ends()[1] + 2)[3])
        assert states[-1] == mm.state(1, 1, m.row_ends()[1], m.row_ends()[1] + 2)
    for a in avails:
        want = pm.walk(b, a, m.fix_t2)
        assert mm.walk_from(b, mm.FRESH, a, m.fix_t2) == want
        for st in states:
            got = mm.walk_from(b, st, a, m.fix_t2)
            if a < st["avail_seen"]:
                assert got == (mm.ARG, pm.empty_plan()), (a, st)
            else:
                assert got == want, (a, st)


def _peek_from(b, st, a, fix):
    arr = himg_amd.prefix_states(1)
    for k, v in st.items():
        arr[k][0] = v
    before = arr.copy()
    try:
        got = 0, himg_amd.prefix_peek_from(b, arr[0:1], a, fix)
    except himg_amd.HimgError as e:
        got = e.code, e.plan
    assert np.array_equal(arr, before)   # the state is read, never written
    return got


def _same(b, st, a, fix):
    code, plan = _peek_from(b, st, a, fix)
    mcode, mplan = mm.walk_from(b, st, a, fix)
    assert code == mcode, (a, st, code, mcode)
    if code in (0, mm.ARG):
        assert {k: plan[k] for k in KEYS} == {k: mplan[k] for k in KEYS}, (a, st)
    else:   # what the walk had reached
        for k in ("packed_size", "width", "height", "num_channels", "head_bytes"):
            assert plan[k] == mplan[k], (a, st, k)
    return code, plan


@pytest.mark.parametrize("name", CASES)
def test_peek_from_against_the_model(name):
    m, avails = _case(name)
    b = m.packed
    states = _chain_states(m)
    for a in avails:
        piece = b[:a].copy()   # exactly the bytes present: nothing behind them exists
        # a fresh state: himg_hip_prefix_peek
        fresh = _same(piece, mm.FRESH, a, m.fix_t2)
        try:
            plain = 0, himg_amd.prefix_peek(piece, a, m.fix_t2)
        except himg_amd.HimgError as e:
            plain = e.code, e.plan
        assert fresh == plain, a
        for st in states:
            _same(piece, st, a, m.fix_t2)


def test_mixed_batch_verdicts():
    """prefix_more_model.mixed_batch -- the six frames test_gpu_prefix_more sends through one launch -- gives its
    six intended verdicts, by the model and by himg_hip_prefix_peek_from."""
    img = np.ascontiguousarray(himg_amd.synth("randtile", 0, 72, 40)[:, :, :3])
    m = pm.Model(np.frombuffer(ol.oracle_encode(img, 50, True), np.uint8).copy())
    cases = mm.mixed_batch(m)
    assert [c[2] for c in cases] == [0, 0, 0, himg_amd.HIMG_ERR_CAPACITY, himg_amd.HIMG_ERR_ARG, 0]
    got = [mm.step(m, st, a) for st, a, _ in cases]
    assert [g[0] for g in got] == [c[2] for c in cases]
    assert [g[1] for g in got] == [1, 3, 2, -1, -1, 5]
    assert [g[2] for g in got] == [(0, 5), (1, 3), None, None, None, (0, 5)]
    for (st, a, code), g in zip(cases, got):
        assert _same(m.packed[:a].copy(), st, a, False)[0] == code, (st, a)
        assert g[3] == (dict(st) if code else mm.state(1, g[1], m.row_ends()[g[1]], a))


def test_impossible_states():
    m, _ = _case("randtile64")
    b, e = m.packed, m.row_ends()
    head, end = e[0], m.T   # (FRES is the last chunk: it ends with the stream)
    good = mm.state(1, 2, e[2], e[2])
    assert _same(b, good, e[5], False)[0] == 0
    for what, st, a in [("avail below avail_seen", good, e[2] - 1),
                        ("rows_done < 0", mm.state(1, -1, e[2], e[2]), e[5]),
                        ("rows_done > rows", mm.state(1, m.rows + 1, e[2], e[2]), e[5]),
                        ("walk_pos below the first header", mm.state(1, 0, head - 1, head - 1), e[5]),
                        ("walk_pos beyond the chunk", mm.state(1, 8, end + 1, e[2]), m.T),
                        ("walk_pos beyond avail", mm.state(1, 3, e[3], e[1]), e[2])]:
        code, plan = _same(b[:a].copy(), st, a, False)
        assert code == himg_amd.HIMG_ERR_ARG, what
        assert all(plan[k] == 0 for k in KEYS), what
    # a NULL state or plan
    import ctypes as C
    plan = himg_amd.PrefixPlan()
    L = himg_amd.lib()
    assert L.himg_hip_prefix_peek_from(b.ctypes.data, b.nbytes, 0, None, C.byref(plan)) == himg_amd.HIMG_ERR_ARG
    st = himg_amd.PrefixState()
    assert L.himg_hip_prefix_peek_from(b.ctypes.data, b.nbytes, 0, C.addressof(st), None) == himg_amd.HIMG_ERR_ARG
    # the ctypes structure and the numpy layout are the C struct's 16 bytes
    assert C.sizeof(himg_amd.PrefixState) == 16 and himg_amd.prefix_states(3).nbytes == 48
    assert himg_amd.prefix_states(1).dtype.names == ("started", "rows_done", "walk_pos", "avail_seen")
