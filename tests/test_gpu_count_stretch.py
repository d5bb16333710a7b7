"""GPU (-m gpu): the wavefront-per-row count kernel with a STRETCH of consecutive sub-sequences per lane
(HIMG_OPT_COUNT_STRETCH = 2, 4, 8) against its form of one sub-sequence per lane (= 1).

First the records themselves, word for word, through himg_hip_debug_row_records -- which runs the front of
the decode up to the count kernel and NO row kernel: the records drive unguarded LDS writes there, so a new
form is compared here before anything consumes what it writes.  The records are a function of the stream
alone; only the header's `rounds` word (a diagnostic: how often the chain inside a phase was revisited)
depends on the form.  Then pixels and per-frame status of whole decodes against the CPU oracle, every
form, and the same on damaged streams (test_gpu_fuzz's mutations).

Shapes: 4096 x 16 (two full-width rows, sub-sequences of about 270 bits), 4096 x 8 at q90 beside a q50
frame in one launch (sub-sequences beyond 320 bits keep the form of a sub-sequence per lane, chosen per
row), 64 x 512 (128-bit sub-sequences, most lanes and phases beyond the payload), 1024 x 24 and 520 x 24
(the last active sub-sequence inside a stretch), 8 x 8.  Contents: random tiles, noise, a flat colour with
opaque alpha (periodic run tokens that do not self-synchronise: the long re-walk), a gradient.  Everything
runs under HIMG_OPT_FIX_T2, on the engine and in the oracle: the reference rejects flat frames and frames
of at most 8 pixel rows that its own encoder wrote, and streams it accepts decode identically either way."""
import functools
import os

import numpy as np
import pytest
import torch

import himg_amd
import oracle_lib as ol
from test_gpu_fuzz import _chunks, _mutate

pytestmark = pytest.mark.gpu

LANES, HDR = 1024, 72
H_TOTAL, H_END, H_FLAG, H_ROUNDS, H_PER_LANE = LANES, LANES + 1, LANES + 2, LANES + 3, LANES + 4
FORMS = (2, 4, 8)
# (width, height, [(content, quality)])
SHAPES = [
    (4096, 16, [("randtile", 50), ("rand", 50), ("flat", 50), ("grad", 50)]),
    (4096, 8, [("randtile", 90), ("randtile", 50), ("flat", 50), ("grad", 90)]),
    (64, 512, [("randtile", 50), ("rand", 50), ("flat", 50), ("grad", 50)]),
    (1024, 24, [("randtile", 50), ("rand", 50), ("flat", 50), ("grad", 50)]),
    (520, 24, [("randtile", 50), ("rand", 50), ("flat", 50), ("grad", 50)]),
    (8, 8, [("randtile", 50), ("rand", 50), ("flat", 50), ("grad", 50)]),
]
IDS = ["%dx%d" % (w, h) for w, h, _ in SHAPES]


@pytest.fixture(scope="module")
def eng():
    """An engine of its own, created with the wavefront-per-row count kernel forced by the environment."""
    old = os.environ.get("HIMG_COUNT_WAVE")
    os.environ["HIMG_COUNT_WAVE"] = "1"
    try:
        e = himg_amd.Engine(0)
    finally:
        if old is None:
            del os.environ["HIMG_COUNT_WAVE"]
        else:
            os.environ["HIMG_COUNT_WAVE"] = old
    assert e.get_option("count_wave") == 1
    e.set_option("fix_t2", 1)
    yield e
    e.close()


def _picture(kind, w, h):
    if kind == "flat":
        a = np.empty((h, w, 4), np.uint8)
        a[:] = (37, 150, 201, 255)
        return a
    return himg_amd.synth(kind, 11, w, h)


@functools.lru_cache(maxsize=None)
def _good(w, h):
    """The streams of a shape and the oracle's pixels for them (computed once, never written to)."""
    _, _, contents = next(s for s in SHAPES if s[:2] == (w, h))
    streams = [ol.oracle_encode(_picture(k, w, h), q, True) for k, q in contents]
    want = []
    for s in streams:
        rc, px = ol.oracle_decode(s, fix_t2=True)
        assert rc == 0
        want.append(px.reshape(h, w, 4))
    return streams, want


def _upload(streams):
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.zeros((len(streams), stride), np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = s
    return torch.from_numpy(buf).cuda(), stride, np.array([len(s) for s in streams], np.uint32)


def _sub_bits(stream):
    """The row kernels' sub-sequence length of every block row of a stream (bits)."""
    ln = np.asarray(himg_amd.index_host(stream, fix_t2=True)[4], np.int64)
    sb = (8 * ln + LANES - 1) // LANES
    return np.maximum((sb + 31) // 32 * 32, 128)


def _records(e, d_in, stride, sizes, w, h, form):
    """(lane_start [n][rows][1024], lane_off [n][rows][1024 + 72], status [n]) of one form; no row kernel runs."""
    n, rows = len(sizes), (h + 7) // 8
    e.set_option("count_stretch", form)
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    e.row_records_device(d_in, stride, sizes, n, w, h, 4, d_st)
    torch.cuda.synchronize()
    ls = [e.debug_read("lane_start", f, rows * LANES * 4, np.uint32, decoder=True).reshape(rows, LANES).copy() for f in range(n)]
    lo = [e.debug_read("lane_off", f, rows * (LANES + HDR) * 4, np.uint32, decoder=True).reshape(rows, LANES + HDR).copy()
          for f in range(n)]
    return np.stack(ls), np.stack(lo), d_st.cpu().numpy()


def _same_records(old, new, what):
    """Every word a consumer reads: the flag of every row; of a usable row the 1024 starts, the 1024 offsets,
    total, end of the chain and records per lane."""
    (ls0, lo0, st0), (ls1, lo1, st1) = old, new
    assert np.array_equal(st0, st1), (what, st0, st1)
    assert np.array_equal(lo0[..., H_FLAG], lo1[..., H_FLAG]), (what, "flags")
    ok = lo0[..., H_FLAG] == 3
    assert not (lo0[..., H_FLAG][~ok]).any(), (what, "a flag that is neither 0 nor 3")
    for f, r in zip(*np.nonzero(ok)):
        a = np.flatnonzero(ls0[f, r] != ls1[f, r])
        assert a.size == 0, (what, "lane_start", f, r, a[:8], ls0[f, r, a[:8]], ls1[f, r, a[:8]])
        a = np.flatnonzero(lo0[f, r, :LANES] != lo1[f, r, :LANES])
        assert a.size == 0, (what, "lane_off", f, r, a[:8], lo0[f, r, a[:8]], lo1[f, r, a[:8]])
        for k in (H_TOTAL, H_END, H_PER_LANE):
            assert lo0[f, r, k] == lo1[f, r, k], (what, "header word", k - LANES, f, r, lo0[f, r, k], lo1[f, r, k])
    return ok


@pytest.mark.parametrize("w,h", [s[:2] for s in SHAPES], ids=IDS)
def test_records_word_for_word(eng, w, h):
    streams, _ = _good(w, h)
    d_in, stride, sizes = _upload(streams)
    old = _records(eng, d_in, stride, sizes, w, h, 1)
    assert not old[2].any(), old[2]
    usable = old[1][..., H_FLAG] == 3
    sb = np.stack([_sub_bits(s) for s in streams])
    # The premises of the shapes: every row of these small frames has a record; which rows take which form.
    assert usable.all(), np.argwhere(~usable)[:8]
    if (w, h) == (4096, 16):
        assert ((sb[0] > 192) & (sb[0] <= 320)).all(), sb[0]
    if (w, h) == (4096, 8):
        assert (sb[0] > 320).all() and (sb[1] <= 320).all(), (sb[0], sb[1])    # q90 beyond the staged reader, q50 inside
    if (w, h) == (64, 512):
        assert (sb[0] == 128).all()
    for form in FORMS:
        new = _records(eng, d_in, stride, sizes, w, h, form)
        _same_records(old, new, (w, h, form))
    eng.set_option("count_stretch", -1)


def _damaged(w, h):
    """Seeded hostile streams of a shape's random-tile frame with the oracle's verdict and pixels."""
    good = _good(w, h)[0][0]
    ch = _chunks(good)
    rng = np.random.default_rng(4242 + w)
    pool, want = [], []
    for t in range(64):
        bad = _mutate(good, ch, rng, 4 * t if t % 2 else t)    # every other one a flip in the FRES payload
        rc, px = ol.oracle_decode(bad, fix_t2=True)
        pool.append(bad)
        want.append(px.reshape(h, w, 4) if rc == 0 else None)
    return pool, want


_damaged = functools.lru_cache(maxsize=None)(_damaged)


@pytest.mark.parametrize("w,h", [(4096, 16), (1024, 24)], ids=["4096x16", "1024x24"])
def test_records_of_damaged_streams_word_for_word(eng, w, h):
    pool, _ = _damaged(w, h)
    d_in, stride, sizes = _upload(pool)
    old = _records(eng, d_in, stride, sizes, w, h, 1)
    n_rows = 0
    for form in FORMS:
        n_rows = int(_same_records(old, _records(eng, d_in, stride, sizes, w, h, form), (w, h, form, "damaged")).sum())
    assert n_rows >= 16    # (frames whose parse or row walk fails have no records: most of them have)
    eng.set_option("count_stretch", -1)


def _decode(e, d_in, stride, sizes, w, h, form):
    n = len(sizes)
    e.set_option("count_stretch", form)
    d_pix = torch.full((n, h, w, 4), 0xA5, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    e.decode_device(d_in, stride, sizes, n, w, h, 4, d_pix, d_st, 0)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_pix.cpu().numpy()


@pytest.mark.parametrize("w,h", [s[:2] for s in SHAPES], ids=IDS)
def test_pixels_and_status_match_oracle(eng, w, h):
    streams, want = _good(w, h)
    d_in, stride, sizes = _upload(streams)
    for form in (1,) + FORMS:
        st, pix = _decode(eng, d_in, stride, sizes, w, h, form)
        assert not st.any(), (w, h, form, st)
        for f in range(len(streams)):
            assert np.array_equal(pix[f], want[f]), (w, h, form, f)
    eng.set_option("count_stretch", -1)


@pytest.mark.parametrize("w,h", [(4096, 16), (1024, 24)], ids=["4096x16", "1024x24"])
def test_damaged_streams_match_oracle(eng, w, h):
    pool, want = _damaged(w, h)
    okv = np.array([x is not None for x in want])
    assert okv.sum() >= 8 and (~okv).sum() >= 8, okv    # the mutations reach both outcomes
    d_in, stride, sizes = _upload(pool)
    for form in (1,) + FORMS:
        st, pix = _decode(eng, d_in, stride, sizes, w, h, form)
        wrong = np.flatnonzero((st == 0) != okv)
        assert wrong.size == 0, (w, h, form, "verdicts", wrong[:8], st[wrong[:8]])
        for f in np.flatnonzero(okv):
            assert np.array_equal(pix[f], want[f]), (w, h, form, f)
    eng.set_option("count_stretch", -1)


def test_option_values(eng):
    assert eng.get_option("count_stretch") == -1
    for v in (1, 2, 4, 8, -1):
        eng.set_option("count_stretch", v)
        assert eng.get_option("count_stretch") == v
    for v in (0, 3, 16, 32):
        with pytest.raises(himg_amd.HimgError):
            eng.set_option("count_stretch", v)
    assert eng.get_option("count_stretch") == -1
