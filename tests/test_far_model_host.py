"""No GPU: tests/far_model.py -- the batch-size and memory arithmetic of the far-address tests, and
their whole-buffer comparisons on CPU tensors with the chunk size and the modulus scaled down.  The
comparisons must flag a wrong byte in a window, a non-sentinel byte in a gap, a changed byte in the tail
and a window written at its offset modulo the wrap, and name the place."""
import re

import numpy as np
import pytest
import torch

import conceal_model as cm
import damage_model as dm
import far_model as fm
import himg_amd
import oracle_lib as ol
import prefix_model as pm

GIB = 1 << 30


# ---- arithmetic -----------------------------------------------------------------------------------

def test_dense_batch_sizes():
    S = fm.DENSE
    assert fm.dense_batch(S * S * 4) == 258           # RGBA bytes
    assert fm.dense_batch(S * S * 12) == 88           # three float32 planes
    assert fm.dense_batch(2040 * 2041 * 4) == 260     # the region windows
    assert fm.dense_batch(2040 * 2041 * 12) == 88
    for fb in (1, 7, 4096, S * S * 4, S * S * 12, 2040 * 2041 * 4, (1 << 32) - 1, 1 << 32, (1 << 32) + 1):
        n = fm.dense_batch(fb)
        assert n * fb >= fm.WRAP + 2 * fb and (n - 1) * fb < fm.WRAP + 2 * fb, fb
        starts = [f * fb for f in (n - 2, n - 1)]
        assert all(s >= fm.WRAP for s in starts) and (n - 3) * fb < fm.WRAP, fb   # exactly two whole frames beyond
    assert fm.dense_batch(100, wrap=1000) == 12


def test_far_constants_reach_the_boundary():
    offs = [f * fm.FAR_STRIDE for f in range(fm.FAR_BATCH)]
    beyond, signed = fm.assert_far(offs)
    assert beyond == [4 * fm.FAR_STRIDE] and signed == [2 * fm.FAR_STRIDE, 3 * fm.FAR_STRIDE]
    assert fm.FAR_STRIDE % 256 == 0 and fm.FAR_PITCH % 4 == 0 and fm.FAR_PITCH % 16 != 0 and (fm.FAR_PITCH + 1) % 2 == 1
    assert 63 * fm.FAR_ROW_PITCH < fm.WRAP <= 64 * fm.FAR_ROW_PITCH and 32 * fm.FAR_ROW_PITCH >= fm.WRAP // 2
    assert fm.FAR_ROW_PITCH % 4 == 0 and (fm.FAR_ROW_PITCH + 1) % 2 == 1


def test_assert_far_refuses_near_offsets():
    with pytest.raises(AssertionError, match="reach"):
        fm.assert_far([0, 1 << 31, (1 << 32) - 1])
    with pytest.raises(AssertionError, match="no offset in"):
        fm.assert_far([0, 1 << 30, 1 << 32])
    with pytest.raises(AssertionError, match="only 1 of"):
        fm.assert_far([0, 1 << 31, 1 << 32], whole_beyond=2)
    assert fm.assert_far([10, 600, 1000, 1100], wrap=1000) == ([1000, 1100], [600])


def test_extent_is_the_librarys():
    """far_model.extent against himg_hip_dst_extent and himg_hip_windows_extent (host functions), far
    pitches included."""
    for ps, rp, fp, org, w, h in [(4, 400, 40000, [(0, 0), (5, 3), (24, 16)], 72, 40),
                                  (4, 96 * 4 + 12, fm.FAR_PITCH, [(0, 0), (5, 3), (4, 8), (24, 16), (24, 16)], 72, 40),
                                  (3, 288 * 3 + 5, fm.FAR_PITCH + 1, [(1, 1), (247, 39), (7, 3), (1, 1), (248, 39)], 40, 17),
                                  (4, fm.FAR_ROW_PITCH, 0, [(3, 50), (100, 60), (192, 64)], 72, 8),
                                  (3, fm.FAR_ROW_PITCH + 1, 0, [(1, 51), (224, 61), (7, 65)], 40, 7)]:
        Wd = max(x + w for x, _ in org)
        Hd = max(y + h for _, y in org)
        want = fm.extent(fp, rp, ps, org, w, h)
        assert himg_amd.dst_extent(himg_amd.dst_desc(Wd, Hd, ps, rp, fp), ps, org, w, h) == want
        assert himg_amd.windows_extent(himg_amd.src_desc(Wd, Hd, ps, rp, fp), ps, org, w, h) == want
    assert fm.extent(fm.FAR_PITCH, 396, 4, [(0, 0)] * 5, 72, 40) > fm.WRAP


def test_encoder_clears():
    """include/himg_hip.h, himg_hip_encode_device: 620 + C * (rows * cols + ceil(rows / 16) * ceil(cols / 16)),
    rounded up to 4."""
    assert fm.encoder_clears(72, 8, 4) == 620 + 4 * (9 + 1) and fm.encoder_clears(72, 8, 3) == 652
    assert fm.encoder_clears(72, 40, 4) == 620 + 4 * (45 + 1) and fm.encoder_clears(512, 64, 4) == 620 + 4 * (512 + 4)
    assert fm.encoder_clears(2048, 2048, 4) == 620 + 4 * (256 * 256 + 16 * 16)
    for w, h, c in [(72, 8, 4), (72, 40, 4), (512, 64, 4), (2048, 2048, 4), (9, 9, 1)]:
        assert fm.encoder_clears(w, h, c) <= himg_amd.max_packed_size(w, h, c)


def test_memory_needs():
    assert fm.need([10, 20], 5, chunk=100) == 335
    far = (fm.FAR_BATCH - 1) * fm.FAR_STRIDE + (1 << 20)
    assert fm.need_far(far) == far + fm.WORKSPACE_FAR + 3 * GIB
    S, stride = fm.DENSE, 4307456
    n = fm.need_dense_decode(258, stride, 258 * S * S * 4, 3 * S * S * 4)
    assert n == (258 + 3) * stride + (258 + 3) * S * S * 4 + fm.TAIL + fm.WORKSPACE_DENSE_DECODE + fm.WORKSPACE_DENSE_ENCODE + 3 * GIB
    assert 8 * GIB < n < 64 * GIB
    e = fm.need_dense_encode(258, S * S * 4, 17042688)
    assert e == (258 + 3) * S * S * 4 + 258 * 17042688 + fm.TAIL + fm.WORKSPACE_DENSE_DECODE + fm.WORKSPACE_DENSE_ENCODE + 3 * GIB


# ---- the chunked whole-buffer comparison ------------------------------------------------------------

WRAP, CHUNK = 1 << 16, 4096
PITCH = (1 << 14) + 260          # frame 4 starts beyond WRAP, frames 2 and 3 beyond WRAP / 2
WIN_BYTES = 1000                 # (windows that cross chunk boundaries: 1000 bytes from 3 * PITCH + 77 on)


def _windows(seed=1):
    rng = np.random.default_rng(seed)
    return [(f * PITCH + 77, rng.integers(0, 256, WIN_BYTES, dtype=np.uint8)) for f in range(5)]


def _buffer(windows, at=lambda off: off):
    n = max(off + w.size for off, w in windows)
    buf = np.full(n + fm.TAIL, fm.SENTINEL, np.uint8)
    for off, w in windows:
        buf[at(off):at(off) + w.size] = w
    return buf


def _check(buf, windows, chunk=CHUNK):
    fm.check_buffer(torch.from_numpy(buf), [(off, torch.from_numpy(w)) for off, w in windows], "case", pitch=PITCH,
                    chunk=chunk, wrap=WRAP)


def test_check_buffer_accepts_the_expectation():
    win = _windows()
    fm.assert_far([off for off, _ in win], wrap=WRAP)
    for chunk in (CHUNK, 1000, 1 << 20, 1):
        if chunk == 1:
            small = [(5, np.arange(7, dtype=np.uint8)), (40, np.arange(3, dtype=np.uint8))]
            fm.check_buffer(torch.from_numpy(_buffer(small)), [(o, torch.from_numpy(w)) for o, w in small], "tiny", chunk=1)
        else:
            _check(_buffer(win), win, chunk)
    # no windows at all: the whole buffer is the sentinel
    fm.check_buffer(torch.full((5000,), fm.SENTINEL, dtype=torch.uint8), [], "empty", chunk=CHUNK)


def test_check_buffer_flags_a_wrong_byte_in_a_window():
    win = _windows()
    for f, i in [(0, 0), (3, 999), (4, 500)]:
        buf = _buffer(win)
        off = win[f][0] + i
        buf[off] ^= 0x40
        with pytest.raises(AssertionError) as e:
            _check(buf, win)
        msg = str(e.value)
        assert "1 of %d bytes differ" % buf.size in msg
        assert "byte %d (= %d mod %d) in frame %d" % (off, off % WRAP, WRAP, f) in msg and "a window's byte" in msg


def test_check_buffer_flags_a_byte_in_a_gap():
    win = _windows()
    for off in (0, 76, 77 + WIN_BYTES, 2 * PITCH - 1, 4 * PITCH + 76):
        buf = _buffer(win)
        buf[off] = 0x00
        with pytest.raises(AssertionError) as e:
            _check(buf, win)
        msg = str(e.value)
        assert "byte %d (= %d mod %d) in frame %d" % (off, off % WRAP, WRAP, off // PITCH) in msg
        assert "got 0x00, expected 0xa5 (the sentinel)" in msg


def test_check_buffer_flags_the_tail():
    win = _windows()
    for back in (1, fm.TAIL):
        buf = _buffer(win)
        buf[buf.size - back] = 0x11
        with pytest.raises(AssertionError) as e:
            _check(buf, win)
        assert "byte %d " % (buf.size - back) in str(e.value) and "the sentinel" in str(e.value)


def test_check_buffer_flags_a_window_at_its_offset_modulo_the_wrap():
    """Frame 4's window written at its offset mod 2^16: it lands in frame 0's picture, and is missing where
    it belongs.  The message names both places, and the two offsets are congruent."""
    win = _windows()
    far = win[4][0]
    assert far >= WRAP and far % WRAP == 4 * 260 + 77
    buf = _buffer(win, at=lambda off: off % WRAP)
    with pytest.raises(AssertionError) as e:
        _check(buf, win)
    msg = str(e.value)
    places = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"byte (\d+) \(= (\d+) mod \d+\) in frame (\d+)", msg)]
    landed = [p for p in places if p[2] == 0]
    missing = [p for p in places if p[2] == 4]
    assert landed and missing, msg
    assert missing[0][0] == far and "expected %#04x (a window's byte)" % win[4][1][0] in msg
    # where it landed: the first byte of the wrapped window that differs from what lies there
    assert far % WRAP <= landed[0][0] < far % WRAP + WIN_BYTES and landed[0][0] % WRAP == landed[0][1]
    assert (missing[0][0] - (far % WRAP)) % WRAP == 0


def test_check_buffer_rejects_overlapping_or_outside_spans():
    buf = torch.full((100,), fm.SENTINEL, dtype=torch.uint8)
    a = torch.zeros(10, dtype=torch.uint8)
    with pytest.raises(AssertionError):
        fm.check_buffer(buf, [(0, a), (5, a)], "overlap")
    with pytest.raises(AssertionError):
        fm.check_buffer(buf, [(95, a)], "outside")


# ---- tight frames ---------------------------------------------------------------------------------------

def _dense_case(batch=9, fb=10000, seed=2):
    rng = np.random.default_rng(seed)
    wants = [torch.from_numpy(rng.integers(0, 256, fb, dtype=np.uint8)) for _ in range(fm.K)]
    buf = torch.full((batch * fb + fm.TAIL,), fm.SENTINEL, dtype=torch.uint8)
    for f in range(batch):
        buf[f * fb:(f + 1) * fb] = wants[f % fm.K]
    return buf, wants, batch, fb


def test_check_dense():
    buf, wants, batch, fb = _dense_case()
    assert batch == fm.dense_batch(fb, WRAP)
    fm.check_dense(buf, fb, batch, wants, "dense", wrap=WRAP)
    fm.check_dense(buf, fb, batch, lambda f: wants[f % fm.K], "dense", wrap=WRAP)
    # a wrong byte in the last frame
    bad = buf.clone()
    off = 6 * fb + 123
    bad[off] ^= 1
    with pytest.raises(AssertionError, match=r"frame 6, 1 bytes, first at byte %d \(= %d mod %d\) in frame 6" % (off, off % WRAP, WRAP)):
        fm.check_dense(bad, fb, batch, wants, "dense", wrap=WRAP)
    # the tail
    bad = buf.clone()
    bad[-1] = 0
    with pytest.raises(AssertionError, match="the tail, first at byte %d" % (batch * fb + fm.TAIL - 1)):
        fm.check_dense(bad, fb, batch, wants, "dense", wrap=WRAP)
    # a frame offset that wrapped: frame 7 (picture 1) was written at 7 * fb mod 2^16 = 4464 -- into frame 0,
    # which holds picture 0 -- and frame 7 still holds the sentinel
    assert 7 * fb >= WRAP and 7 * fb % WRAP == 4464
    bad = buf.clone()
    bad[7 * fb:8 * fb] = fm.SENTINEL
    bad[4464:4464 + fb] = wants[1]
    with pytest.raises(AssertionError) as e:
        fm.check_dense(bad, fb, batch, wants, "dense", wrap=WRAP)
    msg = str(e.value)
    first = int((wants[1] != fm.SENTINEL).to(torch.uint8).argmax())
    assert "3 of 9 frames" in msg and "frame 0, " in msg and "frame 1, " in msg
    assert "frame 7, %d bytes, first at byte %d (= %d mod %d) in frame 7: got 0xa5" % (
        int((wants[1] != fm.SENTINEL).sum()), 7 * fb + first, 4464 + first, WRAP) in msg
    # a frame that holds another frame's picture is named
    bad = buf.clone()
    bad[4 * fb:5 * fb] = wants[2]
    with pytest.raises(AssertionError, match="frame 4, which holds picture 2, not 1"):
        fm.check_dense(bad, fb, batch, wants, "dense", wrap=WRAP)


# ---- the one-row shortcut of the concealing decode's model ------------------------------------------------

@pytest.mark.parametrize("W,H,Cn,ycc,q", [(72, 40, 4, True, 50), (264, 40, 3, False, 90)])
def test_conceal_one_row_is_conceal_model(W, H, Cn, ycc, q):
    img = np.ascontiguousarray(himg_amd.synth("randtile", 2, W, H)[:, :, :Cn])
    good = np.frombuffer(ol.oracle_encode(img, q, ycc), np.uint8).copy()
    fix = ol.oracle_decode(good)[0] != 0
    model = pm.Model(good, fix)
    layout = dm.rows_of(good, fix)[1]
    seen = set()
    for r in range(model.rows):
        o, n = layout[r]
        for at, bit in [(o, 0), (o + n // 2, 4), (o + n - 1, 7), (o + n // 3, 2)]:
            bad = good.copy()
            bad[at] ^= 1 << bit
            pic, rowmap = fm.conceal_one_row(model, bad, r)
            want_pic, want_map = cm.expect(model, bad, fix)
            assert np.array_equal(rowmap, want_map) and np.array_equal(pic, want_pic.reshape(pic.shape)), (r, at, bit)
            seen.add(int(rowmap[r]))
    assert seen == {0, 1}   # both outcomes occurred: a concealed row and an accepted, changed one
