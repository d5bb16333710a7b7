"""GPU (-m gpu): the row-sharded and multi-device paths at the shapes the single-device suite
drives the general kernel forms with -- 1 to 4 channels, pixel_stride > channels, the -rgb mode,
ragged widths and heights, one pixel column, wide rows through HBM.  What these paths add to the
kernels is a first block row above zero and a VIRTUAL frame base (a pointer in front of the buffer
that exists): the halo of a rank's share is uploaded alone, a rank's pixel rows lie between guard
bytes.  Every comparison is byte for byte (word for word) with the CPU oracle."""
import functools
import os
import subprocess

import numpy as np
import pytest

import himg_amd
from himg_amd import build as hb
from himg_amd import sharded

import oracle_lib as ol
from test_cli import _write_pnm, _read_pnm, _freeimage_order

pytestmark = pytest.mark.gpu

# (W, H, channels, pixel_stride, ycbcr, quality)
CASES = [
    (72, 264, 1, 1, True, 50),      # grey, whole tiles, 33 block rows
    (100, 261, 3, 3, True, 70),     # RGB, ragged right and bottom; pitch 300: a virtual base 4-byte aligned at best
    (100, 261, 3, 4, False, 90),    # stride above the channel count, -rgb mode
    (250, 392, 1, 4, True, 50),     # one channel out of four bytes
    (97, 133, 4, 4, True, 50),      # RGBA, ragged width; 17 block rows: of 2 ranks the last owns ONE partial row (5 pixel rows)
    (64, 133, 4, 4, True, 50),      # RGBA, W % 8 == 0, ragged H: the 16-byte-load low-res average with the general tile kernel
    (13, 520, 2, 2, True, 30),      # two tile columns, 2 channels, 65 rows (4 ranks: uneven shares)
    (1, 257, 4, 4, True, 50),       # one pixel column; the last block row is one pixel high
    (264, 257, 4, 4, True, 100),    # densest symbols
    (264, 257, 4, 4, True, 0),      # a stream the reference rejects (trap T2): decoded in the fixed mode
    (6001, 264, 3, 3, True, 50),    # decode only: ragged rows through HBM from a first row above zero
]
WIDE = CASES[-1]
RGB_RAGGED = CASES[1]
SENTINEL = 0x5B
GUARD = 256


def _id(case):
    return "%dx%dx%ds%d%s-q%d" % (case[0], case[1], case[2], case[3], "" if case[4] else "-rgb", case[5])


def _parts(case):
    return (2, 3, 4) if case[1] == 520 else (2, 3)


def _picture(w, h, stride):
    img = himg_amd.synth("randtile", 7 * w + h, w, h)
    return img if stride == 4 else np.ascontiguousarray(img[:, :, :stride])


@functools.lru_cache(maxsize=None)
def _encoded(case):
    """(picture, oracle stream, oracle trace) of a case: computed once, shared, never written to."""
    w, h, ch, stride, ycbcr, q = case
    img = _picture(w, h, stride)
    packed, tr = ol.oracle_encode(img, q, ycbcr, channels=ch, stride=stride, trace=True)
    for a in (img, packed):
        a.setflags(write=False)
    return img, packed, tr


@functools.lru_cache(maxsize=None)
def _decoded(case):
    """(fix_t2, the oracle's pixels [H][W][C]): the plain verdict is 0 for every case but the
    quality-0 one, which the reference refuses (-7) and the fixed mode decodes."""
    w, h, ch, stride, ycbcr, q = case
    packed = _encoded(case)[1]
    rc, pix = ol.oracle_decode(packed)
    fix = q == 0
    assert (rc == -7) if fix else (rc == 0), rc
    if fix:
        rc, pix = ol.oracle_decode(packed, fix_t2=True)
        assert rc == 0
    pix = pix.reshape(h, w, ch)
    pix.setflags(write=False)
    return fix, pix


def _same(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.size == want.size, "%s: %d values, expected %d" % (what, got.size, want.size)
    d = np.flatnonzero(got != want)
    assert d.size == 0, "%s: %d of %d differ, first at %d" % (what, d.size, want.size, d[0])


# ---- a. sharded encode, every rank simulated in one process ------------------------------------

@pytest.mark.parametrize("form", ["assemble", "head"])
@pytest.mark.parametrize("case", CASES[:-1], ids=_id)
def test_sharded_encode_general_shapes(case, form):
    """The device phases of the row-sharded encode as encode_sharded strings them together (the
    structure of test_sharded.py's simulated ranks), each rank holding the halo rows of its share
    and nothing else; through the dense symbol plane and through the token stream.  Stage by stage:
    low-res rows, token histogram, row sizes, stream."""
    import torch
    w, h, ch, stride, ycbcr, q = case
    img, want, tr = _encoded(case)
    rows, cols = (h + 7) // 8, (w + 7) // 8
    assert (tr["rows"], tr["cols"]) == (rows, cols)
    low_want = tr["lowres"].reshape(ch, rows, cols)
    for parts in _parts(case):
        ranges = sharded.shard_rows(rows, parts)
        for tok in (0, 1):
            tag = "%d ranks, row_tokens %d" % (parts, tok)
            backs = []
            for (r0, r1) in ranges:
                y0, y1 = max(0, 8 * r0 - 11), min(h, 8 * r1 + 5)
                if r1 <= r0:
                    y0, y1 = 0, 1
                d = torch.from_numpy(np.array(img[y0:y1])).to("cuda:0")   # the halo rows, to the byte
                assert d.numel() == (y1 - y0) * w * stride
                eng = himg_amd.Engine(0)
                eng.set_option("row_tokens", tok)
                backs.append(sharded.EngineBackend(eng, d, y0, w, h, q, ycbcr, channels=ch, pixel_stride=stride))
            stats = [b.stats(r0, r1) for b, (r0, r1) in zip(backs, ranges)]
            for (r0, r1), s in zip(ranges, stats):
                _same(s[1].cpu().numpy(), low_want[:, r0:r1, :], "%s: low-res rows [%d, %d)" % (tag, r0, r1))
            hist = sum(s[0] for s in stats)
            _same(hist.cpu().numpy(), tr["fres_hist"].astype(np.int64), "%s: token histogram" % tag)
            bits = [b.row_bits(hist) for b in backs]
            all_bits = torch.cat(bits)
            _same((all_bits.cpu().numpy().astype(np.int64) + 7) >> 3, tr["fres_row_bytes"], "%s: row bytes" % tag)
            layout = sharded.fres_layout(all_bits.cpu().numpy(), rows > 1)
            low_full = torch.empty(ch * rows * cols, dtype=torch.uint8, device="cuda:0")
            lf = low_full.view(ch, rows, cols)
            for (r0, r1), s in zip(ranges, stats):
                if r1 > r0:
                    lf[:, r0:r1, :] = s[1].view(ch, r1 - r0, cols)
            if form == "head":
                s0, e0 = sharded.piece_range(layout, *ranges[0])
                buf, base = backs[0].head(low_full, all_bits, s0, e0)
                buf[base + e0: base + layout[3]] = 0xAA            # whatever is not a peer's to send stays rank 0's
                for b, (r0, r1) in list(zip(backs, ranges))[1:]:
                    s, e = sharded.piece_range(layout, r0, r1)
                    if e > s:
                        buf[base + s: base + e] = b.emit(all_bits, s, e)
                out = backs[0].finish(buf)
            else:
                rel_full = torch.empty(layout[3], dtype=torch.uint8, device="cuda:0")
                for b, (r0, r1) in zip(backs, ranges):
                    s, e = sharded.piece_range(layout, r0, r1)
                    rel_full[s:e] = b.emit(all_bits, s, e)
                out = backs[0].assemble(low_full, all_bits, rel_full)
            _same(out, want, "%s: stream" % tag)
            for b in backs:
                b.eng.close()


# ---- b. sharded decode, every rank simulated in one process ------------------------------------

def _upload(packed, fill=0):
    """The stream in HBM, its buffer rounded up to 16 bytes plus 64 (the row kernels read whole
    dwords and a few ahead), the tail `fill`ed."""
    import torch
    cap = (packed.size + 15) // 16 * 16 + 64
    d = torch.full((cap,), fill, dtype=torch.uint8, device="cuda:0")
    d[: packed.size] = torch.from_numpy(np.array(packed)).to("cuda:0")
    return d


class _Guarded:
    """A rank's pixel rows in the middle of ONE tensor of sentinel bytes, 256 guard bytes on each
    side (the start keeps the 16-byte alignment the ABI demands).  The virtual base puts a partial
    last block row at the very end of `rows`: a store form that does not clip it lands in the guard."""

    def __init__(self, nbytes):
        import torch
        self.n = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        self.rows = self.buf[GUARD: GUARD + nbytes]
        assert self.rows.data_ptr() % 16 == 0

    def check(self, want, what):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all(), "%s: bytes written in front of the rank's rows" % what
        assert (got[GUARD + self.n:] == SENTINEL).all(), "%s: bytes written behind the rank's rows" % what
        _same(got[GUARD: GUARD + self.n], want, "%s: pixels" % what)


def _engine(fix):
    eng = himg_amd.Engine(0)
    if fix:
        eng.set_option("fix_t2", 1)
    return eng


@pytest.mark.parametrize("form", ["rows", "indexed", "head_rows"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_sharded_decode_general_shapes(case, form):
    """Every rank decodes its block rows with an engine of its own: by the plain row-range call,
    from a buffer that holds only the head of the stream and its own rows' bytes with the index
    supplied, and in the pipelined form (head phase, then the rows phase, on one context)."""
    import torch
    w, h, ch, stride, ycbcr, q = case
    packed = _encoded(case)[1]
    fix, pix = _decoded(case)
    rows = (h + 7) // 8
    d_full = _upload(packed)
    st = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    gw, gh, gc, off, ln, first = himg_amd.index_host(packed, fix)
    assert (gw, gh, gc) == (w, h, ch)
    d_idx = torch.zeros(2 * rows + 2, dtype=torch.int32, device="cuda:0")
    if form == "indexed":
        eng = _engine(fix)
        eng.decode_index_device(d_full, packed.size, w, h, ch, d_idx, d_idx[2 * rows:], st)
        got = d_idx.cpu().numpy().view(np.uint32)
        assert int(st.item()) == 0 and int(got[2 * rows]) == first
        _same(got[:rows], off, "row offsets")
        _same(got[rows: 2 * rows], ln, "row lengths")
        eng.close()
    else:
        d_idx[: 2 * rows] = torch.from_numpy(np.concatenate([off, ln]).astype(np.uint32).view(np.int32)).to("cuda:0")
    for parts in _parts(case):
        ranges = sharded.shard_rows(rows, parts)
        for (r0, r1), (lo, hi) in zip(ranges, sharded.slice_ranges(off, ln, first, packed.size, ranges)):
            if r1 <= r0:
                continue        # (a rank without rows launches no rows phase: ShardedDecoder, the multi-device handle)
            what = "%d ranks, rows [%d, %d)" % (parts, r0, r1)
            y0, y1 = min(8 * r0, h), min(8 * r1, h)
            out = _Guarded((y1 - y0) * w * ch)
            eng = _engine(fix)
            st.fill_(-1)
            if form == "rows":
                eng.decode_rows_device(d_full, packed.size, w, h, ch, r0, r1, out.rows, st)
            elif form == "indexed":
                d_part = torch.full((d_full.numel(),), 0xAA, dtype=torch.uint8, device="cuda:0")
                head = (first + 15) // 16 * 16
                d_part[:head] = d_full[:head]
                d_part[lo:hi] = d_full[lo:hi]
                eng.decode_rows_indexed_device(d_part, packed.size, w, h, ch, r0, r1, d_idx, out.rows, st)
            else:
                eng.decode_head_device(d_full, packed.size, w, h, ch)
                eng.decode_rows_after_head_device(d_full, packed.size, w, h, ch, r0, r1, d_idx, out.rows, st)
            torch.cuda.synchronize()
            assert int(st.item()) == 0, what
            out.check(pix[y0:y1], what)
            eng.close()


def test_decode_rows_odd_ranges():
    """Row ranges that are no multiples of 16 (the ABI asks for none), unsharded: the second block
    row alone, the partial last one alone, all of them."""
    import torch
    case = RGB_RAGGED
    w, h, ch = case[:3]
    packed = _encoded(case)[1]
    _, pix = _decoded(case)
    rows = (h + 7) // 8
    d_full = _upload(packed)
    st = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    for (r0, r1) in ((1, 2), (rows - 1, rows), (0, rows)):
        y0, y1 = 8 * r0, min(8 * r1, h)
        out = _Guarded((y1 - y0) * w * ch)
        eng = himg_amd.Engine(0)
        st.fill_(-1)
        eng.decode_rows_device(d_full, packed.size, w, h, ch, r0, r1, out.rows, st)
        torch.cuda.synchronize()
        assert int(st.item()) == 0, (r0, r1)
        out.check(pix[y0:y1], "rows [%d, %d)" % (r0, r1))
        eng.close()


# ---- c. damaged streams under sharding ----------------------------------------------------------

def _fres_tree_start(s):
    b, i = bytes(s), 12
    while i + 8 <= len(b):
        if b[i:i + 4] == b"FRES":
            return i + 8
        i += 8 + int.from_bytes(b[i + 4:i + 8], "little")
    raise AssertionError("no FRES chunk")


def test_sharded_decode_damaged_streams():
    """One bit flipped in a row's payload, in a row's size header, in the FRES tree -- drawn by
    seed, judged by the oracle alone: the OR of three ranks' verdicts is the oracle's, and where it
    accepts, the pixels are its pixels.  Among the draws are streams it rejects and streams it
    accepts with other pixels than the undamaged stream's."""
    import torch
    case, parts, per_kind = RGB_RAGGED, 3, 8
    w, h, ch = case[:3]
    packed = _encoded(case)[1]
    _, clean = _decoded(case)
    rows = (h + 7) // 8
    _, _, _, off, ln, first = himg_amd.index_host(packed)
    t0 = _fres_tree_start(packed)
    rng = np.random.RandomState(1000 + w)
    ranges = [r for r in sharded.shard_rows(rows, parts) if r[1] > r[0]]
    engs = [himg_amd.Engine(0) for _ in ranges]
    st = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    rejected = other_pixels = 0
    for kind in ("payload", "header", "tree"):
        for trial in range(per_kind):
            r = int(rng.randint(0, rows))
            if kind == "payload":
                at = int(off[r]) + int(rng.randint(0, int(ln[r])))
            elif kind == "header":
                at = int(off[r]) - 2 + int(rng.randint(0, 2))      # the row's two size bytes
            else:
                at = t0 + int(rng.randint(0, first - t0))
            bad = np.array(packed)
            bad[at] ^= 1 << int(rng.randint(0, 8))
            rc, pix = ol.oracle_decode(bad)
            what = "%s %d (byte %d)" % (kind, trial, at)
            d_bad = _upload(bad)
            failed, outs = False, []
            for eng, (r0, r1) in zip(engs, ranges):
                y0, y1 = min(8 * r0, h), min(8 * r1, h)
                out = _Guarded((y1 - y0) * w * ch)
                st.fill_(-1)
                eng.decode_rows_device(d_bad, bad.size, w, h, ch, r0, r1, out.rows, st)
                torch.cuda.synchronize()
                failed = failed or int(st.item()) != 0
                outs.append((out, y0, y1))
            assert failed == (rc != 0), what
            if rc != 0:
                rejected += 1
                continue
            pix = pix.reshape(h, w, ch)
            other_pixels += int(not np.array_equal(pix, clean))
            for out, y0, y1 in outs:
                out.check(pix[y0:y1], "%s, pixel rows [%d, %d)" % (what, y0, y1))
    for eng in engs:
        eng.close()
    assert rejected >= 1 and other_pixels >= 1, (rejected, other_pixels)


# ---- d. the multi-device handle -----------------------------------------------------------------

SWITCH = [(264, 248, 3, 4, True, 50), (264, 249, 3, 4, True, 50)]    # 31 and 32 block rows: either side of the single-device switch
MULTI_CASES = [c for c in CASES if (c[1] + 7) // 8 >= 32] + SWITCH


def _t2_error_text():
    """himg_hip_last_error after Engine.decode has refused the quality-0 stream."""
    eng = himg_amd.Engine(0)
    with pytest.raises(himg_amd.HimgError) as e:
        eng.decode(_encoded(CASES[9])[1])
    text = himg_amd.lib().himg_hip_last_error(eng._ctx).decode()
    eng.close()
    assert e.value.code == himg_amd.HIMG_ERR_FORMAT and text
    return text


@pytest.mark.parametrize("slots,staged", [(2, 0), (2, 1), (3, 0), (3, 1), (8, 0), (8, 1)])
def test_multi_general_shapes(slots, staged, monkeypatch):
    """himg_hip_multi_encode / _decode with slots that all name GPU 0: streams and pixels are the
    oracle's for every shape of at least 32 block rows and for 31 rows (the single-device path
    behind the same handle); the stream the reference rejects is refused in the single-device
    decoder's words and decoded in the fixed mode."""
    monkeypatch.setenv("HIMG_MULTI_STAGED", str(staged))
    m = himg_amd.MultiEngine([0] * slots)
    for case in MULTI_CASES:
        w, h, ch, stride, ycbcr, q = case
        img, want, _ = _encoded(case)
        fix, pix = _decoded(case)
        if case != WIDE:
            _same(m.encode(img, q, ycbcr, channels=ch, pixel_stride=stride), want, _id(case) + ": stream")
        if fix:
            with pytest.raises(himg_amd.HimgError) as e:
                m.decode(want)
            assert e.value.code == himg_amd.HIMG_ERR_FORMAT
            assert himg_amd.lib().himg_hip_multi_last_error(m._m).decode() == _t2_error_text()
            m.set_option("fix_t2", 1)
        got = m.decode(want)
        assert got.shape == pix.shape, _id(case)
        _same(got, pix, _id(case) + ": pixels")
        if fix:
            m.set_option("fix_t2", 0)
    m.close()


def test_multi_handle_reused_across_geometries():
    """One handle, a large frame, two small ones of other channel counts, the large one again, and
    all of it once more: the slots' buffers only ever grow, so whatever a larger earlier frame left
    in them must not reach a later stream or picture."""
    big = (512, 1024, 4, 4, True, 50)
    m = himg_amd.MultiEngine([0, 0, 0])
    for rnd in range(2):
        for case in (big, RGB_RAGGED, CASES[6], big):
            w, h, ch, stride, ycbcr, q = case
            img, want, _ = _encoded(case)
            _, pix = _decoded(case)
            what = "round %d, %s" % (rnd, _id(case))
            _same(m.encode(img, q, ycbcr, channels=ch, pixel_stride=stride), want, what + ": stream")
            got = m.decode(want)
            assert got.shape == pix.shape, what
            _same(got, pix, what + ": pixels")
    m.close()


# ---- e. the command line under HIMG_DEVICES -----------------------------------------------------

@pytest.mark.parametrize("w,h,ch", [(100, 261, 3), (72, 264, 1)])
def test_cli_shards_pnm_files(tmp_path, w, h, ch):
    """chimg / dhimg with HIMG_DEVICES naming two slots on a P6 and a P5 file (33 block rows: the
    sharded path): the files are the oracle's stream and the oracle's pixels."""
    chimg, dhimg = hb.build_cli()[:2]
    rgba = himg_amd.synth("randtile", 7 * w + h, w, h)
    img = rgba[:, :, 0] if ch == 1 else rgba[:, :, :ch]
    src, packed_path, out_path = tmp_path / "in.pnm", tmp_path / "out.himg", tmp_path / "back.pnm"
    _write_pnm(src, img)
    env = dict(os.environ, HIMG_DEVICES="0,0")
    r = subprocess.run([chimg, "-q", "70", str(src), str(packed_path)], stdout=subprocess.PIPE, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    want = ol.oracle_encode(_freeimage_order(img), 70, True, channels=ch, stride=ch)
    _same(np.fromfile(packed_path, np.uint8), want, "stream")
    assert "Low resolution data: " in r.stdout and "Compressed size: %d" % want.size in r.stdout
    r = subprocess.run([dhimg, str(packed_path), str(out_path)], stdout=subprocess.PIPE, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    rc, pix = ol.oracle_decode(want)
    assert rc == 0
    _same(_freeimage_order(_read_pnm(out_path)), pix.reshape(h, w, ch), "pixels")
