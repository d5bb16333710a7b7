"""What a decode that looks at only part of a stream must say about a DAMAGED stream (include/himg_hip.h:
the region decode and its scaled, tensor and pitched forms, the prefix decode), in numpy and plain Python,
with the CPU oracle as the only judge of a payload.

Block rows are independently coded units behind their own size headers.  So the bytes a form sees can be
respliced into a COMPLETE stream: the good stream's head, the rows the form sees with the payloads that the
damaged stream's header chain delimits, every other row with the good stream's payload.  The oracle's full
decode of that stream is the form's verdict, and its pixel rows of the seen block rows are the form's pixels.
tests/test_damage_model_host.py proves the premises (identity, row independence) with the oracle alone.

The header walk is prefix_model's (one copy of the decoder's rules: _head and _rows), bounded at a region's
last row.  Also here: the seeded corpus of damaged streams that test_damage_model_host.py counts and
test_gpu_partial_damage.py runs.

Test infrastructure only.
"""
import functools
import hashlib
import struct
from collections import namedtuple

import numpy as np

import himg_amd
import oracle_lib as ol
import prefix_model as pm
import scaled_model as sm

OK, FORMAT, CAPACITY = pm.OK, pm.FORMAT, pm.CAPACITY


def _bytes(s):
    return s if isinstance(s, bytes) else np.ascontiguousarray(s, np.uint8).tobytes()


def walk_rows(stream, upto, avail=None, fix=False):
    """The decoder's header rules over rows 0 .. upto-1 of the first `avail` bytes (default: all) of a stream,
    to the end of the chunk when upto is the frame's rows or None ("fewer blocks than block rows", "a header
    crosses the end of the chunk" included): (OK / FORMAT / CAPACITY, [(payload offset, length)] of the rows
    delimited, the plan as prefix_model.walk fills it)."""
    b = _bytes(stream)[:avail]
    p, ranges = pm.empty_plan(), []
    try:
        q, end = pm._head(b, fix, p)
        pm._rows(b, fix, p, q, end, upto, ranges)
    except pm._Short:
        return CAPACITY, ranges, p
    except pm._Format:
        return FORMAT, ranges, p
    return OK, ranges, p


def rows_of(stream, fix=False):
    """(head_bytes, [(payload offset, length)] of every block row) of a stream the walk accepts
    (huffman_dec.cpp:232-248: a 2-byte header, 4 bytes when bit 15 is set with n = low15 | next16 << 15; under
    fix_t2 a frame of one block row has no header)."""
    code, ranges, p = walk_rows(stream, None, None, fix)
    assert code == OK and len(ranges) == p["rows"], (code, len(ranges), p)
    return p["head_bytes"], ranges


def _size_header(n):
    """huffman_enc.cpp:342-352."""
    if n <= 0x7fff:
        return struct.pack("<H", n)
    return struct.pack("<HH", (n & 0x7fff) | 0x8000, n >> 15)


def resplice(good, payloads, fix=False):
    """A complete stream: good[:head_bytes], then each payload behind a freshly written size header (none
    for the one block row of a fix_t2 frame), what follows good's FRES chunk, and the FRES chunk's and the
    RIFF sizes patched."""
    g = _bytes(good)
    p = pm.empty_plan()
    head, end = pm._head(g, fix, p)
    coff, csz = sm.find_chunks(g)["FRES"]
    assert coff + csz == end and len(payloads) == p["rows"]
    if fix and p["rows"] == 1:
        body = bytes(payloads[0])
    else:
        body = b"".join(_size_header(len(x)) + bytes(x) for x in payloads)
    out = bytearray(g[:head] + body + g[end:])
    struct.pack_into("<I", out, coff - 4, head - coff + len(body))
    struct.pack_into("<I", out, 4, len(out) - 8)
    return bytes(out)


_judged, _scaled = {}, {}


def _fix_for(X, fix):
    """Trap T2 compares the FRES chunk's size, a field of the head, which every form sees as the damaged
    stream has it -- and there it passed, or the walk would not have come here.  X's chunk has a size of its
    own (a damaged header delimits another payload), so where X alone would fall into the trap it is judged
    under the encoder's rule (the oracle's compat fix), which changes nothing else for a stream whose trees
    hold more than one symbol (test_damage_model_host.py: test_fix_changes_nothing_else)."""
    if fix:
        return True
    try:
        pm._head(X, False, pm.empty_plan())
    except pm._Format:
        return True
    return False


def judge(X, fix):
    """(rc, pixels) of the oracle's full decode of a respliced stream, kept by the stream's hash."""
    key = (hashlib.sha1(X).digest(), bool(fix))
    if key not in _judged:
        if len(_judged) > 600:
            _judged.clear()
        _judged[key] = ol.oracle_decode(np.frombuffer(X, np.uint8), fix_t2=_fix_for(X, fix))
    return _judged[key]


def scaled(X, scale_log2, fix):
    """scaled_model.expected of a respliced stream the oracle accepts: the picture at 1/2 or 1/4 scale."""
    key = (hashlib.sha1(X).digest(), scale_log2, bool(fix))
    if key not in _scaled:
        if len(_scaled) > 600:
            _scaled.clear()
        rc, img = sm.expected(np.frombuffer(X, np.uint8), scale_log2, _fix_for(X, fix))
        assert rc == 0
        _scaled[key] = img
    return _scaled[key]


def expect_rows(good, bad, seen_rows, fix, avail=None):
    """The verdict and pixels of a form that sees the head, the payloads of block rows `seen_rows` (a range)
    and -- a region (avail None) -- the size headers of rows 0 .. seen_rows[-1] (all of them, to the end of
    the chunk, when that is the last row), or -- a prefix -- every header that lies wholly in bad[:avail].
    For damage at or after head_bytes.  (OK, the oracle's picture of X, X) or (FORMAT, None, X or None):
    only the pixel rows of seen_rows are the form's."""
    seen = range(seen_rows[0], seen_rows[-1] + 1)
    upto = None if avail is not None else seen[-1] + 1
    code, ranges, _ = walk_rows(bad, upto, avail, fix)
    if code != OK:
        return code, None, None
    assert len(ranges) > seen[-1]
    g, b = _bytes(good), _bytes(bad)
    _, layout = rows_of(g, fix)
    payloads = [b[ranges[r][0]:ranges[r][0] + ranges[r][1]] if r in seen else g[o:o + n] for r, (o, n) in enumerate(layout)]
    X = resplice(g, payloads, fix)
    rc, img = judge(X, fix)
    return (FORMAT, None, X) if rc != 0 else (OK, img, X)


def expect_region(good, bad, rect, fix):
    """expect_rows for the rectangle (x, y, w, h) at full resolution: (code, the crop or None, X)."""
    x, y, w, h = rect
    code, img, X = expect_rows(good, bad, range(y // 8, (y + h + 7) // 8), fix)
    return code, (img[y:y + h, x:x + w] if code == OK else None), X


def expect_prefix(model, bad, avail, fix):
    """(code, k or -1, picture or None) of bad[:avail], for damage at or after head_bytes.  `model` is
    prefix_model.Model(good): the fill of the rows that have not arrived depends on the head alone, which
    damage of this kind leaves intact, so it is the good stream's."""
    code, p = pm.walk(bad, avail, fix)
    if code != OK:
        return code, -1, None
    k = p["rows_complete"]
    if k == 0:
        return OK, 0, model.fill.copy()
    code, img, _ = expect_rows(model.packed, bad, range(k), fix, avail)
    if code != OK:
        return code, -1, None
    out = model.fill.copy()
    out[:8 * k] = img[:8 * k]
    return OK, k, out


# ---- the corpus ------------------------------------------------------------------------------------------

Base = namedtuple("Base", "name kind W H C q ycc fix n win")
# n: streams per class (fewer on the wide bases, whose oracle work dominates); win: the window (w, h) that
# the device forms with one window size per launch use.  fix: decoded under HIMG_OPT_FIX_T2 -- the two
# bases that are there for it, and the 4352-wide one, whose three rows of q50 tiles are smaller than a block
# row's symbols (trap T2: the reference rejects it as it stands).
BASES = [
    Base("randtile256x72", "randtile", 256, 72, 4, 50, True, False, 240, (100, 20)),   # nine rows, a single row in the last group
    Base("gradn61x27", "gradn", 61, 27, 3, 90, True, False, 240, (30, 10)),            # ragged
    Base("rand64x16c1", "rand", 64, 16, 1, 50, False, False, 240, (20, 6)),            # no YCbCr
    Base("randtile4352x24", "randtile", 4352, 24, 4, 50, True, True, 120, (4300, 9)),  # two column strips of the region kernel's LDS layout
    Base("rand4096x24q100", "rand", 4096, 24, 4, 100, True, False, 120, (300, 9)),     # 4-byte size headers
    Base("grad40x40q0", "grad", 40, 40, 4, 0, True, True, 240, (17, 11)),              # trap T2
    Base("randtile40x8", "randtile", 40, 8, 4, 50, True, True, 120, (17, 5)),          # one block row, no header
]
BASE = {b.name: b for b in BASES}
SEED = 20260


@functools.lru_cache(maxsize=None)
def good_model(name):
    """prefix_model.Model of the base's oracle-encoded stream."""
    b = BASE[name]
    img = himg_amd.synth(b.kind, 0, b.W, b.H)
    img = np.ascontiguousarray(img[:, :, :b.C] if b.C > 1 else img[:, :, 0])
    s = np.frombuffer(ol.oracle_encode(img, b.q, b.ycc), np.uint8).copy()
    return pm.Model(s, b.fix)


Stream = namedtuple("Stream", "bad rows")   # rows: the damaged block rows, sorted (class C: ())


@functools.lru_cache(maxsize=None)
def streams(name, cls):
    """The damaged streams of a base and class, seeded.
    P: 1-3 bit flips strictly inside the payloads of 1-2 rows.
    H: one bit flipped in one row's size header, any of its 2 or 4 bytes (none in a frame of one row).
    C: one bit flipped below head_bytes -- but not in the RIFF size word nor in FRMT's width, height and
       channel count: the device entries are called with the caller's buffer and geometry, and a stream that
       contradicts them is the full decode's fuzz (test_gpu_fuzz.py)."""
    b, m = BASE[name], good_model(name)
    rng = np.random.default_rng([SEED, BASES.index(b), "PHC".index(cls)])
    head, layout = rows_of(m.packed, b.fix)
    out = []
    if cls == "H" and b.fix and m.rows == 1:
        return out
    for _ in range(b.n):
        bad = m.packed.copy()
        if cls == "P":
            rows = sorted(int(r) for r in rng.choice(m.rows, size=min(m.rows, int(rng.integers(1, 3))), replace=False))
            hit = list(rows) + [rows[int(rng.integers(0, len(rows)))] for _ in range(int(rng.integers(0, 4 - len(rows))))]
            for r in hit:
                o, n = layout[r]
                bad[o + int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
            if np.array_equal(bad, m.packed):   # (two flips of one bit)
                bad[layout[rows[0]][0]] ^= 1
        elif cls == "H":
            r = int(rng.integers(0, m.rows))
            o, n = layout[r]
            hdr = 4 if n > 0x7fff else 2
            bad[o - 1 - int(rng.integers(0, hdr))] ^= 1 << int(rng.integers(0, 8))
            rows = [r]
        else:
            while True:
                i = int(rng.integers(0, head))
                if not (4 <= i < 8 or 21 <= i < 30):
                    break
            bad[i] ^= 1 << int(rng.integers(0, 8))
            rows = []
        out.append(Stream(bad, tuple(rows)))
    return out


def _span_y(rng, H, h, d):
    """An origin y of a window of height h whose block rows contain row d in about half of the draws and lie
    above it or below it in the others (where such a window exists)."""
    ys = np.arange(0, H - h + 1)
    r0, r1 = ys // 8, (ys + h + 7) // 8
    sets = {"in": ys[(r0 <= d) & (d < r1)], "above": ys[r1 <= d], "below": ys[r0 > d]}
    mode = ("in", "in", "above", "below")[int(rng.integers(0, 4))]
    pick = sets[mode] if len(sets[mode]) else sets["in"] if len(sets["in"]) else ys
    return int(pick[int(rng.integers(0, len(pick)))])


@functools.lru_cache(maxsize=None)
def origins(name, cls):
    """Per stream, the origin (x, y) of the base's window `win`: the device forms with an origin per frame."""
    b = BASE[name]
    rng = np.random.default_rng([SEED + 1, BASES.index(b), "PHC".index(cls)])
    w, h = b.win
    return [(int(rng.integers(0, b.W - w + 1)), _span_y(rng, b.H, h, s.rows[0])) for s in streams(name, cls)]


@functools.lru_cache(maxsize=None)
def rects(name, cls):
    """Per stream, a random rectangle (x, y, w, h) whose row span is drawn like _span_y's: decode_region and
    the host batch."""
    b = BASE[name]
    rng = np.random.default_rng([SEED + 2, BASES.index(b), "PHC".index(cls)])
    out = []
    for s in streams(name, cls):
        h = int(rng.integers(1, b.H + 1))
        y = _span_y(rng, b.H, h, s.rows[0])
        x = int(rng.integers(0, b.W))
        out.append((x, y, int(rng.integers(1, b.W - x + 1)), h))
    return out


def one_rect(name):
    """The rectangle of decode_region_device (one for the whole batch): the base's window over its middle rows
    (over its first ones in a frame of three rows or fewer, so that a row stays below it where there is one)."""
    b = BASE[name]
    w, h = b.win
    rows = (b.H + 7) // 8
    return (min(3, b.W - w), min(8 * (rows // 3) + 3 if rows > 3 else 1, b.H - h), w, h)


@functools.lru_cache(maxsize=None)
def avails(name, cls):
    """Per stream of class P or H, the prefix lengths: head_bytes, just behind the (first) damaged row's
    header, inside its payload, just behind it, a random one, and T."""
    b, m = BASE[name], good_model(name)
    rng = np.random.default_rng([SEED + 3, BASES.index(b), "PHC".index(cls)])
    head, layout = rows_of(m.packed, b.fix)
    out = []
    for s in streams(name, cls):
        o, n = layout[s.rows[0]]
        out.append(sorted({head, o, o + n // 2, o + n, int(rng.integers(head, m.T + 1)), m.T}))
    return out


def region_cases(name, cls):
    """Every region case of a base and class: (stream index, rectangle) over rects, origins and one_rect."""
    b = BASE[name]
    n = len(streams(name, cls))
    out = [(i, r) for i, r in enumerate(rects(name, cls))]
    out += [(i, (x, y) + b.win) for i, (x, y) in enumerate(origins(name, cls))]
    return out + [(i, one_rect(name)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def outcomes(name):
    """How the cases of classes P and H of a base come out, by the model alone:
      P  'damaged'   accepted, with other pixels than the good stream's inside the seen rows
         'rejected'  rejected by damage inside the seen rows
         'outside'   no damaged row is seen: accepted, the good pixels
         'same'      accepted, and the damage (pad bits, say) changed no pixel of the seen rows
      H  'walk'      the walk over the headers the form sees rejects
         'past'      the walk passes and went over the damaged header (whatever the oracle then says)
         'unseen'    the damaged header is not among those the form sees
    over region_cases and every prefix length of avails."""
    b, m = BASE[name], good_model(name)
    cnt = dict(damaged=0, rejected=0, outside=0, same=0, walk=0, past=0, unseen=0)

    def count_p(hit, seen, code, img):
        lo, hi = 8 * seen[0], 8 * seen[-1] + 8
        if not any(r in seen for r in hit):
            assert code == OK and np.array_equal(img[lo:hi], m.full[lo:hi])
            cnt["outside"] += 1
        elif code != OK:
            cnt["rejected"] += 1
        else:
            cnt["same" if np.array_equal(img[lo:hi], m.full[lo:hi]) else "damaged"] += 1

    for cls in "PH":
        ss = streams(name, cls)
        for i, (x, y, w, h) in region_cases(name, cls):
            seen = range(y // 8, (y + h + 7) // 8)
            code, img, X = expect_rows(m.packed, ss[i].bad, seen, b.fix)
            if cls == "P":
                count_p(ss[i].rows, seen, code, img)
            elif seen[-1] + 1 < m.rows and ss[i].rows[0] > seen[-1]:
                assert code == OK and X == m.packed.tobytes()
                cnt["unseen"] += 1
            else:
                cnt["walk" if X is None else "past"] += 1
        for s, av in zip(ss, avails(name, cls)):
            for a in av:
                wcode, p = pm.walk(s.bad, a, b.fix)
                k = p["rows_complete"] if wcode == OK else 0
                if cls == "H":
                    cnt["walk" if wcode != OK else "past" if k > s.rows[0] else "unseen"] += 1
                elif k == 0:
                    assert wcode == OK
                    cnt["outside"] += 1
                else:
                    code, _, pic = expect_prefix(m, s.bad, a, b.fix)
                    count_p(s.rows, range(k), code, pic)
    return cnt


@functools.lru_cache(maxsize=None)
def head_cases(name):
    """Class C, the prefix decode alone.  Per stream: (oracle rc of the full decode, [(avail, kind, code, k,
    picture)]) with kind
      'walk'    the walk rejects (FORMAT) or is short (CAPACITY): that code;
      'head'    the walk passes and the oracle fails in a head stage (rc -6 .. -1): FORMAT;
      'model'   the oracle accepts: prefix_model.Model(bad).expect(avail) in full;
      'fres'    the oracle fails in the FRES stage: FORMAT at avail = T, accepted with k = 0 where the prefix
                holds no whole row;
      'open'    the FRES stage fails and the prefix holds whole rows below T: not judged.
    avail: T, head_bytes and head_bytes + 1 (k = 0), a random one behind; and, only where the oracle accepts
    (the header leaves a body check below head_bytes to the decoder's order), head_bytes - 1 and a random one
    below."""
    b, m = BASE[name], good_model(name)
    rng = np.random.default_rng([SEED + 4, BASES.index(b)])
    out = []
    for s in streams(name, "C"):
        T = s.bad.size
        rc, _ = ol.oracle_decode(s.bad, fix_t2=b.fix)
        hb = pm.walk(s.bad, T, b.fix)[1]["head_bytes"] or m.plan["head_bytes"]
        hb = min(hb, T)
        av = {T, hb, min(hb + 1, T), int(rng.integers(hb, T + 1))}
        if rc == 0:
            av |= {hb - 1, int(rng.integers(0, hb))}
        bm = pm.Model(s.bad, b.fix) if rc == 0 else None
        cases = []
        for a in sorted(av):
            code, p = pm.walk(s.bad, a, b.fix)
            if code != OK:
                cases.append((a, "walk", code, -1, None))
            elif -6 <= rc <= -1:
                cases.append((a, "head", FORMAT, -1, None))
            elif rc == 0:
                cases.append((a, "model") + bm.expect(a))
            elif a == T:
                cases.append((a, "fres", FORMAT, -1, None))
            elif p["rows_complete"] == 0:
                cases.append((a, "fres", OK, 0, None))
            else:
                cases.append((a, "open", None, None, None))
        out.append((rc, cases))
    return out
