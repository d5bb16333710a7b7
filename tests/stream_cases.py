"""The case table of tests/test_gpu_streams.py: every device entry point on a caller's stream, with its
inputs (a REAL one and a DECOY of the same geometry) and the bytes every output must hold, from the CPU
references the suite already uses for that form -- oracle_lib, scaled_model, tensor_model, prefix_model,
conceal_model, budget_model, target_model.  Host only: no GPU is needed to build the table, and
tests/test_streams_host.py keeps it honest.

A case is a dict:
  id, form, shape      the entry point (FORMS) and the geometry's name (SHAPES)
  geom                 (W, H, C, B)
  fix                  the context's HIMG_OPT_FIX_T2
  opts                 further context options (the forced encoder forms), or {}
  real, decoy          uint8 arrays of one shape: the input buffer's contents
  args                 the call's host arguments
  outs                 {name: {"want": array, "mask": bool array over want's BYTES or None, "init": the byte
                       pattern the buffer holds before the call: an int, or an array (a canvas)}}
Sequences (SEQUENCES) name cases by id.

Test infrastructure only.
"""
from collections import namedtuple

import numpy as np

import budget_model as bm
import conceal_model as cm
import damage_model as dm
import himg_amd
import oracle_lib as ol
import prefix_model as pm
import scaled_model as sm
import target_model as tgm
import tensor_model as tm

SENTINEL = 0x5A

Shape = namedtuple("Shape", "W H C B kind q fix")
# (what each reaches: tests/test_gpu_streams.py.  The 4608-wide one is noise at q = 90: two block rows of q = 50
# tiles would be smaller than a block row's symbols, which the reference decoder rejects -- trap T2.)
SHAPES = {
    "256x64x4": Shape(256, 64, 4, 3, "randtile", 50, False),
    "200x72x4": Shape(200, 72, 4, 3, "randtile", 50, False),
    "520x64x3": Shape(520, 64, 3, 3, "randtile", 50, False),
    "4608x16x4": Shape(4608, 16, 4, 3, "rand", 90, False),
    "256x1024x4": Shape(256, 1024, 4, 1, "randtile", 50, False),
}
ALL_FORMS_SHAPES = ("256x64x4", "520x64x3")
ENCODE_SHAPES = ("256x64x4", "200x72x4", "520x64x3")
REAL_SEED, DECOY_SEED, SIX_SEED = 0, 100, 300

DECODE_FORMS = ("decode", "preview", "region", "regions", "scaled", "scaled_regions", "tensor", "regions_tensor",
                "into", "regions_into", "prefix", "pyramid", "conceal", "rows")
ENCODE_FORMS = ("encode", "encode_q", "sizes", "sse", "budget", "target", "windows")
FORMS = DECODE_FORMS + ENCODE_FORMS


def pictures(shape, seed0):
    s = SHAPES[shape]
    return [np.ascontiguousarray(himg_amd.synth(s.kind, seed0 + f, s.W, s.H)[:, :, :s.C]) for f in range(s.B)]


def streams(shape, seed0):
    s = SHAPES[shape]
    return [ol.oracle_encode(p, s.q, True) for p in pictures(shape, seed0)]


def pack(real, decoy):
    """Two batches of streams in buffers of one stride: (real [B][stride], decoy [B][stride], stride, the
    real sizes)."""
    stride = (max(len(x) for x in real + decoy) + 3 + 255) // 256 * 256
    out = []
    for batch in (real, decoy):
        buf = np.zeros((len(batch), stride), np.uint8)
        for f, x in enumerate(batch):
            buf[f, :len(x)] = x
        out.append(buf)
    return out[0], out[1], stride, np.array([len(x) for x in real], np.uint32)


def _out(want, mask=None, init=SENTINEL):
    return {"want": np.ascontiguousarray(want), "mask": mask, "init": init}


def _ok(n):
    return _out(np.zeros(n, np.int32))


def full_of(stream, fix):
    rc, pix = ol.oracle_decode(stream, fix_t2=fix)
    assert rc == 0, rc
    return pix


def preview_of(stream, fix):
    """The oracle decoder's low-res plane as a picture (what tests/test_gpu_preview.py compares with)."""
    ol.oracle().himg_oracle_set_compat_fix(1 if fix else 0)
    try:
        rc, tr = ol.oracle_decode_trace(np.ascontiguousarray(stream, np.uint8))
    finally:
        ol.oracle().himg_oracle_set_compat_fix(0)
    assert rc == 0
    H, W, C = tr["pixels"].shape
    low = tr["lowres"].reshape(C, (H + 7) // 8, (W + 7) // 8).transpose(1, 2, 0).copy()
    return sm.ycc_to_rgb(low) if pm.stream_ycc(stream) else low


_scaled = {}


def scaled_of(stream, s, fix):
    key = (np.asarray(stream).tobytes(), s, fix)
    if key not in _scaled:
        rc, pix = sm.expected(stream, s, fix)
        assert rc == 0
        _scaled[key] = pix
    return _scaled[key]


def window_origins(W, H, w, h, B, turn=0):
    """An origin per frame inside W x H, odd ones and both far corners among them; `turn` rotates them."""
    pool = [(1, 0), (W - w, H - h), (min(9, W - w), min(7, H - h)), (0, H - h), (W - w, 0), (min(3, W - w), min(5, H - h))]
    return np.array([pool[(f + turn) % len(pool)] for f in range(B)], np.int32)


def canvas(w, h, ps, B, seed):
    """A pitched destination / source for w x h windows: (w + 24) x (h + 16) pictures, padded rows, a gap
    between the pictures; (descriptor arguments, the buffer's size, a background)."""
    cw, ch = w + 24, h + 16
    row_pitch = cw * ps + (12 if ps == 4 else 5)
    frame_pitch = ((ch - 1) * row_pitch + cw * ps + 15) // 16 * 16
    desc = dict(width=cw, height=ch, pixel_stride=ps, row_pitch=row_pitch, frame_pitch=frame_pitch)
    n = B * frame_pitch
    return desc, n, np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def paste(buf, desc, f, x, y, pic):
    """Picture pic (h, w, c) into window f at (x, y) of a pitched buffer: channel bytes only."""
    h, w, c = pic.shape
    ps = desc["pixel_stride"]
    for i in range(h):
        at = f * desc["frame_pitch"] + (y + i) * desc["row_pitch"] + x * ps
        row = buf[at: at + w * ps].reshape(w, ps)
        row[:, :c] = pic[i]


def damaged_header(model, fix):
    """The first one-bit flip in a row's size header after which the oracle rejects the stream while its head
    is sound and conceal_model conceals some rows, not all: (the stream, picture, rowmap)."""
    _, layout = dm.rows_of(model.packed, fix)
    for r in range(1, model.rows):
        for bit in range(8):
            bad = model.packed.copy()
            bad[layout[r][0] - 2] ^= 1 << bit
            if ol.oracle_decode(bad, fix_t2=fix)[0] == 0:
                continue
            code, _, plan = dm.walk_rows(bad, None, None, fix)
            if plan["head_bytes"] == 0:
                continue
            pic, rowmap = cm.expect(model, bad, fix)
            if 0 < int(rowmap.sum()) < model.rows:
                return bad, pic, rowmap
    raise AssertionError("no damaged size header with a sound head and a rejected row")


def prefix_avails(models):
    """Mid-stream: frame f's prefix ends in the middle of a block row's payload, a different row per frame,
    so that at least one whole row is there and at least one is missing."""
    out = []
    for f, m in enumerate(models):
        ends = m.row_ends()
        k = min(1 + 2 * f, m.rows - 1)
        out.append((ends[k] + ends[k + 1]) // 2)
    return np.array(out, np.uint32)


def decode_cases(shape, forms, real_seed=REAL_SEED, tag="", turn=0):
    s = SHAPES[shape]
    W, H, C, B, fix = s.W, s.H, s.C, s.B, s.fix
    real_s, decoy_s = streams(shape, real_seed), streams(shape, DECOY_SEED)
    real, decoy, stride, sizes = pack(real_s, decoy_s)
    full = np.stack([full_of(x, fix) for x in real_s])
    base = dict(shape=shape, geom=(W, H, C, B), fix=fix, opts={})
    common = dict(in_stride=stride, sizes=sizes)
    cases = []

    def add(form, args, outs, name=None, **over):
        c = dict(base, id="%s%s@%s" % (name or form, tag, shape), form=form, real=real, decoy=decoy,
                 args=dict(common, **args), outs=outs)
        c.update(over)
        cases.append(c)

    w, h = W // 2 + 3, H // 2 + 1
    org = window_origins(W, H, w, h, B, turn)
    crops = np.stack([full[f, y:y + h, x:x + w] for f, (x, y) in enumerate(org)])
    for form in forms:
        if form == "decode":
            add(form, {}, {"pix": _out(full), "status": _ok(B)})
        elif form == "preview":
            add(form, {}, {"pix": _out(np.stack([preview_of(x, fix) for x in real_s])), "status": _ok(B)})
        elif form == "region":
            x, y = 13, 5
            add(form, dict(x=x, y=y, w=w, h=h), {"pix": _out(full[:, y:y + h, x:x + w]), "status": _ok(B)})
        elif form == "regions":
            add(form, dict(origins=org, w=w, h=h), {"pix": _out(crops), "status": _ok(B)})
        elif form == "scaled":
            for sc in (1, 2):
                add(form, dict(scale=sc), {"pix": _out(np.stack([scaled_of(x, sc, fix) for x in real_s])), "status": _ok(B)},
                    name="scaled%d" % sc)
        elif form == "scaled_regions":
            ow, oh = (W + 1) // 2, (H + 1) // 2
            sw, sh = ow // 2 + 1, oh // 2 + 1
            so = window_origins(ow, oh, sw, sh, B, turn)
            half = [scaled_of(x, 1, fix) for x in real_s]
            add(form, dict(scale=1, origins=so, w=sw, h=sh),
                {"pix": _out(np.stack([half[f][y:y + sh, x:x + sw] for f, (x, y) in enumerate(so)])), "status": _ok(B)})
        elif form == "tensor":
            for dt, kind, co in ((tm.F32, "imagenet", min(C, 3)), (tm.F16, "mix", C)):
                desc = tm.DESCS[kind](dt, co)
                add(form, dict(dtype=dt, kind=kind, co=co),
                    {"pix": _out(np.stack([tm.expected(full[f], desc) for f in range(B)])), "status": _ok(B)},
                    name="tensor_%s" % ("f32" if dt == tm.F32 else "f16"))
        elif form == "regions_tensor":
            for dt, kind, co in ((tm.F32, "mix", C), (tm.BF16, "imagenet", min(C, 3))):
                desc = tm.DESCS[kind](dt, co)
                add(form, dict(dtype=dt, kind=kind, co=co, origins=org, w=w, h=h),
                    {"pix": _out(np.stack([tm.expected(crops[f], desc) for f in range(B)])), "status": _ok(B)},
                    name="regions_tensor_%s" % ("f32" if dt == tm.F32 else "bf16"))
        elif form == "into":
            desc, n, bg = canvas(W, H, 4, B, 11)       # (3 channels into 4-byte pixels: the alpha that was there stays)
            do = window_origins(desc["width"], desc["height"], W, H, B, turn + 1)
            want = bg.copy()
            for f, (x, y) in enumerate(do):
                paste(want, desc, f, int(x), int(y), full[f])
            add(form, dict(dst=desc, origins=do), {"canvas": _out(want, init=bg), "status": _ok(B)})
        elif form == "regions_into":
            desc, n, bg = canvas(w, h, 4, B, 12)
            do = window_origins(desc["width"], desc["height"], w, h, B, turn + 2)
            want = bg.copy()
            for f, (x, y) in enumerate(do):
                paste(want, desc, f, int(x), int(y), crops[f])
            add(form, dict(src_origins=org, w=w, h=h, dst=desc, dst_origins=do),
                {"canvas": _out(want, init=bg), "status": _ok(B)})
        elif form == "prefix":
            models = [pm.Model(x, fix) for x in real_s]
            avail = prefix_avails(models)
            exp = [m.expect(int(a)) for m, a in zip(models, avail)]
            assert all(e[0] == pm.OK for e in exp)
            add(form, dict(sizes=avail), {"pix": _out(np.stack([e[2] for e in exp])),
                                          "rows": _out(np.array([e[1] for e in exp], np.int32)), "status": _ok(B)})
        elif form == "pyramid":
            add(form, {}, {"level0": _out(full), "level1": _out(np.stack([scaled_of(x, 1, fix) for x in real_s])),
                           "level2": _out(np.stack([scaled_of(x, 2, fix) for x in real_s])),
                           "level3": _out(np.stack([preview_of(x, fix) for x in real_s])), "status": _ok(B)})
        elif form == "conceal":
            f_bad = 1 % B
            bad, pic, rowmap = damaged_header(pm.Model(real_s[f_bad], fix), fix)
            mixed = list(real_s)
            mixed[f_bad] = bad
            c_real, c_decoy, c_stride, c_sizes = pack(mixed, decoy_s)
            pix = full.copy()
            pix[f_bad] = pic.reshape(H, W, C)
            maps = np.zeros((B, (H + 7) // 8), np.uint8)
            maps[f_bad] = rowmap
            add(form, dict(in_stride=c_stride, sizes=c_sizes, damaged=f_bad),
                {"pix": _out(pix), "concealed": _out(maps.sum(1).astype(np.int32)), "rowmap": _out(maps), "status": _ok(B)},
                real=c_real, decoy=c_decoy)
            # ... and, for the sequence behind it, a clean full decode into a buffer whose decoy is the damaged batch
            a_real, a_decoy, a_stride, a_sizes = pack(real_s, mixed)
            add("decode", dict(in_stride=a_stride, sizes=a_sizes), {"pix": _out(full), "status": _ok(B)},
                name="decode_after_conceal", real=a_real, decoy=a_decoy)
        elif form == "rows":
            rows = (H + 7) // 8
            r0, r1 = 1, rows - 1
            one, one_decoy, st1, sz1 = pack(real_s[:1], decoy_s[:1])
            add(form, dict(in_stride=st1, sizes=sz1, row0=r0, row1=r1),
                {"pix": _out(full[0, 8 * r0: min(8 * r1, H)]), "status": _ok(1)}, real=one, decoy=one_decoy,
                geom=(W, H, C, 1))
        else:
            raise KeyError(form)
    return cases


def _sse(pic, q):
    rc, dec = ol.oracle_decode(ol.oracle_encode(pic, q, True), fix_t2=True)
    assert rc == 0
    return tgm.sse(pic, dec)


def encode_cases(shape, forms, opts=None, tag=""):
    s = SHAPES[shape]
    W, H, C, B = s.W, s.H, s.C, s.B
    real_p, decoy_p = pictures(shape, REAL_SEED + 7), pictures(shape, DECOY_SEED + 7)
    real = np.stack(real_p).reshape(B, -1)
    decoy = np.stack(decoy_p).reshape(B, -1)
    cap = himg_amd.max_packed_size(W, H, C)
    base = dict(shape=shape, geom=(W, H, C, B), fix=False, opts=dict(opts or {}))
    quals = [10, 50, 90][:B]
    cases = []

    def stream_outs(want_streams):
        buf, mask = np.zeros((B, cap), np.uint8), np.zeros((B, cap), bool)
        for f, x in enumerate(want_streams):
            buf[f, :len(x)] = x
            mask[f, :len(x)] = True
        return {"out": _out(buf, mask), "sizes": _out(np.array([len(x) for x in want_streams], np.uint32)), "status": _ok(B)}

    def add(form, args, outs, **over):
        c = dict(base, id="%s%s@%s" % (form, tag, shape), form=form, real=real, decoy=decoy,
                 args=dict(out_stride=cap, **args), outs=outs)
        c.update(over)
        cases.append(c)

    size_of = [{} for _ in range(B)]

    def size(f, q):
        if q not in size_of[f]:
            size_of[f][q] = len(ol.oracle_encode(real_p[f], q, True))
        return size_of[f][q]

    for form in forms:
        if form == "encode":
            add(form, dict(quality=50), stream_outs([ol.oracle_encode(p, 50, True) for p in real_p]))
        elif form == "encode_q":
            add(form, dict(qualities=quals), stream_outs([ol.oracle_encode(p, q, True) for p, q in zip(real_p, quals)]))
        elif form == "sizes":
            o = stream_outs([ol.oracle_encode(p, q, True) for p, q in zip(real_p, quals[::-1])])
            add(form, dict(qualities=quals[::-1]), {"sizes": o["sizes"], "status": o["status"]})
        elif form == "sse":
            add(form, dict(qualities=quals), {"sse": _out(np.array([_sse(p, q) for p, q in zip(real_p, quals)], np.uint64)),
                                              "status": _ok(B)})
        elif form == "budget":
            qmin, qmax = 20, 84
            budgets = [size(f, (30, 84, 57)[f % 3]) + (5, 0, -1)[f % 3] for f in range(B)]
            res = [bm.search(lambda q, f=f: size(f, q), budgets[f], qmin, qmax)[0] for f in range(B)]
            assert all(r >= 0 for r in res)
            o = stream_outs([ol.oracle_encode(p, r, True) for p, r in zip(real_p, res)])
            o["quality"] = _out(np.array(res, np.int32))
            add(form, dict(qmin=qmin, qmax=qmax, budgets=budgets), o)
        elif form == "target":
            qmin, qmax = 30, 70
            targets = [_sse(real_p[f], (45, 30, 64)[f % 3]) + (3, 0, 0)[f % 3] for f in range(B)]
            res = [tgm.search(lambda q, f=f: _sse(real_p[f], q), targets[f], qmin, qmax)[0] for f in range(B)]
            assert all(r >= 0 for r in res)
            o = stream_outs([ol.oracle_encode(p, r, True) for p, r in zip(real_p, res)])
            o["quality"] = _out(np.array(res, np.int32))
            o["sse"] = _out(np.array([_sse(p, r) for p, r in zip(real_p, res)], np.uint64))
            add(form, dict(qmin=qmin, qmax=qmax, targets=targets), o)
        elif form == "windows":
            desc, n, bg = canvas(W, H, C, B, 13)
            org = np.array([(5, 3), (1, 0), (desc["width"] - W - 1, desc["height"] - H)][:B], np.int32)   # odd x
            src_real, src_decoy = bg.copy(), np.random.default_rng(14).integers(0, 256, n, dtype=np.uint8)
            for f, (x, y) in enumerate(org):
                paste(src_real, desc, f, int(x), int(y), real_p[f])
                paste(src_decoy, desc, f, int(x), int(y), decoy_p[f])
            add(form, dict(src=desc, origins=org, w=W, h=H, qualities=quals),
                stream_outs([ol.oracle_encode(p, q, True) for p, q in zip(real_p, quals)]), real=src_real, decoy=src_decoy)
        else:
            raise KeyError(form)
    return cases


SIX_SHAPE = "256x64x4"
FORCED_OPTS = {"front": 1, "row_tokens": 1}      # as tests/test_gpu_tokens.py forces them on a small frame

# Sequences on one warm context and one stream, no host wait between the calls (ids of cases below).
SEQUENCES = {
    "four_decodes": ["decode@200x72x4", "preview@520x64x3", "regions@520x64x3", "decode@256x64x4"],
    "four_decodes_reversed": ["decode@256x64x4", "regions@520x64x3", "preview@520x64x3", "decode@200x72x4"],
    "four_encodes": ["encode@256x64x4", "sizes@200x72x4", "budget@256x64x4", "windows@200x72x4"],
    "six_decodes": ["regions#%d@%s" % (k, SIX_SHAPE) for k in range(6)],
    "conceal_then_decode": ["conceal@256x64x4", "decode_after_conceal@256x64x4"],
}
# Two contexts on two streams, issued interleaved: the encode forms on one, the decode forms on the other.
TWO_CONTEXTS = {"encode": ["%s@256x64x4" % f for f in ENCODE_FORMS],
                "decode": ["%s@256x64x4" % f for f in ("decode", "preview", "regions", "scaled1", "prefix", "pyramid", "conceal")]}
# One context moved from one stream to another, ordered by the caller's event.
MOVED = ["decode@256x64x4", "regions@520x64x3"]


def build():
    """Every case, in the order the children run them."""
    cases = []
    for shape in SHAPES:
        cases += decode_cases(shape, DECODE_FORMS if shape in ALL_FORMS_SHAPES else ("decode",))
    for shape in ENCODE_SHAPES:
        cases += encode_cases(shape, ENCODE_FORMS)
    cases += encode_cases("256x64x4", ("encode",), FORCED_OPTS, tag="_forced")
    for k in range(6):
        cases += decode_cases(SIX_SHAPE, ("regions",), SIX_SEED + 10 * k, "#%d" % k, turn=k)
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids), ids
    return cases


def single_ids(cases):
    """The cases of part A: all but those that exist for a sequence alone."""
    return [c["id"] for c in cases if "#" not in c["id"] and not c["id"].startswith("decode_after_conceal")]
