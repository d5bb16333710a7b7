#!/usr/bin/env python3
"""Decode into pitched pictures against what it replaces, one JSON line (GPU box), written to
profiles/into_time.json as well.  B RGBA randtile streams of 4096^2 in HBM, q50 (encoded on the device
beforehand); "decode + copy" is decode_device (decode_regions_device) into a tight buffer followed by a
torch strided copy into the destination -- two expressions are timed, bytes and 4-byte words, and the
faster one is named.  All variants of a case alternated in one process, device events after warm-up,
medians with min - max; every variant's result is compared with decode + copy's.
(a) same picture, same bytes: a tight destination at origin 0 against decode_device.
(b) pitched: destinations 4224 x 4160, the pictures at (64, 32), against decode + copy; again at
    (65, 33), where no tile row is 16-byte aligned.
(c) tiling: 1024 streams of 512^2 tiles into one 16384^2 picture (frame_pitch = 0) against decode + copy.
(d) regions: 256^2 windows at seeded per-frame origins into 512^2 pictures at (128, 128) against
    decode_regions_device + copy.
args: [batch] [iters]"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
it = int(sys.argv[2]) if len(sys.argv) > 2 else 7
W = H = 4096
Q = 50
eng = himg_amd.Engine(0)


def stats(v):
    return {"min": min(v), "median": float(np.median(v)), "max": max(v), "runs": len(v)}


def timed(fns):
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(it):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: stats(v) for k, v in ts.items()}


def u8(*shape):
    return torch.empty(shape, dtype=torch.uint8, device="cuda")


def words(t):
    """A view of 4-byte pixels as int32 elements, the channel dimension gone."""
    return t.view(torch.int32)[..., 0]


COPIES = {"dst[...].copy_(src)": lambda d, s: d.copy_(s),
          "dst.view(int32)[...].copy_(src.view(int32))": lambda d, s: words(d).copy_(words(s))}


class Streams:
    """n streams of w x h RGBA pictures in HBM: encoded on the device from windows of d_src."""

    def __init__(self, d_src, src, org, w, h):
        n = len(org)
        self.n, self.w, self.h = n, w, h
        self.stride = (himg_amd.max_packed_size(w, h, 4) + 255) // 256 * 256
        self.d = torch.zeros((n, self.stride), dtype=torch.uint8, device="cuda")
        d_sz = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_st = torch.ones(n, dtype=torch.int32, device="cuda")
        eng.encode_windows_device(d_src, src, n, 4, org, w, h, [Q] * n, True, self.d, self.stride, d_sz, d_st)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any()
        self.sizes = d_sz.cpu().numpy().astype(np.uint32)
        self.st = torch.ones(n, dtype=torch.int32, device="cuda")

    def ok(self):
        torch.cuda.synchronize()
        assert not self.st.cpu().numpy().any()

    def decode(self, d_out):
        eng.decode_device(self.d, self.stride, self.sizes, self.n, self.w, self.h, 4, d_out, self.st)

    def into(self, d_dst, dst, org):
        eng.decode_into_device(self.d, self.stride, self.sizes, self.n, self.w, self.h, 4, d_dst, dst, org, self.st)


def best_copy(t, prefix):
    names = [k for k in t if k.startswith(prefix)]
    best = min(names, key=lambda k: t[k]["median"])
    return best, t[best]["median"]


with ThreadPoolExecutor(16) as pool:
    frames = list(pool.map(lambda s: himg_amd.synth("randtile", s, W, H), range(B)))
d_tight = u8(B, H, W, 4)
for f, fr in enumerate(frames):
    d_tight[f] = torch.from_numpy(fr).cuda()
del frames
zero = np.zeros((B, 2), np.int32)
S = Streams(d_tight, himg_amd.src_desc(W, H, 4), zero, W, H)
res = {"iters": it, "frames": B, "content": "randtile q%d RGBA %dx%d" % (Q, W, H),
       "mean_stream_bytes": float(S.sizes.mean())}

# (a) the two forms, the same bytes
d_out, d_out2 = u8(B, H, W, 4), d_tight   # (the source pictures are no longer needed: their buffer is reused)
tight = himg_amd.dst_desc(W, H, 4)
t = timed({"decode_device": lambda: S.decode(d_out), "into_tight": lambda: S.into(d_out2, tight, zero)})
S.ok()
assert torch.equal(d_out, d_out2)
e, p = t["decode_device"], t["into_tight"]
t["into_median_inside_decode_device_range"] = bool(e["min"] <= p["median"] <= e["max"])
t["into_over_decode_device"] = p["median"] / e["median"]
res["a_same_bytes"] = t
del d_out2, d_tight
torch.cuda.empty_cache()

# (b) pitched destinations
DW, DH = W + 128, H + 64
pitched = himg_amd.dst_desc(DW, DH, 4)
d_pa, d_pb = torch.zeros((B, DH, DW, 4), dtype=torch.uint8, device="cuda"), torch.zeros((B, DH, DW, 4), dtype=torch.uint8, device="cuda")
fns = {}
for x, y in ((64, 32), (65, 33)):
    org = np.tile(np.int32([x, y]), (B, 1))
    fns["into_%d_%d" % (x, y)] = lambda org=org: S.into(d_pa, pitched, org)
    for name, cp in COPIES.items():
        def both(x=x, y=y, cp=cp):
            S.decode(d_out)
            cp(d_pb[:, y:y + H, x:x + W], d_out)
        fns["decode_copy_%d_%d %s" % (x, y, name)] = both
t = timed(fns)
for x, y in ((64, 32), (65, 33)):
    d_pa.zero_(); d_pb.zero_()
    fns["into_%d_%d" % (x, y)]()
    fns["decode_copy_%d_%d %s" % (x, y, next(iter(COPIES)))]()
    S.ok()
    assert torch.equal(d_pa, d_pb)
    best, m = best_copy(t, "decode_copy_%d_%d" % (x, y))
    t["copy_best_%d_%d" % (x, y)] = best
    t["into_over_decode_copy_%d_%d" % (x, y)] = t["into_%d_%d" % (x, y)]["median"] / m
t["odd_over_aligned"] = t["into_65_33"]["median"] / t["into_64_32"]["median"]
t["destination"] = [DW, DH]
res["b_pitched"] = t
del d_pa, d_pb, fns
torch.cuda.empty_cache()

# (c) tiling: one 16384^2 picture (4 x 4 of the decoded frames) as 1024 tile streams of 512^2
if B >= 16:
    G, T = 16384, 512
    NT = (G // T) ** 2
    S.decode(d_out)
    S.ok()
    d_big = d_out[:16].view(4, 4, H, W, 4).permute(0, 2, 1, 3, 4).reshape(G, G, 4).contiguous()
    grid = np.int32([(x, y) for y in range(0, G, T) for x in range(0, G, T)])
    ST = Streams(d_big, himg_amd.src_desc(G, G, 4, frame_pitch=0), grid, T, T)
    big = himg_amd.dst_desc(G, G, 4, frame_pitch=0)
    d_tiles, d_big2 = u8(NT, T, T, 4), torch.zeros((G, G, 4), dtype=torch.uint8, device="cuda")
    d_big.zero_()
    fns = {"into": lambda: ST.into(d_big, big, grid)}
    for name, cp in COPIES.items():
        def both(cp=cp):
            ST.decode(d_tiles)
            cp(d_big2.view(G // T, T, G // T, T, 4).permute(0, 2, 1, 3, 4), d_tiles.view(G // T, G // T, T, T, 4))
        fns["decode_copy %s" % name] = both
    fns["decode_device_tiles_alone"] = lambda: ST.decode(d_tiles)
    t = timed(fns)
    ST.ok()
    assert torch.equal(d_big, d_big2)
    best, m = best_copy(t, "decode_copy")
    t["copy_best"] = best
    t["into_over_decode_copy"] = t["into"]["median"] / m
    t["into_over_decode_device"] = t["into"]["median"] / t["decode_device_tiles_alone"]["median"]
    t["picture"], t["tile"], t["tiles"] = [G, G], [T, T], NT
    res["c_tiling"] = t
    del d_big, d_big2, d_tiles, ST, fns
    torch.cuda.empty_cache()

# (d) regions into pictures
R, P, DX, DY = 256, 512, 128, 128
rng = np.random.default_rng(20261019)
ORG = np.stack([rng.integers(0, W - R + 1, B), rng.integers(0, H - R + 1, B)], axis=1).astype(np.int32)
DORG = np.tile(np.int32([DX, DY]), (B, 1))
pics = himg_amd.dst_desc(P, P, 4)
d_crop = u8(B, R, R, 4)
d_pa, d_pb = torch.zeros((B, P, P, 4), dtype=torch.uint8, device="cuda"), torch.zeros((B, P, P, 4), dtype=torch.uint8, device="cuda")


def regions():
    eng.decode_regions_device(S.d, S.stride, S.sizes, B, W, H, 4, ORG, R, R, d_crop, S.st)


fns = {"regions_into": lambda: eng.decode_regions_into_device(S.d, S.stride, S.sizes, B, W, H, 4, ORG, R, R, d_pa, pics,
                                                               DORG, S.st)}
for name, cp in COPIES.items():
    def both(cp=cp):
        regions()
        cp(d_pb[:, DY:DY + R, DX:DX + R], d_crop)
    fns["regions_copy %s" % name] = both
fns["decode_regions_device_alone"] = regions
t = timed(fns)
S.ok()
assert torch.equal(d_pa, d_pb)
best, m = best_copy(t, "regions_copy")
t["copy_best"] = best
t["into_over_regions_copy"] = t["regions_into"]["median"] / m
t["into_over_decode_regions_device"] = t["regions_into"]["median"] / t["decode_regions_device_alone"]["median"]
t["window"], t["picture"], t["origins"] = [R, R], [P, P], "seeded uniform (numpy default_rng(20261019))"
res["d_regions"] = t

eng.close()
line = json.dumps(res)
print(line)
if os.environ.get("HIMG_INTO_TIME_WRITE", "1") == "1":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "into_time.json"), "w") as f:
        f.write(line + "\n")
