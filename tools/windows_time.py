#!/usr/bin/env python3
"""Window encode against what it replaces, one JSON line (GPU box), written to
profiles/windows_time.json as well.  B RGBA randtile frames of 4096^2 in HBM, q50; "copy + encode" is a
torch .contiguous() copy of the crop followed by encode_device_q.  All variants of a case alternated in
one process, device events after warm-up, medians with min - max.
(a) same picture, same bytes: windows 4096^2 at (0, 0) of the tight buffer against encode_device_q on it.
(b) pitched: windows 4096^2 at (64, 32) of B sources 4224 x 4160 against copy + encode; again at
    (65, 33), where every tile load is under-aligned.
(c) tiling: one 16384^2 frame, frame_pitch = 0, 1024 windows 512^2 on the tile grid, against copy +
    encode of the 1024 tiles and against encode_device_q on tiles copied beforehand.
(d) regions of interest: 256^2 windows at seeded per-frame origins against copy + encode (the crops
    gathered by one indexing expression, and by a stack of slices).
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


class Out:
    """Output buffers of a batch of n windows w x h."""

    def __init__(self, n, w, h):
        self.n, self.cap = n, himg_amd.max_packed_size(w, h, 4)
        self.out = torch.empty((n, self.cap), dtype=torch.uint8, device="cuda")
        self.sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.st = torch.ones(n, dtype=torch.int32, device="cuda")

    def same(self, other):
        torch.cuda.synchronize()
        assert not self.st.cpu().numpy().any() and not other.st.cpu().numpy().any()
        a, b = self.sizes.cpu().numpy(), other.sizes.cpu().numpy()
        assert np.array_equal(a, b) and a.all()
        top = int(a.max())
        assert torch.equal(self.out[:, :top], other.out[:, :top])


def enc_q(d_frames, n, w, h, o):
    eng.encode_device_q(d_frames, n, w, h, 4, 4, [Q] * n, True, o.out, o.cap, o.sizes, o.st)


def enc_w(d_src, src, org, w, h, o):
    eng.encode_windows_device(d_src, src, o.n, 4, org, w, h, [Q] * o.n, True, o.out, o.cap, o.sizes, o.st)


with ThreadPoolExecutor(16) as pool:
    frames = list(pool.map(lambda s: himg_amd.synth("randtile", s, W, H), range(B)))
d_tight = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
for f, fr in enumerate(frames):
    d_tight[f] = torch.from_numpy(fr).cuda()
del frames
res = {"iters": it, "frames": B, "content": "randtile q%d RGBA %dx%d" % (Q, W, H)}

# (a) the two forms on the same bytes
o1, o2 = Out(B, W, H), Out(B, W, H)
tight = himg_amd.src_desc(W, H, 4)
zero = np.zeros((B, 2), np.int32)
t = timed({"encode_device_q": lambda: enc_q(d_tight, B, W, H, o1),
           "windows_tight": lambda: enc_w(d_tight, tight, zero, W, H, o2)})
o1.same(o2)
e, w_ = t["encode_device_q"], t["windows_tight"]
t["windows_median_inside_encode_q_range"] = bool(e["min"] <= w_["median"] <= e["max"])
t["windows_over_encode_q"] = w_["median"] / e["median"]
res["a_same_bytes"] = t

# (b) pitched sources: every byte of them picture content, so that a window anywhere is a randtile picture
SW, SH = W + 128, H + 64
d_pitched = torch.empty((B, SH, SW, 4), dtype=torch.uint8, device="cuda")
d_pitched[:, :H, :W] = d_tight
d_pitched[:, H:, :W] = d_tight[:, :SH - H]
d_pitched[:, :, W:] = d_pitched[:, :, :SW - W]
pitched = himg_amd.src_desc(SW, SH, 4)
d_copy = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")


def copy_encode_b(x, y):
    d_copy.copy_(d_pitched[:, y:y + H, x:x + W])   # (what .contiguous() does, into a buffer kept across repetitions)
    enc_q(d_copy, B, W, H, o1)


even, odd = np.tile(np.int32([64, 32]), (B, 1)), np.tile(np.int32([65, 33]), (B, 1))
t = timed({"windows_64_32": lambda: enc_w(d_pitched, pitched, even, W, H, o2),
           "copy_encode_64_32": lambda: copy_encode_b(64, 32),
           "windows_65_33": lambda: enc_w(d_pitched, pitched, odd, W, H, o2),
           "copy_encode_65_33": lambda: copy_encode_b(65, 33)})
for org, xy in ((even, (64, 32)), (odd, (65, 33))):
    enc_w(d_pitched, pitched, org, W, H, o2)
    copy_encode_b(*xy)
    o1.same(o2)
t["windows_over_copy_encode_64_32"] = t["windows_64_32"]["median"] / t["copy_encode_64_32"]["median"]
t["windows_over_copy_encode_65_33"] = t["windows_65_33"]["median"] / t["copy_encode_65_33"]["median"]
t["odd_over_aligned"] = t["windows_65_33"]["median"] / t["windows_64_32"]["median"]
t["source"] = [SW, SH]
res["b_pitched"] = t
del d_pitched, d_copy, o1, o2
torch.cuda.empty_cache()

# (c) tiling: one 16384^2 frame (4 x 4 of the frames), 1024 tiles of 512^2
if B >= 16:
    G, T = 16384, 512
    NT = (G // T) ** 2
    d_big = d_tight[:16].view(4, 4, H, W, 4).permute(0, 2, 1, 3, 4).reshape(G, G, 4).contiguous()
    big = himg_amd.src_desc(G, G, 4, frame_pitch=0)
    grid = np.int32([(x, y) for y in range(0, G, T) for x in range(0, G, T)])
    d_tiles = torch.empty((NT, T, T, 4), dtype=torch.uint8, device="cuda")
    o1, o2 = Out(NT, T, T), Out(NT, T, T)

    def copy_tiles():
        d_tiles.view(G // T, G // T, T, T, 4).copy_(d_big.view(G // T, T, G // T, T, 4).permute(0, 2, 1, 3, 4))

    def copy_encode_c():
        copy_tiles()
        enc_q(d_tiles, NT, T, T, o1)

    copy_tiles()
    t = timed({"windows": lambda: enc_w(d_big, big, grid, T, T, o2),
               "copy_encode": copy_encode_c,
               "encode_device_q_tiles_copied_before": lambda: enc_q(d_tiles, NT, T, T, o1)})
    enc_w(d_big, big, grid, T, T, o2)
    copy_encode_c()
    o1.same(o2)
    t["windows_over_copy_encode"] = t["windows"]["median"] / t["copy_encode"]["median"]
    t["windows_over_encode_q"] = t["windows"]["median"] / t["encode_device_q_tiles_copied_before"]["median"]
    t["frame"], t["tile"], t["tiles"] = [G, G], [T, T], NT
    res["c_tiling"] = t
    del d_big, d_tiles, o1, o2
    torch.cuda.empty_cache()

# (d) regions of interest
R = 256
rng = np.random.default_rng(20261019)
ORG = np.stack([rng.integers(0, W - R + 1, B), rng.integers(0, H - R + 1, B)], axis=1).astype(np.int32)
o1, o2 = Out(B, R, R), Out(B, R, R)
d_crop = torch.empty((B, R, R, 4), dtype=torch.uint8, device="cuda")
fi = torch.arange(B, device="cuda")[:, None, None]
yi = (torch.from_numpy(ORG[:, 1].astype(np.int64)).cuda()[:, None] + torch.arange(R, device="cuda"))[:, :, None]
xi = (torch.from_numpy(ORG[:, 0].astype(np.int64)).cuda()[:, None] + torch.arange(R, device="cuda"))[:, None, :]


def copy_encode_gather():
    d_crop.copy_(d_tight[fi, yi, xi])   # (advanced indexing: one gather kernel)
    enc_q(d_crop, B, R, R, o1)


def copy_encode_slices():
    torch.stack([d_tight[f, y:y + R, x:x + R] for f, (x, y) in enumerate(ORG)], out=d_crop)
    enc_q(d_crop, B, R, R, o1)


t = timed({"windows": lambda: enc_w(d_tight, tight, ORG, R, R, o2),
           "copy_encode_gather": copy_encode_gather, "copy_encode_slices": copy_encode_slices})
enc_w(d_tight, tight, ORG, R, R, o2)
copy_encode_slices()
o1.same(o2)
copy_encode_gather()
o1.same(o2)
best = min(("copy_encode_gather", "copy_encode_slices"), key=lambda k: t[k]["median"])
t["copy_encode_best"] = best
t["windows_over_copy_encode"] = t["windows"]["median"] / t[best]["median"]
t["window"], t["origins"] = [R, R], "seeded uniform (numpy default_rng(20261019))"
res["d_regions_of_interest"] = t

eng.close()
line = json.dumps(res)
print(line)
if os.environ.get("HIMG_WINDOWS_TIME_WRITE", "1") == "1":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "windows_time.json"), "w") as f:
        f.write(line + "\n")
