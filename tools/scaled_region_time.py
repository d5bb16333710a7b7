#!/usr/bin/env python3
"""The scaled region decode against the calls that give the same bytes without it, one JSON line
(GPU box), written to profiles/scaled_region_time.json as well (or to --out).
Baseline of every case: decode_scaled_device followed by a device crop (one gather kernel over the
batch), timed in the same process; the variants alternated, device events after warm-up, medians of
`iters` with min and max.
Cases: B x 4096^2 RGBA randtile at q50 and q90 in HBM, windows 256^2 and 1024 x 64 of the scaled
picture at per-frame origins, both scales, also against decode_regions_device of the covered
full-resolution rectangles; one 16384^2 frame, a 1920 x 1080 window at both scales, top-left, centre
and bottom-right; 64 pinned host streams through decode_scaled_regions (with the bytes uploaded)
against decode_scaled_batch; a whole-picture rectangle against decode_scaled_device alone.
The kernel times come from separate
`rocprofv3 --kernel-trace --stats -- python tools/scaled_region_time.py --profile VARIANT` runs, which
launch one variant alone (B x 4096^2 q50 at 1/2 scale): scaled, scaled_region_whole or scaled_region_256.
args: [--batch B] [--iters N] [--big W] [--only CASE] [--no-write] [--out PATH] [--profile VARIANT]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--big", type=int, default=16384)
ap.add_argument("--only", default=None)
ap.add_argument("--no-write", action="store_true")
ap.add_argument("--profile", default=None, choices=["scaled", "scaled_region_whole", "scaled_region_256"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_region_time.json"))
args = ap.parse_args()
B, it = args.batch, args.iters
eng = himg_amd.Engine(0)


def encode(w, h, n, q=50):
    cap = himg_amd.max_packed_size(w, h, 4)
    d_out = torch.empty((n, cap), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    for s0 in range(0, n, 16):
        k = min(16, n - s0)
        d_frames = torch.from_numpy(np.stack([himg_amd.synth("randtile", s, w, h) for s in range(s0, s0 + k)])).cuda()
        eng.encode_device(d_frames, k, w, h, 4, 4, q, True, d_out[s0:], cap, d_sizes[s0:], d_st[s0:])
        torch.cuda.synchronize()
        del d_frames
    assert not d_st.cpu().numpy().any()
    return d_out, cap, d_sizes.cpu().numpy().astype(np.uint32)


def timed(fns):
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    names = list(fns)
    for i in range(it):
        for k in names[i % len(names):] + names[:i % len(names)]:   # (rotated: no variant keeps a place in the order)
            fn = fns[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)} for k, v in ts.items()}


def crop_index(org, n, ow, oh, ww, wh):
    """Flat pixel indices (RGBA pixels as int32) of frame f's window at org[f] in n x oh x ow."""
    o = torch.from_numpy(np.asarray(org, np.int64)).cuda()
    f = torch.arange(n, device="cuda").view(n, 1, 1)
    y = o[:, 1].view(n, 1, 1) + torch.arange(wh, device="cuda").view(1, wh, 1)
    x = o[:, 0].view(n, 1, 1) + torch.arange(ww, device="cuda").view(1, 1, ww)
    return ((f * oh + y) * ow + x).reshape(-1)


def windows(d_in, cap, sizes, n, w, h, wins, with_regions, rng):
    """wins: (name, ww, wh, origin mode) of the scaled picture; returns {name_scale: timings}."""
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    res = {}
    for s in (1, 2):
        F = 1 << s
        ow, oh = himg_amd.scaled_size(w, h, s)
        full = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
        flat = full.view(torch.int32).reshape(-1)
        for name, ww, wh, mode in wins:
            if mode == "random":
                org = np.stack([rng.integers(0, ow - ww + 1, n), rng.integers(0, oh - wh + 1, n)], 1).astype(np.int32)
            elif mode == "top_left":
                org = np.zeros((n, 2), np.int32)
            elif mode == "centre":
                org = np.tile(np.array([(ow - ww) // 2, (oh - wh) // 2], np.int32), (n, 1))
            else:
                org = np.tile(np.array([ow - ww, oh - wh], np.int32), (n, 1))
            out = torch.empty((n, wh, ww, 4), dtype=torch.uint8, device="cuda")
            ref = torch.empty((n, wh, ww, 4), dtype=torch.uint8, device="cuda")
            idx = crop_index(org, n, ow, oh, ww, wh)
            ref32 = ref.view(torch.int32).reshape(-1)

            def base():
                eng.decode_scaled_device(d_in, cap, sizes, n, w, h, 4, s, full, d_st)
                torch.index_select(flat, 0, idx, out=ref32)

            fns = {"scaled_then_crop": base,
                   "scaled_region": lambda: eng.decode_scaled_regions_device(d_in, cap, sizes, n, w, h, 4, s, org, ww, wh,
                                                                             out, d_st)}
            if with_regions:   # the covered full-resolution rectangles (F times the samples per side)
                fw, fh = min(F * ww, w), min(F * wh, h)
                forg = np.minimum(F * org, np.array([w - fw, h - fh], np.int32)).astype(np.int32)
                fout = torch.empty((n, fh, fw, 4), dtype=torch.uint8, device="cuda")
                fns["regions_full_resolution"] = lambda: eng.decode_regions_device(d_in, cap, sizes, n, w, h, 4, forg, fw,
                                                                                   fh, fout, d_st)
            t = timed(fns)
            assert not d_st.cpu().numpy().any()
            fns["scaled_then_crop"](); fns["scaled_region"]()
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (name, s)   # the same bytes
            t["window"], t["origins"], t["scale"] = [ww, wh], mode, "1/%d" % F
            t["scaled_region"]["ratio_median"] = t["scaled_region"]["median"] / t["scaled_then_crop"]["median"]
            res["%s_1_%d" % (name, F)] = t
            del out, ref, idx
        del full, flat
        torch.cuda.empty_cache()
    return res


def batch_case(q, whole):
    n, w, h = B, 4096, 4096
    d_in, cap, sizes = encode(w, h, n, q)
    rng = np.random.default_rng(5)
    res = {"frames": n, "width": w, "height": h, "content": "randtile q%d RGBA" % q,
           "packed_bytes": int(sizes.astype(np.int64).sum())}
    res.update(windows(d_in, cap, sizes, n, w, h, [("256x256", 256, 256, "random"), ("1024x64", 1024, 64, "random")], True, rng))
    if whole:   # a whole-picture rectangle against decode_scaled_device alone
        d_st = torch.ones(n, dtype=torch.int32, device="cuda")
        for s in (1, 2):
            ow, oh = himg_amd.scaled_size(w, h, s)
            a = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
            b = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
            org = np.zeros((n, 2), np.int32)
            t = timed({"scaled": lambda: eng.decode_scaled_device(d_in, cap, sizes, n, w, h, 4, s, a, d_st),
                       "scaled_region_whole": lambda: eng.decode_scaled_regions_device(d_in, cap, sizes, n, w, h, 4, s,
                                                                                       org, ow, oh, b, d_st)})
            assert torch.equal(a, b) and not d_st.cpu().numpy().any()
            t["scaled_region_whole"]["ratio_median"] = t["scaled_region_whole"]["median"] / t["scaled"]["median"]
            res["whole_picture_1_%d" % (1 << s)] = t
            del a, b
            torch.cuda.empty_cache()
    return res, (d_in, cap, sizes)


def big_case():
    w = h = args.big
    d_in, cap, sizes = encode(w, h, 1, 50)
    res = {"frames": 1, "width": w, "height": h, "content": "randtile q50 RGBA", "packed_bytes": int(sizes[0])}
    rng = np.random.default_rng(6)
    res.update(windows(d_in, cap, sizes, 1, w, h, [("1920x1080_top_left", 1920, 1080, "top_left"),
                                                   ("1920x1080_centre", 1920, 1080, "centre"),
                                                   ("1920x1080_bottom_right", 1920, 1080, "bottom_right")], False, rng))
    return res


def host_case(enc, n=64, w=4096, h=4096):
    d_in, cap, sizes = enc
    n = min(n, len(sizes))
    streams = []
    for i in range(n):
        p = himg_amd.pinned_empty(int(sizes[i]))
        p[:] = d_in[i, :int(sizes[i])].cpu().numpy()
        streams.append(p)
    rng = np.random.default_rng(7)
    res = {"frames": n, "width": w, "height": h, "content": "randtile q50 RGBA, pinned host memory",
           "stream_bytes": int(sizes[:n].astype(np.int64).sum())}
    ww = wh = 256
    fns, up = {}, {}
    for s in (1, 2):
        ow, oh = himg_amd.scaled_size(w, h, s)
        rl = [(int(rng.integers(0, ow - ww + 1)), int(rng.integers(0, oh - wh + 1)), ww, wh) for _ in range(n)]
        plans = [himg_amd.scaled_region_peek(streams[i], s, *rl[i]) for i in range(n)]
        up[s] = sum(p["head_bytes"] + p["rows_end"] - p["rows_begin"] for p in plans)
        outs_r = [himg_amd.pinned_empty(ww * wh * 4) for _ in range(n)]
        outs_f = [himg_amd.pinned_empty(ow * oh * 4) for _ in range(n)]
        fns["decode_scaled_batch_1_%d" % (1 << s)] = (lambda s=s, o=outs_f: eng.decode_scaled_batch(streams, s, o))
        fns["decode_scaled_regions_1_%d" % (1 << s)] = (lambda s=s, o=outs_r, rl=rl: eng.decode_scaled_regions(streams, s, rl, o))
    ts = {k: [] for k in fns}
    for k in range(max(2, it // 3) + 1):
        for name, fn in fns.items():
            t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
            if k:
                ts[name].append((t1 - t0) * 1e3)
    for name, v in ts.items():
        res[name] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    for s in (1, 2):
        k = "decode_scaled_regions_1_%d" % (1 << s)
        res[k]["bytes_uploaded"] = int(up[s])
        res[k]["ratio_median"] = res[k]["median"] / res["decode_scaled_batch_1_%d" % (1 << s)]["median"]
    return res


if args.profile:
    n, w, h, s = B, 4096, 4096, 1
    d_in, cap, sizes = encode(w, h, n, 50)
    ow, oh = himg_amd.scaled_size(w, h, s)
    ww, wh = (256, 256) if args.profile == "scaled_region_256" else (ow, oh)
    out = torch.empty((n, wh, ww, 4), dtype=torch.uint8, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(5)
    org = np.stack([rng.integers(0, ow - ww + 1, n), rng.integers(0, oh - wh + 1, n)], 1).astype(np.int32)
    for _ in range(it + 2):
        if args.profile == "scaled":
            eng.decode_scaled_device(d_in, cap, sizes, n, w, h, 4, s, out, d_st)
        else:
            eng.decode_scaled_regions_device(d_in, cap, sizes, n, w, h, 4, s, org, ww, wh, out, d_st)
        torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    eng.close()
    sys.exit(0)

res = {"iters": it}
want = lambda name: not args.only or args.only == name
enc50 = None
if want("batch_q50") or want("host_batch_64"):
    r, enc50 = batch_case(50, whole=True)
    if want("batch_q50"):
        res["batch_q50"] = r
if want("host_batch_64"):
    res["host_batch_64"] = host_case(enc50)
del enc50
torch.cuda.empty_cache()
if want("batch_q90"):
    res["batch_q90"] = batch_case(90, whole=False)[0]
    torch.cuda.empty_cache()
if want("single_big"):
    res["single_big"] = big_case()
eng.close()
line = json.dumps(res)
print(line)
if not args.no_write and not args.only:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
