#!/usr/bin/env python3
"""Scaled windows on opened streams (OpenedStreams.scaled_regions_device) against the stateless alternatives, one
JSON line (GPU box), written to profiles/opened_scaled_time.json as well.  The alternatives are entry points the
parent commit has, with kernels this change leaves as they are (tools/asm_compare.py): decode_scaled_regions_device
over a batch with a stream copied per window, the same as n calls of batch 1, and -- at 1/8 scale --
preview_device plus a torch gather of the crops.
Per configuration, scale and iteration a fresh handle: open, the scaled call (cold rows), the same call again
(warm), the handle's own full-resolution call over the covered rectangles R^ (warm; where its output stays under
1 GiB); the stateless forms alternate with it in one process.  Per configuration a pan-and-zoom of ten calls, each
moved by 128 full-resolution pixels in x and y, that alternates full-resolution, 1/2- and 1/4-scale windows of
w x h samples, on a handle and stateless.  Device events after warm-up, medians of `iters` (7) with min and max.
Configurations (those of tools/opened_time.py):
  a  one 16384^2 RGBA q50 randtile stream, 64 windows of 256^2 samples at seeded random origins: scales 1, 2, 3
  b  the same stream, 16 windows of 1920 x 1080 samples: scales 1, 2
  c  B x 4096^2 q50, eight 256^2 windows per stream: scales 1, 2, 3
--compare TREE (a built checkout of the parent commit): decode_device alone (tools/prefix_time.py's child) and
bench.py's headline at both trees, alternated in child processes.
args: [--batch B] [--iters N] [--big W] [--compare TREE] [--bench-steps K]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--big", type=int, default=16384)
ap.add_argument("--compare", default=None)
ap.add_argument("--bench-steps", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B, it, BIG = args.batch, args.iters, args.big
eng = himg_amd.Engine(0)
PAN, STEP = 10, 128


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


def stat(v):
    return {"min": min(v), "median": float(np.median(v)), "max": max(v)}


def spread(s):
    return s["max"] - s["min"]


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def size_at(W, H, s):
    F = 1 << s
    return (W + F - 1) // F, (H + F - 1) // F


def copies(d_in, sizes, so):
    """A batch with a stream copied per window, at a stride that just covers the largest stream."""
    stride = (int(sizes.max()) + 64 + 255) // 256 * 256
    d = torch.zeros((len(so), stride), dtype=torch.uint8, device="cuda")
    for k, s in enumerate(so):
        d[k, :int(sizes[s])] = d_in[s, :int(sizes[s])]
    return d, stride, sizes[so].copy()


def rounds(passes):
    """Two warm-up rounds, then `it` kept ones; the order of the passes rotates."""
    for i in range(-2, it):
        k = i % len(passes)
        for p in passes[k:] + passes[:k]:
            p(i >= 0)


def scale_config(d_in, cap, sizes, n_streams, W, H, so, org, w, h, s, cp):
    """org: origins in the picture at scale 2^-s.  cp: copies() of the streams."""
    n, F = len(so), 1 << s
    d_cp, cp_stride, cp_sizes = cp
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    ref = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    d_st1 = torch.ones(1, dtype=torch.int32, device="cuda")
    up = s < 3 and n * (F * h) * (F * w) * 4 <= 1 << 30
    out_up = torch.empty((n, F * h, F * w, 4), dtype=torch.uint8, device="cuda") if up else None
    names = ["open", "cold", "warm"] + (["warm_full_resolution_over_R"] if up else [])
    names += ["preview_plus_crop"] if s == 3 else ["stateless_copies", "stateless_batch1_calls"]
    ts = {k: [] for k in names}
    if s == 3:
        cols, rows = size_at(W, H, 3)
        pv = torch.empty((n_streams, rows, cols, 4), dtype=torch.uint8, device="cuda")
        d_pst = torch.ones(n_streams, dtype=torch.int32, device="cuda")
        i_s = torch.from_numpy(so.astype(np.int64)).cuda()[:, None, None]
        i_y = (torch.from_numpy(org[:, 1].astype(np.int64)).cuda()[:, None] + torch.arange(h, device="cuda")[None, :])[:, :, None]
        i_x = (torch.from_numpy(org[:, 0].astype(np.int64)).cuda()[:, None] + torch.arange(w, device="cuda")[None, :])[:, None, :]

    def opened_pass(keep):
        e = [ev()]
        hd = eng.open_streams_device(d_in, cap, sizes, n_streams, W, H, 4)
        e.append(ev())
        hd.scaled_regions_device(s, so, org, w, h, out, d_st)
        e.append(ev())
        hd.scaled_regions_device(s, so, org, w, h, out, d_st)
        e.append(ev())
        if up:
            hd.regions_device(so, F * org, F * w, F * h, out_up, d_st)
            e.append(ev())
            hd.regions_device(so, F * org, F * w, F * h, out_up, d_st)
            e.append(ev())
        torch.cuda.synchronize()
        if keep:
            for k, name in enumerate(("open", "cold", "warm")):
                ts[name].append(e[k].elapsed_time(e[k + 1]))
            if up:
                ts["warm_full_resolution_over_R"].append(e[4].elapsed_time(e[5]))
        return hd

    def copies_pass(keep):
        a = ev()
        eng.decode_scaled_regions_device(d_cp, cp_stride, cp_sizes, n, W, H, 4, s, org, w, h, ref, d_st)
        b = ev()
        torch.cuda.synchronize()
        if keep:
            ts["stateless_copies"].append(a.elapsed_time(b))

    def batch1_pass(keep):
        a = ev()
        for k in range(n):
            eng.decode_scaled_regions_device(d_in[so[k]], cap, sizes[so[k]:so[k] + 1], 1, W, H, 4, s, org[k:k + 1], w, h, ref[k], d_st1)
        b = ev()
        torch.cuda.synchronize()
        if keep:
            ts["stateless_batch1_calls"].append(a.elapsed_time(b))

    def preview_pass(keep):
        a = ev()
        eng.preview_device(d_in, cap, sizes, n_streams, W, H, 4, pv, d_pst)
        ref.copy_(pv[i_s, i_y, i_x])
        b = ev()
        torch.cuda.synchronize()
        if keep:
            ts["preview_plus_crop"].append(a.elapsed_time(b))

    rounds([lambda keep: opened_pass(keep).close()] + ([preview_pass] if s == 3 else [copies_pass, batch1_pass]))
    # the same bytes, and the stages of a warm call
    hd = opened_pass(False)
    (preview_pass if s == 3 else copies_pass)(False)
    assert not d_st.cpu().numpy().any() and torch.equal(out, ref)
    eng.profile(True)
    eng.profile_reset()
    hd.scaled_regions_device(s, so, org, w, h, out, d_st)
    torch.cuda.synchronize()
    warm_stages = {k: round(v[0], 4) for k, v in eng.profile_read().items()}
    eng.profile_reset()
    (preview_pass if s == 3 else copies_pass)(False)
    stateless_stages = {k: round(v[0], 4) for k, v in eng.profile_read().items()}
    eng.profile(False)
    eng.profile_reset()
    info = hd.info()
    hd.close()
    t = {k: stat(v) for k, v in ts.items()}
    best = "preview_plus_crop" if s == 3 else min(("stateless_copies", "stateless_batch1_calls"), key=lambda k: t[k]["median"])
    # what a stateless call runs in front of its row kernel: the head a handle does not repeat
    head = sum(v for k, v in stateless_stages.items()
               if any(x in k for x in ("parse", "lres_", "walk", "set_index", "memset")) and "lres_preview" not in k)
    t.update(scale_log2=s, streams=n_streams, windows=n, window=[w, h], rows_counted=info["rows_counted"],
             stages_warm_call=warm_stages, stages_stateless_call=stateless_stages, best_stateless=best)
    t["open_plus_cold"] = {"median": t["open"]["median"] + t["cold"]["median"],
                           "ratio_to_best_stateless": (t["open"]["median"] + t["cold"]["median"]) / t[best]["median"]}
    t["warm"]["ratio_to_best_stateless"] = t["warm"]["median"] / t[best]["median"]
    t["warm_below_best_stateless_by_more_than_both_spreads"] = bool(
        t[best]["median"] - t["warm"]["median"] > spread(t["warm"]) + spread(t[best]))
    t["best_stateless_minus_its_head"] = t[best]["median"] - head
    t["warm_below_stateless_minus_its_head"] = bool(t["warm"]["median"] < t[best]["median"] - head)
    if up:
        t["warm"]["ratio_to_full_resolution_over_R"] = t["warm"]["median"] / t["warm_full_resolution_over_R"]["median"]
    return t


def pan_zoom(d_in, cap, sizes, n_streams, W, H, so, org0, w, h, cp):
    """Ten calls, call i at scale i % 3 (0: full resolution), its windows w x h samples at the full-resolution
    origins org0 + 128 i brought to the scale: neighbouring calls overlap in block rows."""
    n = len(so)
    d_cp, cp_stride, cp_sizes = cp
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    steps = []
    for i in range(1, PAN + 1):
        s = i % 3
        ow, oh = size_at(W, H, s)
        o = np.stack([np.minimum((org0[:, 0] + STEP * i) >> s, ow - w), np.minimum((org0[:, 1] + STEP * i) >> s, oh - h)], 1)
        steps.append((s, o.astype(np.int32)))
    ts = {"pan_zoom_opened": [], "pan_zoom_stateless": []}
    info = {}

    def opened_pass(keep):
        hd = eng.open_streams_device(d_in, cap, sizes, n_streams, W, H, 4)
        a = ev()
        for s, o in steps:
            if s:
                hd.scaled_regions_device(s, so, o, w, h, out, d_st)
            else:
                hd.regions_device(so, o, w, h, out, d_st)
        b = ev()
        torch.cuda.synchronize()
        if keep:
            ts["pan_zoom_opened"].append(a.elapsed_time(b))
            info.update(hd.info())
        hd.close()

    def stateless_pass(keep):
        a = ev()
        for s, o in steps:
            if s:
                eng.decode_scaled_regions_device(d_cp, cp_stride, cp_sizes, n, W, H, 4, s, o, w, h, out, d_st)
            else:
                eng.decode_stream_regions_device(d_in, cap, sizes, n_streams, W, H, 4, so, o, w, h, out, d_st)
        b = ev()
        torch.cuda.synchronize()
        if keep:
            ts["pan_zoom_stateless"].append(a.elapsed_time(b))

    rounds([opened_pass, stateless_pass])
    t = {k: stat(v) for k, v in ts.items()}
    t.update(calls=PAN, step=STEP, scales=[s for s, _ in steps], window=[w, h], rows_counted_after=info["rows_counted"])
    t["pan_zoom_opened"]["ratio_to_stateless"] = t["pan_zoom_opened"]["median"] / t["pan_zoom_stateless"]["median"]
    return t


def config(d_in, cap, sizes, n_streams, W, H, so, w, h, scales, seed):
    cp = copies(d_in, sizes, so)
    r = {}
    for s in scales:
        ow, oh = size_at(W, H, s)
        rng = np.random.default_rng(seed + s)
        org = np.stack([rng.integers(0, ow - w + 1, len(so)), rng.integers(0, oh - h + 1, len(so))], 1).astype(np.int32)
        r["scale_%d" % s] = scale_config(d_in, cap, sizes, n_streams, W, H, so, org, w, h, s, cp)
        print("measured: scale %d of %d windows %d x %d" % (s, len(so), w, h), file=sys.stderr, flush=True)
    ow, oh = size_at(W, H, 2)
    rng = np.random.default_rng(seed)
    org0 = np.stack([rng.integers(0, 4 * (ow - w) + 1, len(so)), rng.integers(0, 4 * (oh - h) + 1, len(so))], 1).astype(np.int32)
    r["pan_zoom"] = pan_zoom(d_in, cap, sizes, n_streams, W, H, so, org0, w, h, cp)
    return r


def write(r):
    line = json.dumps(r)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "opened_scaled_time.json"), "w") as f:
        f.write(line + "\n")
    return line


res = {"iters": it, "content": "randtile q50 RGBA"}
d_in, cap, sizes = encode(BIG, BIG, 1)
res["big"] = {"width": BIG, "height": BIG, "packed_bytes": int(sizes[0])}
res["a_64_windows_256"] = config(d_in, cap, sizes[:1], 1, BIG, BIG, np.zeros(64, np.int32), 256, 256, (1, 2, 3), 41)
write(res)
res["b_16_windows_1080p"] = config(d_in, cap, sizes[:1], 1, BIG, BIG, np.zeros(16, np.int32), 1920, 1080, (1, 2), 42)
del d_in
torch.cuda.empty_cache()
write(res)
W = H = 4096
d_in, cap, sizes = encode(W, H, B)
res["c_eight_windows_per_stream"] = config(d_in, cap, sizes, B, W, H, np.repeat(np.arange(B, dtype=np.int32), 8), 256, 256,
                                           (1, 2, 3), 44)
eng.close()
del d_in
torch.cuda.empty_cache()
write(res)

if args.compare:
    compare = os.path.abspath(args.compare)

    def run(cmd, cwd=None):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=cwd)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    def decode(tree):
        return run([sys.executable, os.path.join(ROOT, "tools", "prefix_time.py"), "--decode-only", tree, str(B), str(it)])["decode_device"]

    def bench(tree):
        j = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "5"], cwd=tree)
        return {"value": j["value"], "unit": j.get("unit")}

    cmp_ = {k: {"this": [], "parent": []} for k in ("decode_device_ms", "bench_headline")}
    res["this_commit_against_parent"] = cmp_
    for key, fn in (("decode_device_ms", decode), ("bench_headline", bench)):
        for _ in range(2):
            for name, tree in (("this", ROOT), ("parent", compare)):
                cmp_[key][name].append(fn(tree))
                print("%s %s: %s" % (key, name, json.dumps(cmp_[key][name][-1])), file=sys.stderr, flush=True)
                write(res)

print(write(res))
