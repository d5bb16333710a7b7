#!/usr/bin/env python3
"""Windows in many calls on opened streams (open_streams_device, OpenedStreams.regions_device) against
decode_stream_regions_device of the same windows, one JSON line (GPU box), written to profiles/opened_time.json
as well.  Per configuration and iteration a fresh handle: open, the first call (cold rows), the same call again
(warm), then a pan of ten calls each moved by 128 pixels in x and y; the stateless call and its pan alternate
with it in one process.  Device events after warm-up, medians of `iters` (7) with min and max.
Configurations (the stream-regions row of the README):
  a  one 16384^2 RGBA q50 randtile stream, 64 windows of 256^2 at seeded random origins
  b  the same stream, 16 windows of 1920 x 1080
  c  B x 4096^2 q50, eight 256^2 windows per stream
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


def config(d_in, cap, sizes, n_streams, W, H, so, org, w, h):
    n = len(so)
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    ref = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    pans = [np.stack([np.minimum(org[:, 0] + STEP * i, W - w), np.minimum(org[:, 1] + STEP * i, H - h)], 1).astype(np.int32)
            for i in range(1, PAN + 1)]
    ts = {k: [] for k in ("open", "cold", "warm", "pan_opened", "stateless", "pan_stateless")}
    info = {}

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stateless(o=org, dst=ref):
        eng.decode_stream_regions_device(d_in, cap, sizes, n_streams, W, H, 4, so, o, w, h, dst, d_st)

    def opened_pass(keep):
        e = [ev()]
        hd = eng.open_streams_device(d_in, cap, sizes, n_streams, W, H, 4)
        e.append(ev())
        hd.regions_device(so, org, w, h, out, d_st)
        e.append(ev())
        hd.regions_device(so, org, w, h, out, d_st)
        e.append(ev())
        for p in pans:
            hd.regions_device(so, p, w, h, out, d_st)
        e.append(ev())
        torch.cuda.synchronize()
        if keep:
            for k, name in enumerate(("open", "cold", "warm", "pan_opened")):
                ts[name].append(e[k].elapsed_time(e[k + 1]))
            info.update(hd.info())
        return hd

    def stateless_pass(keep):
        e = [ev()]
        stateless()
        e.append(ev())
        for p in pans:
            stateless(p)
        e.append(ev())
        torch.cuda.synchronize()
        if keep:
            ts["stateless"].append(e[0].elapsed_time(e[1]))
            ts["pan_stateless"].append(e[1].elapsed_time(e[2]))

    for i in range(-2, it):   # (two warm-up rounds; the order alternates)
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            if which == 0:
                opened_pass(i >= 0).close()
            else:
                stateless_pass(i >= 0)
    # the same bytes, and what is left of a warm call: its stages
    hd = opened_pass(False)
    hd.regions_device(so, org, w, h, out, d_st)
    stateless()
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any() and torch.equal(out, ref)
    eng.profile(True)
    eng.profile_reset()
    hd.regions_device(so, org, w, h, out, d_st)
    torch.cuda.synchronize()
    warm_stages = {k: round(v[0], 4) for k, v in eng.profile_read().items()}
    eng.profile_reset()
    stateless()
    torch.cuda.synchronize()
    stateless_stages = {k: round(v[0], 4) for k, v in eng.profile_read().items()}
    eng.profile(False)
    hd.close()
    t = {k: stat(v) for k, v in ts.items()}
    t.update(streams=n_streams, windows=n, window=[w, h], pan_calls=PAN, pan_step=STEP,
             device_bytes=info["device_bytes"], rows_counted_after_pan=info["rows_counted"],
             stages_warm_call=warm_stages, stages_stateless_call=stateless_stages)
    t["open_plus_cold"] = {"median": t["open"]["median"] + t["cold"]["median"],
                           "ratio_to_stateless": (t["open"]["median"] + t["cold"]["median"]) / t["stateless"]["median"]}
    t["warm"]["ratio_to_stateless"] = t["warm"]["median"] / t["stateless"]["median"]
    t["pan_opened"]["ratio_to_stateless"] = t["pan_opened"]["median"] / t["pan_stateless"]["median"]
    t["warm_below_stateless_by_more_than_both_spreads"] = bool(
        t["stateless"]["median"] - t["warm"]["median"] > spread(t["warm"]) + spread(t["stateless"]))
    return t


def random_origins(rng, n, W, H, w, h):
    return np.stack([rng.integers(0, W - w + 1, n), rng.integers(0, H - h + 1, n)], 1).astype(np.int32)


def write(r):
    print("measured: %s" % ", ".join(k for k in r if k[1:2] == "_"), file=sys.stderr, flush=True)
    line = json.dumps(r)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "opened_time.json"), "w") as f:
        f.write(line + "\n")
    return line


res = {"iters": it, "content": "randtile q50 RGBA"}
d_in, cap, sizes = encode(BIG, BIG, 1)
res["big"] = {"width": BIG, "height": BIG, "packed_bytes": int(sizes[0])}
res["a_64_windows_256"] = config(d_in, cap, sizes[:1], 1, BIG, BIG, np.zeros(64, np.int32),
                                 random_origins(np.random.default_rng(41), 64, BIG, BIG, 256, 256), 256, 256)
write(res)
res["b_16_windows_1080p"] = config(d_in, cap, sizes[:1], 1, BIG, BIG, np.zeros(16, np.int32),
                                   random_origins(np.random.default_rng(42), 16, BIG, BIG, 1920, 1080), 1920, 1080)
del d_in
torch.cuda.empty_cache()
write(res)
W = H = 4096
d_in, cap, sizes = encode(W, H, B)
res["c_eight_windows_per_stream"] = config(d_in, cap, sizes, B, W, H, np.repeat(np.arange(B, dtype=np.int32), 8),
                                           random_origins(np.random.default_rng(44), 8 * B, W, H, 256, 256), 256, 256)
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
