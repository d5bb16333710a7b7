#!/usr/bin/env python3
"""Many windows of one stream (decode_stream_regions_device) against the calls that give the same bytes without
it, one JSON line (GPU box), written to profiles/stream_regions_time.json as well.  The variants of a case are
alternated in one process, device events after warm-up, medians of `iters` (7) with min and max.
Cases:
  a  one 16384^2 RGBA q50 randtile stream, 64 windows of 256^2 at seeded random origins in one call, against 64
     decode_region_device calls back to back (this commit, and -- with --compare TREE, a built checkout of the
     parent commit, alternated in child processes -- the parent) and against one decode_regions_device call over
     64 copies of the stream
  b  the same stream, 16 windows of 1920 x 1080
  c  B x 4096^2 q50, eight 256^2 windows per stream, against eight decode_regions_device calls
  d  the identity map (a window per stream) against decode_regions_device
  e  64 windows in the same block rows against 64 windows in disjoint rows of the 16384^2 stream, with the stage timer
  f  (--compare) decode_device alone (tools/prefix_time.py's child) and bench.py's headline at both trees
child: --calls-only TREE big iters   (one JSON line: the 64 decode_region_device calls with TREE's package)
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
ap.add_argument("--calls-only", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.calls_only) if args.calls_only else ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B, it, BIG = args.batch, args.iters, args.big
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
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fns[k](); e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)} for k, v in ts.items()}


def random_origins(rng, n, W, H, w, h):
    return np.stack([rng.integers(0, W - w + 1, n), rng.integers(0, H - h + 1, n)], 1).astype(np.int32)


def region_calls(d_in, cap, sizes, W, H, org, w, h, out, d_st):
    """A decode_region_device call per window, back to back."""
    def fn():
        for k, (x, y) in enumerate(org):
            eng.decode_region_device(d_in, cap, sizes[:1], 1, W, H, 4, int(x), int(y), w, h, out[k], d_st[k:k + 1])
    return fn


def stages(fn):
    eng.profile(True)
    fn(); torch.cuda.synchronize()
    eng.profile_reset()
    fn(); torch.cuda.synchronize()
    p = eng.profile_read()
    eng.profile(False)
    return {k: round(v[0], 4) for k, v in p.items()}


def one_stream(d_in, cap, sizes, W, H, org, w, h, expanded):
    n = len(org)
    so = np.zeros(n, np.int32)
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    ref = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    fns = {"stream_regions": lambda: eng.decode_stream_regions_device(d_in, cap, sizes[:1], 1, W, H, 4, so, org, w, h, out, d_st),
           "region_calls": region_calls(d_in, cap, sizes, W, H, org, w, h, ref, d_st)}
    if expanded:
        stride = (int(sizes[0]) + 255) // 256 * 256
        copies = d_in[0, :stride].repeat(n, 1).contiguous()
        exp = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
        fns["regions_device_over_copies"] = lambda: eng.decode_regions_device(copies, stride, np.full(n, sizes[0], np.uint32),
                                                                            n, W, H, 4, org, w, h, exp, d_st)
    t = timed(fns)
    assert not d_st.cpu().numpy().any() and torch.equal(out, ref)   # the same bytes
    if expanded:
        assert torch.equal(out, exp)
        t["regions_device_over_copies"]["bytes_of_copies"] = int(stride) * n
    t["windows"], t["window"] = n, [w, h]
    t["stream_regions"]["ratio_to_calls"] = t["stream_regions"]["median"] / t["region_calls"]["median"]
    t["stages_stream_regions"] = stages(fns["stream_regions"])
    return t


if args.calls_only:
    d_in, cap, sizes = encode(BIG, BIG, 1)
    org = random_origins(np.random.default_rng(41), 64, BIG, BIG, 256, 256)
    out = torch.empty((64, 256, 256, 4), dtype=torch.uint8, device="cuda")
    d_st = torch.ones(64, dtype=torch.int32, device="cuda")
    t = timed({"region_calls": region_calls(d_in, cap, sizes, BIG, BIG, org, 256, 256, out, d_st)})
    assert not d_st.cpu().numpy().any()
    eng.close()
    print(json.dumps(t))
    sys.exit(0)


def write(r):
    print("measured: %s" % ", ".join(k for k in r if k[1:2] == "_"), file=sys.stderr, flush=True)
    line = json.dumps(r)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "stream_regions_time.json"), "w") as f:
        f.write(line + "\n")
    return line


res = {"iters": it, "content": "randtile q50 RGBA"}
d_in, cap, sizes = encode(BIG, BIG, 1)
res["big"] = {"width": BIG, "height": BIG, "packed_bytes": int(sizes[0])}
org_a = random_origins(np.random.default_rng(41), 64, BIG, BIG, 256, 256)
res["a_64_windows_256"] = one_stream(d_in, cap, sizes, BIG, BIG, org_a, 256, 256, expanded=True)
torch.cuda.empty_cache()
write(res)
res["b_16_windows_1080p"] = one_stream(d_in, cap, sizes, BIG, BIG, random_origins(np.random.default_rng(42), 16, BIG, BIG, 1920, 1080),
                                       1920, 1080, expanded=False)
write(res)
# e: the same block rows (x varies) against disjoint rows (64 bands of 256 pixel rows)
rng = np.random.default_rng(43)
same = np.stack([rng.integers(0, BIG - 255, 64), np.full(64, 8192)], 1).astype(np.int32)
disj = np.stack([rng.integers(0, BIG - 255, 64), 256 * np.arange(64)], 1).astype(np.int32)
e = {}
for name, org in (("same_rows", same), ("disjoint_rows", disj)):
    n = 64
    out = torch.empty((n, 256, 256, 4), dtype=torch.uint8, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    fn = lambda org=org, out=out, d_st=d_st: eng.decode_stream_regions_device(d_in, cap, sizes[:1], 1, BIG, BIG, 4,
                                                                              np.zeros(64, np.int32), org, 256, 256, out, d_st)
    e[name] = timed({"stream_regions": fn})["stream_regions"]
    e[name]["stages"] = stages(fn)
    e[name]["rows_counted"] = int(len({(int(y) // 8 + r) for _, y in org for r in range((int(y) % 8 + 256 + 7) // 8)}))
    assert not d_st.cpu().numpy().any()
res["e_same_rows_against_disjoint_rows"] = e
del d_in
torch.cuda.empty_cache()
write(res)

# c, d: a batch of 4096^2 streams
W = H = 4096
d_in, cap, sizes = encode(W, H, B)
rng = np.random.default_rng(44)
org8 = random_origins(rng, 8 * B, W, H, 256, 256)
so8 = np.repeat(np.arange(B, dtype=np.int32), 8)
out = torch.empty((8 * B, 256, 256, 4), dtype=torch.uint8, device="cuda")
ref = torch.empty((B, 8, 256, 256, 4), dtype=torch.uint8, device="cuda")
tmp = torch.empty((8, B, 256, 256, 4), dtype=torch.uint8, device="cuda")
d_st = torch.ones(8 * B, dtype=torch.int32, device="cuda")


def eight_calls():
    for j in range(8):
        eng.decode_regions_device(d_in, cap, sizes, B, W, H, 4, org8[j::8], 256, 256, tmp[j], d_st[:B])


t = timed({"stream_regions": lambda: eng.decode_stream_regions_device(d_in, cap, sizes, B, W, H, 4, so8, org8, 256, 256, out, d_st),
           "eight_regions_device_calls": eight_calls})
assert not d_st.cpu().numpy().any() and torch.equal(out.view(B, 8, 256, 256, 4), tmp.transpose(0, 1))
t["stream_regions"]["ratio"] = t["stream_regions"]["median"] / t["eight_regions_device_calls"]["median"]
t["streams"], t["windows"] = B, 8 * B
res["c_eight_windows_per_stream"] = t
org1, so1 = org8[::8].copy(), np.arange(B, dtype=np.int32)
t = timed({"stream_regions": lambda: eng.decode_stream_regions_device(d_in, cap, sizes, B, W, H, 4, so1, org1, 256, 256, out, d_st),
           "regions_device": lambda: eng.decode_regions_device(d_in, cap, sizes, B, W, H, 4, org1, 256, 256, tmp[0], d_st)})
assert not d_st.cpu().numpy().any() and torch.equal(out[:B], tmp[0])
t["stream_regions"]["overhead_ms"] = t["stream_regions"]["median"] - t["regions_device"]["median"]
res["d_identity_map"] = t
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

    def calls(tree):
        return run([sys.executable, os.path.abspath(__file__), "--calls-only", tree, "--big", str(BIG), "--iters", str(it)])["region_calls"]

    def decode(tree):
        return run([sys.executable, os.path.join(ROOT, "tools", "prefix_time.py"), "--decode-only", tree, str(B), str(it)])["decode_device"]

    def bench(tree):
        j = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "5"], cwd=tree)
        return {"value": j["value"], "unit": j.get("unit")}

    cmp_ = {k: {"this": [], "parent": []} for k in ("a_64_region_calls_ms", "decode_device_ms", "bench_headline")}
    res["this_commit_against_parent"] = cmp_
    for key, fn in (("a_64_region_calls_ms", calls), ("decode_device_ms", decode), ("bench_headline", bench)):
        for _ in range(2):
            for name, tree in (("this", ROOT), ("parent", compare)):
                cmp_[key][name].append(fn(tree))
                print("%s %s: %s" % (key, name, json.dumps(cmp_[key][name][-1])), file=sys.stderr, flush=True)
                write(res)
    p = float(np.median([x["median"] for x in cmp_["a_64_region_calls_ms"]["parent"]]))
    res["a_64_windows_256"]["stream_regions"]["ratio_to_calls_at_parent"] = res["a_64_windows_256"]["stream_regions"]["median"] / p

print(write(res))
