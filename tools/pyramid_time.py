#!/usr/bin/env python3
"""The pyramid decode against the calls it replaces, one JSON line (GPU box), written to
profiles/pyramid_time.json as well.  B RGBA randtile streams of 4096^2 in HBM, q50 (encoded on the device
beforehand).  decode_pyramid_device with all four levels, the four existing calls back to back
(decode_device, decode_scaled_device at 1 and at 2, preview_device), decode_device alone, the subsets
{0, 1} and {1, 2}, and every single call a one-level pyramid stands in for: alternated in one process,
device events after warm-up, medians with min - max.  The pyramid's levels are compared with the four
calls' outputs, byte for byte.  The same for one 16384^2 frame (a 4096^2 randtile picture tiled 4 x 4).

The condition the feature has to meet: the four-level pyramid's median is below the four calls' median
by more than the larger of the two spreads (max - min over the repetitions).

--compare TREE: decode_device alone, and bench.py's headline, at this tree and at the tree in TREE (a
checkout of the parent commit, built), alternated in child processes: whether the new forms have leaked
into the existing kernels.

args: [batch] [iters] [--compare TREE] [--bench-steps K] [--no-large]
child: --decode-only TREE batch iters   (one JSON line: decode_device's times with TREE's package)"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
child_tree = None
if argv and argv[0] == "--decode-only":
    child_tree = os.path.abspath(argv[1])
    argv = argv[2:]
compare = None
bench_steps = 20
large = True
while "--compare" in argv:
    i = argv.index("--compare")
    compare = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
while "--bench-steps" in argv:
    i = argv.index("--bench-steps")
    bench_steps = int(argv[i + 1])
    del argv[i:i + 2]
while "--no-large" in argv:
    argv.remove("--no-large")
    large = False
sys.path.insert(0, child_tree or ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B = int(argv[0]) if len(argv) > 0 else 128
it = int(argv[1]) if len(argv) > 1 else 7
Q = 50
STORE_FLOOR_MS = 0.57   # 21/64 of 128 x 4096^2 x 4 bytes at the measured 4.96 TB/s write ceiling


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


def dims(W, H, k):
    f = 1 << k
    return (H + f - 1) // f, (W + f - 1) // f


def workload(eng, n, W, H, d_frames):
    """The streams of d_frames ([n][H][W][4]) in HBM: (d_in, stride, sizes)."""
    stride = (himg_amd.max_packed_size(W, H, 4) + 255) // 256 * 256
    d_in = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    d_sz = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    eng.encode_device(d_frames, n, W, H, 4, 4, Q, True, d_in, stride, d_sz, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    return d_in, stride, d_sz.cpu().numpy().astype(np.uint32)


def measure(eng, n, W, H, d_in, stride, sizes, d_full):
    """Every configuration on one workload; d_full: a [n][H][W][4] buffer for level 0."""
    own = {0: d_full}    # the existing calls' outputs
    pyr = {0: torch.empty_like(d_full)}
    for k in (1, 2, 3):
        oh, ow = dims(W, H, k)
        own[k] = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
        pyr[k] = torch.empty_like(own[k])
    st = torch.ones(n, dtype=torch.int32, device="cuda")
    st2 = torch.ones(n, dtype=torch.int32, device="cuda")

    def call(k):
        if k == 0:
            eng.decode_device(d_in, stride, sizes, n, W, H, 4, own[0], st)
        elif k == 3:
            eng.preview_device(d_in, stride, sizes, n, W, H, 4, own[3], st)
        else:
            eng.decode_scaled_device(d_in, stride, sizes, n, W, H, 4, k, own[k], st)

    def calls(levels):
        for k in levels:
            call(k)

    def pyramid(levels):
        desc = himg_amd.pyramid_desc(*[pyr[k] if k in levels else None for k in range(4)])
        eng.decode_pyramid_device(d_in, stride, sizes, n, W, H, 4, desc, st2)

    sets = {"0123": (0, 1, 2, 3), "01": (0, 1), "12": (1, 2), "1": (1,), "2": (2,), "3": (3,)}
    fns = {"decode_device": lambda: call(0)}
    for name, lv in sets.items():
        fns["pyramid_" + name] = lambda lv=lv: pyramid(lv)
        fns["calls_" + name] = lambda lv=lv: calls(lv)
    t = timed(fns)
    # the outputs: every level of the pyramid is its own entry point's, byte for byte
    calls((0, 1, 2, 3))
    pyramid((0, 1, 2, 3))
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not st2.cpu().numpy().any()
    for k in range(4):
        assert torch.equal(own[k], pyr[k]), "level %d differs from its own entry point" % k
    res = {"times_ms": t}
    p, c = t["pyramid_0123"], t["calls_0123"]
    margin = max(p["max"] - p["min"], c["max"] - c["min"])
    res["condition"] = {"pyramid_median_ms": p["median"], "four_calls_median_ms": c["median"],
                        "saved_ms": c["median"] - p["median"], "larger_spread_ms": margin,
                        "met": bool(c["median"] - p["median"] > margin)}
    dd = t["decode_device"]["median"]
    res["pyramid_over_decode_device"] = p["median"] / dd
    res["pyramid_minus_decode_device_ms"] = p["median"] - dd
    res["pyramid_over_the_calls_it_replaces"] = {name: t["pyramid_" + name]["median"] / t["calls_" + name]["median"]
                                                 for name in sets}
    res["slower_than_the_calls_it_replaces"] = sorted(name for name, r in res["pyramid_over_the_calls_it_replaces"].items()
                                                      if r > 1.0)
    return res


eng = himg_amd.Engine(0)
W = H = 4096
with ThreadPoolExecutor(16) as pool:
    frames = list(pool.map(lambda s: himg_amd.synth("randtile", s, W, H), range(B)))
d_frames = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
for f, fr in enumerate(frames):
    d_frames[f] = torch.from_numpy(fr).cuda()
tile = torch.from_numpy(frames[0]).cuda()
del frames
d_in, stride, sizes = workload(eng, B, W, H, d_frames)
print("%d streams of %dx%d in HBM" % (B, W, H), file=sys.stderr, flush=True)

if child_tree:
    st = torch.ones(B, dtype=torch.int32, device="cuda")
    t = timed({"decode_device": lambda: eng.decode_device(d_in, stride, sizes, B, W, H, 4, d_frames, st)})
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    print(json.dumps({"tree": child_tree, "frames": B, "decode_device": t["decode_device"]}))
    eng.close()
    sys.exit(0)

res = {"iters": it, "frames": B, "content": "randtile q%d RGBA %dx%d" % (Q, W, H),
       "mean_stream_bytes": float(sizes.mean()), "store_floor_ms_128_frames": STORE_FLOOR_MS}
res.update(measure(eng, B, W, H, d_in, stride, sizes, d_frames))   # (the source pictures' buffer is reused)


def write(r):
    line = json.dumps(r)
    if os.environ.get("HIMG_PYRAMID_TIME_WRITE", "1") == "1":
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "pyramid_time.json"), "w") as f:
            f.write(line + "\n")
    return line


write(res)
print("128 frames: %s" % json.dumps(res["condition"]), file=sys.stderr, flush=True)
del d_frames, d_in
torch.cuda.empty_cache()
if large:
    W2 = H2 = 16384
    d_big = tile.repeat(H2 // H, W2 // W, 1).reshape(1, H2, W2, 4).contiguous()
    d_in2, stride2, sizes2 = workload(eng, 1, W2, H2, d_big)
    big = {"content": "one frame, randtile 4096^2 tiled 4 x 4, q%d RGBA %dx%d" % (Q, W2, H2), "stream_bytes": int(sizes2[0])}
    big.update(measure(eng, 1, W2, H2, d_in2, stride2, sizes2, d_big))
    res["one_frame_16384"] = big
    write(res)
    del d_big, d_in2
eng.close()
del tile
torch.cuda.empty_cache()

if compare:
    def child(tree):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--decode-only", tree, str(B), str(it)],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["decode_device"]

    def bench(tree):
        r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(bench_steps),
                            "--warmup", "5"], capture_output=True, text=True, timeout=1500, cwd=tree)
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        return {"value": j["value"], "unit": j.get("unit")}

    cmp_ = {"decode_device_ms": {"this": [], "parent": []}, "bench_headline": {"this": [], "parent": []}}
    res["this_commit_against_parent"] = cmp_
    for key, fn in (("decode_device_ms", child), ("bench_headline", bench)):
        for _ in range(2):
            for name, tree in (("this", ROOT), ("parent", compare)):
                cmp_[key][name].append(fn(tree))
                print("%s %s: %s" % (key, name, json.dumps(cmp_[key][name][-1])), file=sys.stderr, flush=True)
                write(res)

print(write(res))
