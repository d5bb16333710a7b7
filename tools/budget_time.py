#!/usr/bin/env python3
"""The encode to a byte budget against what it is made of and against the parent ABI's way to the same
result, one JSON line (GPU box), written to profiles/budget_time.json as well.
B x 4096^2 RGBA frames of bench.py's generator (randtile, seeds 0 .. B-1), quality range 0 .. 100, each
frame's budget its own size at quality 50:
  (a) encode_budget_device                     (b) encode_sizes_device at q50
  (c) encode_device at q50                     -- alternated in one process, device events after warm-up
  (d) per frame, the same bisection by encode_device calls of batch 1 with the size read back after each
      probe, then the encode at the result: what a caller of the parent commit's ABI has to do.  Wall clock
      (the host round trips are the point), --serial-frames of the B frames, scaled to B.
The search's overhead: (a) against probes x (b) + (c).
--bench-parent FILE / --bench-this FILE: the output of `python bench.py --full ...` at the parent commit and
at this one (same session); the last JSON line of each goes into the record with the verdict whether this
one's value lies within the parent's per-step spread.
args: [--batch B] [--iters N] [--serial-frames K] [--bench-parent FILE] [--bench-this FILE] [--parent-commit ID]
[--no-write]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--serial-frames", type=int, default=16)
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--bench-parent", default=None)
ap.add_argument("--bench-this", default=None)
ap.add_argument("--parent-commit", default="", help="recorded: the commit this change sits on")
ap.add_argument("--no-write", action="store_true")
args = ap.parse_args()
B, it, W, H = args.batch, args.iters, args.size, args.size
QMIN, QMAX = 0, 100
eng = himg_amd.Engine(0)

d_frames = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
with ThreadPoolExecutor(16) as pool:
    for i, fr in enumerate(pool.map(lambda sd: himg_amd.synth("randtile", sd % 256, W, H), range(B))):
        d_frames[i].copy_(torch.from_numpy(fr))
cap = himg_amd.max_packed_size(W, H, 4)
d_out = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
d_sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
d_st = torch.ones(B, dtype=torch.int32, device="cuda")
d_q = torch.zeros(B, dtype=torch.int32, device="cuda")

eng.encode_sizes_device(d_frames, B, W, H, 4, 4, [50] * B, True, d_sizes, d_st)
torch.cuda.synchronize()
assert not d_st.cpu().numpy().any()
budgets = [int(x) for x in d_sizes.cpu().numpy()]
probes = himg_amd.budget_probes(QMIN, QMAX)

fns = {
    "budget": lambda: eng.encode_budget_device(d_frames, B, W, H, 4, 4, QMIN, QMAX, True, budgets, d_out, cap, d_sizes,
                                               d_q, d_st),
    "sizes_q50": lambda: eng.encode_sizes_device(d_frames, B, W, H, 4, 4, [50] * B, True, d_sizes, d_st),
    "encode_q50": lambda: eng.encode_device(d_frames, B, W, H, 4, 4, 50, True, d_out, cap, d_sizes, d_st),
}
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
        assert not d_st.cpu().numpy().any(), k
res = {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)} for k, v in ts.items()}

# what the search chose (the last timed call of (a) ran before other encodes overwrote d_sizes: run it once more)
fns["budget"]()
torch.cuda.synchronize()
chosen = d_q.cpu().numpy().astype(int)
sizes_a = d_sizes.cpu().numpy().astype(np.int64)
assert (sizes_a <= np.array(budgets)).all() and (chosen >= QMIN).all()


def serial_search(f):
    """Frame f by the parent's ABI: encode_device of batch 1 per probe, the size read back each time."""
    def size_of(q):
        eng.encode_device(d_frames[f], 1, W, H, 4, 4, q, True, d_out[f], cap, d_sizes[f:], d_st[f:])
        return int(d_sizes[f].item())          # (synchronises: the next quality depends on it)
    b = budgets[f]
    if size_of(QMIN) > b:
        return -1
    if size_of(QMAX) <= b:
        return QMAX                            # (the stream at qmax is the result: already written)
    lo, hi = QMIN, QMAX
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if size_of(mid) <= b:
            lo = mid
        else:
            hi = mid
    size_of(lo)                                # the stream that is kept
    return lo


K = min(args.serial_frames, B)
serial_search(0)                               # warm-up
torch.cuda.synchronize()
per_frame = []
for f in range(K):
    t0 = time.perf_counter()
    q = serial_search(f)
    torch.cuda.synchronize()
    per_frame.append((time.perf_counter() - t0) * 1e3)
    assert q == chosen[f], (f, q, chosen[f])   # the same result both ways
serial_ms = float(np.sum(per_frame)) * B / K

a, b_, c = res["budget"]["median"], res["sizes_q50"]["median"], res["encode_q50"]["median"]
out = {
    "parent_commit": args.parent_commit, "frames": B, "width": W, "height": H, "content": "randtile RGBA, seeds 0..%d" % (B - 1),
    "quality_range": [QMIN, QMAX], "budget": "each frame's own size at quality 50", "probes": probes,
    "warmup": 2, "iters": it, "unit": "ms per %d frames" % B,
    "a_encode_budget_device": res["budget"], "b_encode_sizes_device_q50": res["sizes_q50"],
    "c_encode_device_q50": res["encode_q50"],
    "d_parent_abi_bisection": {"frames_measured": K, "per_frame_ms": {"min": min(per_frame), "median": float(np.median(per_frame)),
                                                                       "max": max(per_frame)},
                               "scaled_to_batch_ms": serial_ms},
    "ratio_d_over_a": serial_ms / a,
    "b_over_c": b_ / c, "c_minus_b_ms": c - b_,
    "search_overhead": {"probes_x_b_plus_c_ms": probes * b_ + c, "a_over_that": a / (probes * b_ + c)},
    "chosen_quality": {"min": int(chosen.min()), "median": float(np.median(chosen)), "max": int(chosen.max())},
}


def last_json_line(path):
    line = None
    for l in open(path):
        l = l.strip()
        if l.startswith("{") and l.endswith("}"):
            line = l
    return json.loads(line) if line else None


if args.bench_parent and args.bench_this:
    bp, bt = last_json_line(args.bench_parent), last_json_line(args.bench_this)
    out["bench_parent"], out["bench_this"] = bp, bt
    if bp and bt and "step_ms" in bp:
        # the parent's per-step spread as a spread of its value (the value is pixels per step time)
        lo = bp["value"] * bp["step_ms"]["mean"] / bp["step_ms"]["max"]
        hi = bp["value"] * bp["step_ms"]["mean"] / bp["step_ms"]["min"]
        out["bench_verdict"] = {"parent_value_spread": [round(lo, 2), round(hi, 2)], "this_value": bt["value"],
                                "within_spread_or_above": bool(bt["value"] >= lo)}
eng.close()
line = json.dumps(out)
print(line)
if not args.no_write:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "budget_time.json"), "w") as f:
        f.write(line + "\n")
