#!/usr/bin/env python3
"""The encode to a distortion target against what it is made of and against the parent ABI's way to the
same result, one JSON line (GPU box), written to profiles/target_time.json as well.
B x 4096^2 RGBA frames of bench.py's generator (randtile, seeds 0 .. B-1), quality range 0 .. 100, each
frame's target its own sse at quality 50:
  (a) encode_target_device                     (b) encode_sse_device at q50
  (c) the probe without this feature, through the parent's entry points: encode_device_q at q50, the
      sizes read back, decode_device with HIMG_OPT_FIX_T2 on, the squared difference in torch (exact:
      int32 difference, square in place, int64 sum) -- also timed without that comparison
      -- alternated in one process, device events after warm-up (plus encode_device_q at q50 alone)
  (d) per frame, the same search through the parent's entry points of batch 1 with the value read back
      after every probe, then the encode at the result.  Wall clock (the host round trips are the
      point), --serial-frames of the B frames, scaled to B.
The search's overhead: (a) against probes x (b) + encode.
--bench-parent FILE / --bench-this FILE: the output of `python bench.py --full ...` at the parent commit and
at this one (same session, alternated); the last JSON line of each goes into the record with the verdict
whether this one's value lies within the parent's per-step spread.
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
eng.set_option("fix_t2", 1)

d_frames = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
with ThreadPoolExecutor(16) as pool:
    for i, fr in enumerate(pool.map(lambda sd: himg_amd.synth("randtile", sd % 256, W, H), range(B))):
        d_frames[i].copy_(torch.from_numpy(fr))
cap = himg_amd.max_packed_size(W, H, 4)
d_out = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
d_pix = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
d_sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
d_st = torch.ones(B, dtype=torch.int32, device="cuda")
d_q = torch.zeros(B, dtype=torch.int32, device="cuda")
d_sse = torch.zeros(B, dtype=torch.int64, device="cuda")
d_ref = torch.zeros(B, dtype=torch.int64, device="cuda")
probes = himg_amd.budget_probes(QMIN, QMAX)
CH = 16   # frames per piece of the torch difference (its int32 temporary stays at 4 GiB)


def torch_sse(f0, f1, dst):
    """Exact, in four passes per piece: the difference in int32, its square in place, the sum in int64."""
    for a in range(f0, f1, CH):
        b = min(a + CH, f1)
        d = d_frames[a:b].to(torch.int32)
        d.sub_(d_pix[a:b])
        d.mul_(d)
        dst[a:b] = d.sum(dim=(1, 2, 3), dtype=torch.int64)


def parent_probe(f0, n, quals, compare=True):
    """sse of frames f0 .. f0 + n - 1 at `quals` by the parent's entry points, into d_ref."""
    eng.encode_device_q(d_frames[f0:], n, W, H, 4, 4, quals, True, d_out[f0:], cap, d_sizes[f0:], d_st[f0:])
    sizes = d_sizes[f0:f0 + n].cpu().numpy().astype(np.uint32)   # (synchronises: the decode takes them on the host)
    eng.decode_device(d_out[f0:], cap, sizes, n, W, H, 4, d_pix[f0:], d_st[f0:])
    if compare:
        torch_sse(f0, f0 + n, d_ref)


eng.encode_sse_device(d_frames, B, W, H, 4, 4, [50] * B, True, d_sse, d_st)
torch.cuda.synchronize()
assert not d_st.cpu().numpy().any()
targets = [int(x) for x in d_sse.cpu().numpy()]
parent_probe(0, B, [50] * B)
torch.cuda.synchronize()
assert [int(x) for x in d_ref.cpu().numpy()] == targets, "the probe and the parent's way disagree"

fns = {
    "target": lambda: eng.encode_target_device(d_frames, B, W, H, 4, 4, QMIN, QMAX, True, targets, d_out, cap, d_sizes,
                                               d_q, d_sse, d_st),
    "sse_q50": lambda: eng.encode_sse_device(d_frames, B, W, H, 4, 4, [50] * B, True, d_sse, d_st),
    "parent_probe_q50": lambda: parent_probe(0, B, [50] * B),
    "parent_encode_decode_q50": lambda: parent_probe(0, B, [50] * B, compare=False),   # ((c) without the comparison)
    "encode_q50": lambda: eng.encode_device_q(d_frames, B, W, H, 4, 4, [50] * B, True, d_out, cap, d_sizes, d_st),
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

# the stages of one probe
eng.profile(True)
eng.profile_reset()
fns["sse_q50"]()
torch.cuda.synchronize()
stages = {k: round(v[0] if isinstance(v, (tuple, list)) else float(v), 4) for k, v in eng.profile_read().items()}
eng.profile(False)


def eng_stage_ms(prefix):
    return sum(v for k, v in stages.items() if k.startswith(prefix))


fns["target"]()
torch.cuda.synchronize()
chosen = d_q.cpu().numpy().astype(int)
sse_a = [int(x) for x in d_sse.cpu().numpy()]
assert all(s <= t for s, t in zip(sse_a, targets)) and (chosen >= QMIN).all()


def serial_search(f):
    """Frame f by the parent's entry points: encode, decode and compare per probe, the value read back."""
    def sse_of(q):
        parent_probe(f, 1, [q])
        return int(d_ref[f].item())            # (synchronises: the next quality depends on it)
    t = targets[f]
    if sse_of(QMAX) > t:
        return -1
    if sse_of(QMIN) <= t:
        return QMIN                            # (the stream at qmin is the result: already written)
    lo, hi = QMIN, QMAX
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if sse_of(mid) <= t:
            hi = mid
        else:
            lo = mid
    eng.encode_device_q(d_frames[f:], 1, W, H, 4, 4, [hi], True, d_out[f:], cap, d_sizes[f:], d_st[f:])   # the stream that is kept
    return hi


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

a, b_, c, e = res["target"]["median"], res["sse_q50"]["median"], res["parent_probe_q50"]["median"], res["encode_q50"]["median"]
out = {
    "parent_commit": args.parent_commit, "frames": B, "width": W, "height": H, "content": "randtile RGBA, seeds 0..%d" % (B - 1),
    "quality_range": [QMIN, QMAX], "target": "each frame's own sse at quality 50", "probes": probes,
    "warmup": 2, "iters": it, "unit": "ms per %d frames" % B,
    "a_encode_target_device": res["target"], "b_encode_sse_device_q50": res["sse_q50"],
    "c_parent_probe_q50": res["parent_probe_q50"], "c_without_the_torch_comparison": res["parent_encode_decode_q50"],
    "encode_device_q_q50": res["encode_q50"],
    "d_parent_abi_search": {"frames_measured": K, "per_frame_ms": {"min": min(per_frame), "median": float(np.median(per_frame)),
                                                                    "max": max(per_frame)},
                            "scaled_to_batch_ms": serial_ms},
    "ratio_d_over_a": serial_ms / a,
    "b_over_c": b_ / c, "b_below_c": bool(b_ < c),
    "b_over_c_without_the_torch_comparison": b_ / res["parent_encode_decode_q50"]["median"],
    "k_sse_bytes_per_s": (2.0 * B * W * H * 4) / (1e-3 * eng_stage_ms("k_sse")) if eng_stage_ms("k_sse") else None,
    "search_overhead": {"probes_x_b_plus_encode_ms": probes * b_ + e, "a_over_that": a / (probes * b_ + e)},
    "probe_stages_ms": stages,
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
    with open(os.path.join(ROOT, "profiles", "target_time.json"), "w") as f:
        f.write(line + "\n")
