#!/usr/bin/env python3
"""The planes decode against the full decode, one JSON line (GPU box), written to
profiles/planes_time.json as well (or to --out).
Workload: B x 4096^2 RGBA randtile at q50 in HBM, and one 16384^2 frame.  Variants, alternated in one
process (rotated order), device events after warm-up, medians of `iters` (>= 7) with min and max:
decode_device; decode_planes_device with masks 0x1 (luma), 0x8 (alpha), 0x7 (planar YCbCr) and 0xF (all
planes); and, for alpha, the only exact alternative without the planes decode: decode_device followed
by a torch copy of channel 3 (two ways to write that copy; the faster one counts).
The profiler's stage times of decode_device and of mask 0x1 (one profiled call each, behind the timed
ones) give the store kernel's own time.
--parent ROOT: a checkout of the parent commit, built.  decode_device (this script with --decode-only
--root) and the bench.py headline are then run in child processes, ROOT and this tree alternated,
`rounds` times, to show that they stand where they were.
args: [--batch B] [--iters N] [--big W] [--no-write] [--out PATH] [--parent ROOT] [--rounds R]
      [--decode-only] [--root ROOT]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--iters", type=int, default=9)
ap.add_argument("--big", type=int, default=16384)
ap.add_argument("--no-write", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "planes_time.json"))
ap.add_argument("--parent", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=5)
ap.add_argument("--decode-only", action="store_true")
ap.add_argument("--root", default=HERE)
args = ap.parse_args()
assert args.iters >= 7
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B, it = args.batch, args.iters
eng = himg_amd.Engine(0)
MASKS = (0x1, 0x8, 0x7, 0xF)


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


def stages(fn):
    eng.profile(True)
    eng.profile_reset()
    fn()
    torch.cuda.synchronize()
    out = {k: round(ms, 4) for k, (ms, _) in eng.profile_read().items()}
    eng.profile(False)
    return out


def case(w, h, n, planes):
    d_in, cap, sizes = encode(w, h, n)
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    d_pix = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    fns = {"decode_device": lambda: eng.decode_device(d_in, cap, sizes, n, w, h, 4, d_pix, d_st)}
    res = {"frames": n, "width": w, "height": h, "packed_bytes": int(sizes.sum())}
    if planes:
        d_pl = torch.empty((n, 4, h, w), dtype=torch.uint8, device="cuda")
        d_a = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        pix32 = d_pix.view(torch.int32).view(n, h, w)
        for m in MASKS:
            fns["planes_%#x" % m] = lambda m=m: eng.decode_planes_device(d_in, cap, sizes, n, w, h, 4, m, d_pl, d_st)

        def alpha_strided():
            eng.decode_device(d_in, cap, sizes, n, w, h, 4, d_pix, d_st)
            d_a.copy_(d_pix[:, :, :, 3])

        def alpha_shift():
            eng.decode_device(d_in, cap, sizes, n, w, h, 4, d_pix, d_st)
            d_a.copy_(pix32 >> 24)

        fns["decode_device_then_alpha_strided_copy"] = alpha_strided
        fns["decode_device_then_alpha_shift_copy"] = alpha_shift
        # what is timed is what is checked: the planes through the colour inverse are decode_device's picture
        eng.decode_device(d_in, cap, sizes, n, w, h, 4, d_pix, d_st)
        eng.decode_planes_device(d_in, cap, sizes, n, w, h, 4, 0x8, d_pl, d_st)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any() and torch.equal(d_pl.view(-1)[:n * h * w].view(n, h, w), d_pix[:, :, :, 3])
    res["ms"] = timed(fns)
    assert not d_st.cpu().numpy().any()
    if planes:
        res["stage_ms"] = {"decode_device": stages(fns["decode_device"]), "planes_0x1": stages(fns["planes_0x1"]),
                           "planes_0xf": stages(fns["planes_0xf"])}
        base = res["ms"]["decode_device"]
        res["spread_ms_decode_device"] = round(base["max"] - base["min"], 4)
        for m in MASKS:
            v = res["ms"]["planes_%#x" % m]
            res["planes_%#x_faster_beyond_spread" % m] = bool(
                base["median"] - v["median"] > max(base["max"] - base["min"], v["max"] - v["min"]))
    return res


def child(root, argv):
    r = subprocess.run([sys.executable] + argv, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert r.returncode == 0, (root, argv, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


if args.decode_only:
    print(json.dumps(case(4096, 4096, B, False)["ms"]["decode_device"]), flush=True)
    sys.exit(0)

out = {"iters": it, "batch_4096": case(4096, 4096, B, True)}
torch.cuda.empty_cache()
out["one_%d" % args.big] = case(args.big, args.big, 1, True)
if args.parent:
    eng.close()
    torch.cuda.empty_cache()
    me = os.path.abspath(__file__)
    runs = {"parent": {"decode_device_ms": [], "bench": []}, "this": {"decode_device_ms": [], "bench": []}}
    for _ in range(args.rounds):
        for name, root in (("parent", os.path.abspath(args.parent)), ("this", HERE)):
            d = child(root, [me, "--decode-only", "--root", root, "--batch", str(B), "--iters", str(it)])
            runs[name]["decode_device_ms"].append(d["median"])
            b = child(root, ["bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "2"])
            runs[name]["bench"].append(b["value"])
    out["parent_baseline"] = {"rounds": args.rounds, "bench_steps": args.bench_steps, **runs}
print(json.dumps(out), flush=True)
if not args.no_write:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
