#!/usr/bin/env python3
"""Region decode with a window per frame, one JSON line (GPU box), written to
profiles/regions_time.json as well.
M1 / M2: B x 4096^2 RGBA randtile streams in HBM at q50 / q90: decode_regions_device with 256^2
windows at seeded per-frame origins, against the same batch with every origin at (1001, 1003)
through decode_region_device, and against decode_device -- alternated in one process, device
events after warm-up, medians.
M3: 64 of the q50 streams in pinned host memory, 256^2 windows at per-frame origins:
decode_regions (himg_hip_decode_regions_batch) against a loop of decode_region calls and against
decode_batch followed by the crops, with the bytes each uploads (host wall clock).
The kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/regions_time.py 128 3 m1` run (M1 only).
args: [batch] [iters] [m1]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
it = int(sys.argv[2]) if len(sys.argv) > 2 else 10
M1_ONLY = len(sys.argv) > 3 and sys.argv[3] == "m1"
NH = 64   # M3's frames
W = H = 4096
RW = RH = 256
eng = himg_amd.Engine(0)


def encode(n, q):
    cap = himg_amd.max_packed_size(W, H, 4)
    d_out = torch.empty((n, cap), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    for s0 in range(0, n, 16):
        k = min(16, n - s0)
        d_frames = torch.from_numpy(np.stack([himg_amd.synth("randtile", s, W, H) for s in range(s0, s0 + k)])).cuda()
        eng.encode_device(d_frames, k, W, H, 4, 4, q, True, d_out[s0:], cap, d_sizes[s0:], d_st[s0:])
        torch.cuda.synchronize()
        del d_frames
    assert not d_st.cpu().numpy().any()
    return d_out, cap, d_sizes.cpu().numpy().astype(np.uint32)


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


rng = np.random.default_rng(20261016)
ORG = np.stack([rng.integers(0, W - RW + 1, B), rng.integers(0, H - RH + 1, B)], axis=1).astype(np.int32)
res = {"iters": it, "frames": B, "window": [RW, RH], "origins": "seeded uniform (numpy default_rng(20261016))"}


def batch_case(q, d_in, cap, sizes):
    d_st = torch.ones(B, dtype=torch.int32, device="cuda")
    d_reg = torch.empty((B, RH, RW, 4), dtype=torch.uint8, device="cuda")
    d_one = torch.empty((B, RH, RW, 4), dtype=torch.uint8, device="cuda")
    d_pix = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
    out = {"content": "randtile q%d RGBA" % q, "width": W, "height": H,
           "touched_rows_per_frame": [int(v) for v in np.unique((ORG[:, 1] + RH + 7) // 8 - ORG[:, 1] // 8)],
           "touched_tiles_per_frame": [int(v) for v in np.unique((ORG[:, 0] + RW + 7) // 8 - ORG[:, 0] // 8)]}
    t = timed({"regions_per_frame": lambda: eng.decode_regions_device(d_in, cap, sizes, B, W, H, 4, ORG, RW, RH, d_reg, d_st),
               "region_one_origin": lambda: eng.decode_region_device(d_in, cap, sizes, B, W, H, 4, 1001, 1003, RW, RH, d_one, d_st),
               "decode": lambda: eng.decode_device(d_in, cap, sizes, B, W, H, 4, d_pix, d_st)})
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    eng.decode_regions_device(d_in, cap, sizes, B, W, H, 4, ORG, RW, RH, d_reg, d_st)
    eng.decode_device(d_in, cap, sizes, B, W, H, 4, d_pix, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    for f, (x, y) in enumerate(ORG):
        assert torch.equal(d_reg[f], d_pix[f, y:y + RH, x:x + RW]), f
    t["per_frame_over_one_origin"] = t["regions_per_frame"]["median"] / t["region_one_origin"]["median"]
    t["per_frame_over_decode"] = t["regions_per_frame"]["median"] / t["decode"]["median"]
    out.update(t)
    return out


d_in, cap, sizes = encode(B, 50)
res["M1_q50"] = batch_case(50, d_in, cap, sizes)
if not M1_ONLY:
    # M3: pinned host streams (the first NH q50 frames)
    ps = [himg_amd.pinned_empty(int(sizes[i])) for i in range(NH)]
    for i in range(NH):
        ps[i][:] = d_in[i, :int(sizes[i])].cpu().numpy()
    rects = [(int(x), int(y), RW, RH) for x, y in ORG[:NH]]
    outs_r = [himg_amd.pinned_empty(RW * RH * 4) for _ in range(NH)]
    outs_f = [np.empty(W * H * 4, np.uint8) for _ in range(NH)]

    def loop_region_to():
        return [eng.decode_region(ps[i], *rects[i], out=outs_r[i]) for i in range(NH)]

    def batch_then_crop():
        full = eng.decode_batch(ps, outs=outs_f)
        return [np.ascontiguousarray(full[i][y:y + RH, x:x + RW]) for i, (x, y, _, _) in enumerate(rects)]

    fns = {"regions_batch": lambda: eng.decode_regions(ps, rects, outs=outs_r),
           "region_to_loop": loop_region_to, "decode_batch_then_crop": batch_then_crop}
    want = batch_then_crop()
    got = eng.decode_regions(ps, rects)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    host = {k: [] for k in fns}
    for k in range(it + 1):
        for name, fn in fns.items():
            t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
            if k:
                host[name].append((t1 - t0) * 1e3)
    m3 = {"frames": NH, "content": "randtile q50 RGBA, pinned host memory", "window": [RW, RH]}
    m3.update({k: stats(v) for k, v in host.items()})
    plans = [himg_amd.region_peek(ps[i], *rects[i]) for i in range(NH)]
    up = int(sum(p["head_bytes"] + p["rows_end"] - p["rows_begin"] for p in plans))
    m3["bytes_uploaded"] = {"regions_batch": up, "region_to_loop": up,
                            "decode_batch_then_crop": int(sizes[:NH].astype(np.int64).sum())}
    res["M3_host_q50"] = m3
    del ps, outs_f
    del d_in
    torch.cuda.empty_cache()
    d_in, cap, sizes = encode(B, 90)
    res["M2_q90"] = batch_case(90, d_in, cap, sizes)
eng.close()
line = json.dumps(res)
print(line)
if os.environ.get("HIMG_REGIONS_TIME_WRITE", "1") == "1" and not M1_ONLY:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "regions_time.json"), "w") as f:
        f.write(line + "\n")
