#!/usr/bin/env python3
"""Region decode against the full decode, one JSON line (GPU box), written to
profiles/region_time.json as well.
Batch: B x 4096^2 RGBA q50 randtile streams in HBM, decode_region_device for three rectangles
against decode_device, alternated in one process, device events after warm-up; the same at q90
(rows longer than k_row_count<true>'s LDS staging buffer) for two rectangles, in a batch and for a
single frame.
Single frame: one 16384^2 frame, decode_region_device of 1920 x 1080 windows (top-left, centre,
bottom-right) against decode_rows_device over the same block rows plus the crop copy; and
decode_region (host, pinned memory) against decode with the bytes each uploads.
The kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/region_time.py` run.
args: [batch] [iters] [big width]"""
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
WB = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
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
    for _ in range(it):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)} for k, v in ts.items()}


res = {"iters": it}


def batch_case(n, q, rects):
    """n x 4096^2 frames at quality q: region against the full decode, per rectangle."""
    w = h = 4096
    d_in, cap, sizes = encode(w, h, n, q)
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    d_pix = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    out = {"frames": n, "width": w, "height": h, "content": "randtile q%d RGBA" % q,
           "mean_row_payload_bytes": int(sizes.astype(np.int64).sum() // (n * ((h + 7) // 8)))}
    for rect in rects:
        x, y, rw, rh = rect
        d_reg = torch.empty((n, rh, rw, 4), dtype=torch.uint8, device="cuda")
        t = timed({"region": lambda: eng.decode_region_device(d_in, cap, sizes, n, w, h, 4, x, y, rw, rh, d_reg, d_st),
                   "decode": lambda: eng.decode_device(d_in, cap, sizes, n, w, h, 4, d_pix, d_st)})
        assert not d_st.cpu().numpy().any()
        eng.decode_region_device(d_in, cap, sizes, n, w, h, 4, x, y, rw, rh, d_reg, d_st)
        eng.decode_device(d_in, cap, sizes, n, w, h, 4, d_pix, d_st)
        torch.cuda.synchronize()
        assert torch.equal(d_reg, d_pix[:, y:y + rh, x:x + rw]), rect
        t["ratio_median"] = t["region"]["median"] / t["decode"]["median"]
        out["%dx%d@%d,%d" % (rw, rh, x, y)] = t
        del d_reg
    del d_pix, d_in
    torch.cuda.empty_cache()
    return out


res["batch"] = batch_case(B, 50, [(1536, 1536, 1024, 1024), (1001, 1003, 256, 256), (0, 2048, 4096, 64)])
res["batch_q90"] = batch_case(B, 90, [(1001, 1003, 256, 256), (2047, 2047, 1, 1)])
res["single_4096_q90"] = batch_case(1, 90, [(1001, 1003, 256, 256), (2047, 2047, 1, 1)])
# ---- one large frame ----
w = h = WB
d_in, cap, sizes = encode(w, h, 1)
size = int(sizes[0])
d_st = torch.ones(1, dtype=torch.int32, device="cuda")
single = {"width": w, "height": h, "content": "randtile q50 RGBA", "stream_bytes": size}
rw, rh = 1920, 1080
for name, (x, y) in {"top_left": (0, 0), "centre": ((w - rw) // 2, (h - rh) // 2),
                     "bottom_right": (w - rw, h - rh)}.items():
    r0, r1 = y // 8, (y + rh + 7) // 8
    d_reg = torch.empty((rh, rw, 4), dtype=torch.uint8, device="cuda")
    d_rows = torch.empty((8 * (r1 - r0), w, 4), dtype=torch.uint8, device="cuda")
    d_crop = torch.empty((rh, rw, 4), dtype=torch.uint8, device="cuda")

    def rows_crop():
        eng.decode_rows_device(d_in, size, w, h, 4, r0, r1, d_rows, d_st)
        d_crop.copy_(d_rows[y - 8 * r0:y - 8 * r0 + rh, x:x + rw])

    t = timed({"region": lambda: eng.decode_region_device(d_in, cap, sizes, 1, w, h, 4, x, y, rw, rh, d_reg, d_st),
               "rows_plus_crop": rows_crop})
    torch.cuda.synchronize()
    assert d_st[0].item() == 0 and torch.equal(d_reg, d_crop), name
    t["ratio_median"] = t["region"]["median"] / t["rows_plus_crop"]["median"]
    t["rect"] = [x, y, rw, rh]
    single[name] = t
    del d_rows
# host path: pinned stream, region_to vs decode_to
p = himg_amd.pinned_empty(size)
p[:] = d_in[0, :size].cpu().numpy()
out_r = himg_amd.pinned_empty(rw * rh * 4)
out_f = himg_amd.pinned_empty(w * h * 4)
x, y = (w - rw) // 2, (h - rh) // 2
plan = himg_amd.region_peek(p, x, y, rw, rh)
host = {"region_to": [], "decode_to": []}
for k in range(max(2, it // 3) + 1):
    for name, fn in (("region_to", lambda: eng.decode_region(p, x, y, rw, rh, out_r)),
                     ("decode_to", lambda: eng.decode(p, out_f))):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if k:
            host[name].append((t1 - t0) * 1e3)
assert np.array_equal(eng.decode_region(p, x, y, rw, rh), eng.decode(p)[y:y + rh, x:x + rw])
single["host_centre_ms"] = {k: {"min": min(v), "median": float(np.median(v))} for k, v in host.items()}
single["host_bytes_uploaded_region"] = int(plan["head_bytes"] + plan["rows_end"] - plan["rows_begin"])
single["host_bytes_uploaded_decode"] = size
res["single"] = single
eng.close()
line = json.dumps(res)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
if os.environ.get("HIMG_REGION_TIME_WRITE", "1") == "1":
    with open(os.path.join(ROOT, "profiles", "region_time.json"), "w") as f:
        f.write(line + "\n")
