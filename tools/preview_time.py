#!/usr/bin/env python3
"""1/8-scale preview against the full decode, one JSON line (GPU box).
Device: B x W^2 RGBA q50 randtile streams in HBM, preview_device and decode_device alternated
in one process, timed with device events after warm-up.  Host: preview_batch and decode_batch
of the same streams from pinned memory, with the bytes each uploads.  The kernel times come
from a separate `rocprofv3 --kernel-trace --stats -- python tools/preview_time.py` run.
args: [width] [batch] [iters]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

w = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
B = int(sys.argv[2]) if len(sys.argv) > 2 else 128
it = int(sys.argv[3]) if len(sys.argv) > 3 else 10
h = w
eng = himg_amd.Engine(0)
cap = himg_amd.max_packed_size(w, h, 4)
d_out = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
d_sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
d_st = torch.ones(B, dtype=torch.int32, device="cuda")
for s0 in range(0, B, 16):   # encode in slices: B full frames do not need to sit in HBM at once
    n = min(16, B - s0)
    d_frames = torch.from_numpy(np.stack([himg_amd.synth("randtile", s, w, h) for s in range(s0, s0 + n)])).cuda()
    eng.encode_device(d_frames, n, w, h, 4, 4, 50, True, d_out[s0:], cap, d_sizes[s0:], d_st[s0:])
    torch.cuda.synchronize()
    del d_frames
assert not d_st.cpu().numpy().any()
sizes = d_sizes.cpu().numpy().astype(np.uint32)
pw, ph = (w + 7) // 8, (h + 7) // 8
d_pix = torch.empty((B, h, w, 4), dtype=torch.uint8, device="cuda")
d_prev = torch.empty((B, ph, pw, 4), dtype=torch.uint8, device="cuda")


def dec():
    eng.decode_device(d_out, cap, sizes, B, w, h, 4, d_pix, d_st, 0)


def prev():
    eng.preview_device(d_out, cap, sizes, B, w, h, 4, d_prev, d_st, 0)


ts = {"preview": [], "decode": []}
for fn in (prev, dec, prev, dec):
    fn()
torch.cuda.synchronize()
for _ in range(it):
    for name, fn in (("preview", prev), ("decode", dec)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts[name].append(e0.elapsed_time(e1))
assert not d_st.cpu().numpy().any()
# The preview is the decoder's own low-res plane: frame 0 against the full decode's
eng.preview_device(d_out, cap, sizes[:1], 1, w, h, 4, d_prev, d_st, 0)
torch.cuda.synchronize()
want = eng.debug_read("lowres", 0, 4 * ph * pw, decoder=True).reshape(4, ph, pw).transpose(1, 2, 0)
assert d_st[0].item() == 0

# Host path: from pinned memory, one call each over the first Bh frames (pinned room for their pixels).
Bh = min(B, 16)
streams = []
for i in range(Bh):
    p = himg_amd.pinned_empty(int(sizes[i]))
    p[:] = d_out[i, : int(sizes[i])].cpu().numpy()
    streams.append(p)
heads = [himg_amd.preview_peek(s)[3] for s in streams]
outs_p = [himg_amd.pinned_empty(ph * pw * 4) for _ in range(Bh)]
outs_d = [himg_amd.pinned_empty(h * w * 4) for _ in range(Bh)]
host = {"preview_batch": [], "decode_batch": []}
for k in range(max(2, it // 3) + 1):
    for name, fn in (("preview_batch", lambda: eng.preview_batch(streams, outs_p)),
                     ("decode_batch", lambda: eng.decode_batch(streams, outs_d))):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if k:   # (the first round warms up)
            host[name].append((t1 - t0) * 1e3)
got = eng.preview_batch(streams[:1])[0]
# frame 0's preview = its low-res plane (YCbCr -> RGB on the host, ycbcr.cpp:54-82)
y, cb, cr = (want[..., i].astype(np.int16) for i in range(3))
cb, cr = (cb << 1) - 255, (cr << 1) - 255
g = y - ((cb + cr + 2) >> 2)
rgb = np.stack([np.clip(g + cr, 0, 255), np.clip(g, 0, 255), np.clip(g + cb, 0, 255), want[..., 3]], -1).astype(np.uint8)
assert np.array_equal(got, rgb), "preview differs from the decoder's low-res plane"
eng.close()
med = lambda a: float(np.median(a))
res = {
    "frames": B, "width": w, "height": h, "content": "randtile q50 RGBA",
    "device_preview_ms": {"min": min(ts["preview"]), "median": med(ts["preview"])},
    "device_decode_ms": {"min": min(ts["decode"]), "median": med(ts["decode"])},
    "device_ratio_median": med(ts["preview"]) / med(ts["decode"]),
    "host_preview_batch_ms": med(host["preview_batch"]), "host_decode_batch_ms": med(host["decode_batch"]),
    "host_frames": Bh, "host_ratio": med(host["preview_batch"]) / med(host["decode_batch"]),
    "host_bytes_uploaded_preview": int(sum(heads)), "host_bytes_uploaded_decode": int(sizes[:Bh].astype(np.int64).sum()),
    "iters": it,
}
print(json.dumps(res))
