#!/usr/bin/env python3
"""The decode at 1/2 and 1/4 scale against the full decode, one JSON line (GPU box), written to
profiles/scaled_time.json as well.
Cases: B x 4096^2 RGBA randtile at q50 and q90, 2 B x 1920x1080 at q50, one 16384^2 frame --
decode_scaled_device at both scales against decode_device on the same streams, the variants
alternated in one process, device events after warm-up, medians of `iters`.  With
--parent-lib PATH (the library built from the parent commit) that library's decode_device runs
in the same alternation, on the same streams, beside this library's decode_device through a
second context made the same way (the control): the full decode must not move.
Host: decode_scaled_batch of 16 pinned 4096^2 streams against decode_batch.
The kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/scaled_time.py --only batch_q50` run.
args: [--batch B] [--iters N] [--big W] [--parent-lib PATH] [--only CASE] [--no-write]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--big", type=int, default=16384)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--only", default=None)
ap.add_argument("--no-write", action="store_true")
args = ap.parse_args()
B, it = args.batch, args.iters
eng = himg_amd.Engine(0)

vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t


def raw_context(path):
    """A second context, created and called through plain ctypes: the parent's library, or -- the
    control -- this one's (a context created second in a process, with its own workspace)."""
    L = C.CDLL(path)
    L.himg_hip_create.argtypes = [i32, C.POINTER(vp)]
    L.himg_hip_decode_device.argtypes = [vp, vp, sz, vp, i32, i32, i32, i32, vp, vp, vp]
    ctx = vp()
    assert L.himg_hip_create(0, C.byref(ctx)) == 0
    return L, ctx


parent = raw_context(os.path.abspath(args.parent_lib)) if args.parent_lib else None
control = raw_context(himg_amd.lib()._name) if parent else None


def raw_decode(lc, d_in, cap, sizes, n, w, h, d_pix, d_st):
    hs = np.ascontiguousarray(sizes, np.uint32)
    rc = lc[0].himg_hip_decode_device(lc[1], d_in.data_ptr(), cap, hs.ctypes.data, n, w, h, 4, d_pix.data_ptr(),
                                      d_st.data_ptr(), None)
    assert rc == 0, rc


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


def case(n, w, h, q):
    d_in, cap, sizes = encode(w, h, n, q)
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    d_pix = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    outs = {}
    for s in (1, 2):
        ow, oh = himg_amd.scaled_size(w, h, s)
        outs[s] = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
    fns = {"decode": lambda: eng.decode_device(d_in, cap, sizes, n, w, h, 4, d_pix, d_st)}
    if parent:
        fns["decode_parent"] = lambda: raw_decode(parent, d_in, cap, sizes, n, w, h, d_pix, d_st)
        fns["decode_second_context"] = lambda: raw_decode(control, d_in, cap, sizes, n, w, h, d_pix, d_st)
    fns["scaled_1_2"] = lambda: eng.decode_scaled_device(d_in, cap, sizes, n, w, h, 4, 1, outs[1], d_st)
    fns["scaled_1_4"] = lambda: eng.decode_scaled_device(d_in, cap, sizes, n, w, h, 4, 2, outs[2], d_st)
    t = timed(fns)
    assert not d_st.cpu().numpy().any()
    # sanity, not parity (tests/test_gpu_scaled.py holds that): close to the shrunken full decode
    fns["decode"]()
    torch.cuda.synchronize()
    for s in (1, 2):
        f = 1 << s
        box = d_pix[0, :h // f * f, :w // f * f].float().reshape(h // f, f, w // f, f, 4).mean(dim=(1, 3))
        diff = (outs[s][0, :h // f, :w // f].float() - box).abs().mean().item()
        assert diff < 2.0, (s, diff)
    t["frames"], t["width"], t["height"], t["content"] = n, w, h, "randtile q%d RGBA" % q
    t["packed_bytes"] = int(sizes.astype(np.int64).sum())
    for k in ("scaled_1_2", "scaled_1_4"):
        t[k]["ratio_median"] = t[k]["median"] / t["decode"]["median"]
    if parent:
        t["decode"]["ratio_to_parent_median"] = t["decode"]["median"] / t["decode_parent"]["median"]
        t["decode_second_context"]["ratio_to_parent_median"] = t["decode_second_context"]["median"] / t["decode_parent"]["median"]
    del d_pix, d_in, outs
    torch.cuda.empty_cache()
    return t


def host_case(n=16, w=4096, h=4096, q=50):
    d_in, cap, sizes = encode(w, h, n, q)
    streams = []
    for i in range(n):
        p = himg_amd.pinned_empty(int(sizes[i]))
        p[:] = d_in[i, :int(sizes[i])].cpu().numpy()
        streams.append(p)
    del d_in
    full = [himg_amd.pinned_empty(w * h * 4) for _ in range(n)]
    res = {"frames": n, "width": w, "height": h, "content": "randtile q%d RGBA, pinned host memory" % q,
           "bytes_uploaded": int(sizes.astype(np.int64).sum())}
    fns = {"decode_batch": lambda: eng.decode_batch(streams, full)}
    for s in (1, 2):
        ow, oh = himg_amd.scaled_size(w, h, s)
        outs = [himg_amd.pinned_empty(ow * oh * 4) for _ in range(n)]
        fns["decode_scaled_batch_1_%d" % (1 << s)] = (lambda s=s, outs=outs: eng.decode_scaled_batch(streams, s, outs))
    ts = {k: [] for k in fns}
    for k in range(max(2, it // 3) + 1):
        for name, fn in fns.items():
            t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
            if k:
                ts[name].append((t1 - t0) * 1e3)
    for name, v in ts.items():
        res[name] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    return res


CASES = {
    "batch_q50": lambda: case(B, 4096, 4096, 50),
    "batch_q90": lambda: case(B, 4096, 4096, 90),
    "batch_1080p_q50": lambda: case(2 * B, 1920, 1080, 50),
    "single_big": lambda: case(1, args.big, args.big, 50),
    "host_batch_16": host_case,
}
res = {"iters": it, "parent_lib": bool(parent)}
for name, fn in CASES.items():
    if args.only and name != args.only:
        continue
    res[name] = fn()
eng.close()
line = json.dumps(res)
print(line)
if not args.no_write and not args.only:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scaled_time.json"), "w") as f:
        f.write(line + "\n")
