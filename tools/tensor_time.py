#!/usr/bin/env python3
"""The tensor decode against the uint8 decode followed by a conversion pass in torch, one JSON line
(GPU box), written to profiles/tensor_time.json as well.
Workload: B x 4096^2 RGBA q50 randtile streams in HBM, Co = 3, ImageNet scale / bias.
  (a) decode_tensor_device for float32, float16 and bfloat16;
  (b) decode_device alone;
  (c) decode_device followed by the fastest plain-torch expression found for the same tensor (every
      candidate is timed and listed; the fastest per dtype is the one (c) reports) -- the way to
      this tensor without the feature;
  (d) the same three for 256 x 256 windows at an origin per frame: decode_regions_tensor_device,
      decode_regions_device, decode_regions_device plus the conversion.
Warm-up 2, then 7 repetitions with all variants alternated in one process, device events around
each call; medians and ranges.  The per-kernel split comes from the stage profiler in a pass of its
own behind the timed one.  The torch candidates compute in two roundings (a product, then a sum) or
in the output type: they are the same tensor up to the last bits, not bit for bit.
args: [batch] [reps]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
WARM = 2
W = H = 4096
WIN = 256
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
eng = himg_amd.Engine(0)


def encode(n):
    cap = himg_amd.max_packed_size(W, H, 4)
    d_out = torch.empty((n, cap), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.ones(n, dtype=torch.int32, device="cuda")
    for s0 in range(0, n, 16):
        k = min(16, n - s0)
        d_frames = torch.from_numpy(np.stack([himg_amd.synth("randtile", s, W, H) for s in range(s0, s0 + k)])).cuda()
        eng.encode_device(d_frames, k, W, H, 4, 4, 50, True, d_out[s0:], cap, d_sizes[s0:], d_st[s0:])
        torch.cuda.synchronize()
        del d_frames
    assert not d_st.cpu().numpy().any()
    return d_out, cap, d_sizes.cpu().numpy().astype(np.uint32)


def timed(fns):
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)} for k, v in ts.items()}


def candidates(dt):
    """Plain-torch expressions for [n][3][h][w] of type dt from the interleaved bytes pix
    ([n][h][w][4] uint8): name -> fn(pix, out)."""
    sc32 = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float64).to(torch.float32).cuda().view(1, 3, 1, 1)
    bi32 = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float64).to(torch.float32).cuda().view(1, 3, 1, 1)
    sc, bi = sc32.to(dt), bi32.to(dt)

    def planar(pix):
        return pix[..., :3].permute(0, 3, 1, 2)

    c = {
        # the cast fused with the permuting copy, then a multiply and an add in place
        "out.copy_(x); out.mul_(scale).add_(bias)": lambda pix, out: out.copy_(planar(pix)).mul_(sc).add_(bi),
        # ... then one addcmul pass
        "out.copy_(x); torch.addcmul(bias, out, scale, out=out)":
            lambda pix, out: torch.addcmul(bi, out.copy_(planar(pix)), sc, out=out),
        # temporaries, as the expression is usually written
        "x.to(dtype).mul(scale).add(bias)": lambda pix, out: planar(pix).to(dt).mul(sc).add(bi),
        "torch.addcmul(bias, x.to(dtype), scale)": lambda pix, out: torch.addcmul(bi, planar(pix).to(dt), sc),
    }
    if dt != torch.float32:   # the arithmetic in float32, one rounding to the output type
        c["torch.addcmul(bias32, x.to(float32), scale32).to(dtype)"] = \
            lambda pix, out: torch.addcmul(bi32, planar(pix).to(torch.float32), sc32).to(dt)
    return c


def stage_split(fn):
    eng.profile(True)
    eng.profile_reset()
    fn()
    torch.cuda.synchronize()
    st = eng.profile_read()
    eng.profile(False)
    return {k: round(ms, 4) for k, (ms, _) in st.items()}


def case(d_in, cap, sizes, org):
    """org None: the full decode; else the WIN x WIN windows at org."""
    h, w = (H, W) if org is None else (WIN, WIN)
    d_st = torch.ones(B, dtype=torch.int32, device="cuda")
    d_pix = torch.empty((B, h, w, 4), dtype=torch.uint8, device="cuda")
    outs = {n: torch.empty((B, 3, h, w), dtype=dt, device="cuda") for n, dt in DTYPES.items()}
    descs = {n: himg_amd.tensor_desc(dt, 3, mean=MEAN, std=STD) for n, dt in DTYPES.items()}

    def u8():
        if org is None:
            eng.decode_device(d_in, cap, sizes, B, W, H, 4, d_pix, d_st)
        else:
            eng.decode_regions_device(d_in, cap, sizes, B, W, H, 4, org, w, h, d_pix, d_st)

    def tens(n):
        if org is None:
            eng.decode_tensor_device(d_in, cap, sizes, B, W, H, 4, descs[n], outs[n], d_st)
        else:
            eng.decode_regions_tensor_device(d_in, cap, sizes, B, W, H, 4, org, w, h, descs[n], outs[n], d_st)

    # which torch expression: each candidate's conversion pass alone, alternated
    u8()
    torch.cuda.synchronize()
    chosen, cand_ms = {}, {}
    for n, dt in DTYPES.items():
        cs = candidates(dt)
        t = timed({k: (lambda f=f: f(d_pix, outs[n])) for k, f in cs.items()})
        cand_ms[n] = {k: v["median"] for k, v in t.items()}
        chosen[n] = min(cand_ms[n], key=cand_ms[n].get)
        torch.cuda.empty_cache()
    fns = {"decode_u8": u8}
    for n, dt in DTYPES.items():
        f = candidates(dt)[chosen[n]]
        fns["tensor_" + n] = lambda n=n: tens(n)
        fns["u8_plus_torch_" + n] = lambda n=n, f=f: (u8(), f(d_pix, outs[n]))
    t = timed(fns)
    assert not d_st.cpu().numpy().any()
    res = {"decode_u8": t["decode_u8"], "stages_decode_u8": stage_split(u8)}
    for n, dt in DTYPES.items():
        a, c = t["tensor_" + n], t["u8_plus_torch_" + n]
        # the same tensor: against float32 arithmetic on two frames, within the output type's rounding
        tens(n)
        torch.cuda.synchronize()
        x = d_pix[:2, ..., :3].permute(0, 3, 1, 2).to(torch.float64)
        sc = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float64, device="cuda").view(1, 3, 1, 1)
        bi = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float64, device="cuda").view(1, 3, 1, 1)
        err = (outs[n][:2].to(torch.float64) - (x * sc + bi)).abs().max().item()
        assert err <= {"float32": 1e-6, "float16": 2e-3, "bfloat16": 2e-2}[n], (n, err)
        res[n] = {"tensor": a, "u8_plus_torch": c, "torch_expression": chosen[n],
                  "torch_candidates_median_ms": cand_ms[n],
                  "tensor_over_decode_u8": a["median"] / t["decode_u8"]["median"],
                  "tensor_over_u8_plus_torch": a["median"] / c["median"],
                  "max_abs_error_vs_float64": err,
                  "stages_tensor": stage_split(lambda n=n: tens(n))}
    return res


d_in, cap, sizes = encode(B)
rng = np.random.default_rng(7)
org = np.stack([rng.integers(0, W - WIN + 1, B), rng.integers(0, H - WIN + 1, B)], axis=1).astype(np.int32)
res = {"frames": B, "width": W, "height": H, "content": "randtile q50 RGBA", "out_channels": 3,
       "scale_bias": "ImageNet mean / std", "warmup": WARM, "reps": REPS,
       "windows": {"w": WIN, "h": WIN, "origins": "one per frame, seeded"}}
res["regions"] = case(d_in, cap, sizes, org)
torch.cuda.empty_cache()
res["full"] = case(d_in, cap, sizes, None)
res["wanted"] = {n: res["full"][n]["tensor_over_u8_plus_torch"] < 1.0 for n in DTYPES}
eng.close()
line = json.dumps(res)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
if os.environ.get("HIMG_TENSOR_TIME_WRITE", "1") == "1":
    with open(os.path.join(ROOT, "profiles", "tensor_time.json"), "w") as f:
        f.write(line + "\n")
