#!/usr/bin/env python3
"""The decode of stream prefixes against the full decode, one JSON line (GPU box), written to
profiles/prefix_time.json as well.  B RGBA randtile streams of 4096^2 in HBM, q50 (encoded on the device
beforehand).  decode_prefix_device at avail = 100 %, 50 % and 10 % of each stream and at each stream's
head_bytes, and decode_device on the same streams: alternated in one process, device events after
warm-up, medians with min - max.  The 100 % result is compared with decode_device's, byte for byte.
The fill kernel's own time (the context's stage timer, avail = head_bytes: every block row is filled)
gives its bytes per second; himg_amd/bin/hbm_calib gives the box's write-only and copy ceilings.

--compare TREE: decode_device alone, and bench.py's headline, at this tree and at the tree in TREE (a
checkout of the parent commit, built), alternated in child processes: whether the new forms have leaked
into the existing kernels.

args: [batch] [iters] [--compare TREE] [--bench-steps K]
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
while "--compare" in argv:
    i = argv.index("--compare")
    compare = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
while "--bench-steps" in argv:
    i = argv.index("--bench-steps")
    bench_steps = int(argv[i + 1])
    del argv[i:i + 2]
sys.path.insert(0, child_tree or ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B = int(argv[0]) if len(argv) > 0 else 128
it = int(argv[1]) if len(argv) > 1 else 7
W = H = 4096
Q = 50


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


eng = himg_amd.Engine(0)
with ThreadPoolExecutor(16) as pool:
    frames = list(pool.map(lambda s: himg_amd.synth("randtile", s, W, H), range(B)))
d_frames = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
for f, fr in enumerate(frames):
    d_frames[f] = torch.from_numpy(fr).cuda()
del frames
stride = (himg_amd.max_packed_size(W, H, 4) + 255) // 256 * 256
d_in = torch.zeros((B, stride), dtype=torch.uint8, device="cuda")
d_sz = torch.zeros(B, dtype=torch.int32, device="cuda")
d_st = torch.ones(B, dtype=torch.int32, device="cuda")
eng.encode_device(d_frames, B, W, H, 4, 4, Q, True, d_in, stride, d_sz, d_st)
torch.cuda.synchronize()
assert not d_st.cpu().numpy().any()
sizes = d_sz.cpu().numpy().astype(np.uint32)
d_out = d_frames            # (the source pictures are no longer needed: their buffer is reused)
st = torch.ones(B, dtype=torch.int32, device="cuda")


def full():
    eng.decode_device(d_in, stride, sizes, B, W, H, 4, d_out, st)


if child_tree:
    t = timed({"decode_device": full})
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    print(json.dumps({"tree": child_tree, "frames": B, "decode_device": t["decode_device"]}))
    eng.close()
    sys.exit(0)

d_pre = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
d_rows = torch.zeros(B, dtype=torch.int32, device="cuda")
st2 = torch.ones(B, dtype=torch.int32, device="cuda")
heads = []
for f in range(B):   # head_bytes of each stream: the host walk over its first bytes
    n = 1 << 16
    while True:
        try:
            heads.append(himg_amd.prefix_peek(d_in[f, :n].cpu().numpy())["head_bytes"])
            break
        except himg_amd.HimgError as e:
            assert e.code == himg_amd.HIMG_ERR_CAPACITY and n < int(sizes[f])
            n = min(4 * n, int(sizes[f]))
heads = np.array(heads, np.uint32)
AVAIL = {"100": sizes, "50": (sizes // 2).astype(np.uint32), "10": (sizes // 10).astype(np.uint32), "head": heads}
assert (AVAIL["10"] >= heads).all()


def prefix(av):
    eng.decode_prefix_device(d_in, stride, av, B, W, H, 4, d_pre, d_rows, st2)


fns = {"decode_device": full}
fns.update({"prefix_" + k: (lambda av=av: prefix(av)) for k, av in AVAIL.items()})
t = timed(fns)
res = {"iters": it, "frames": B, "content": "randtile q%d RGBA %dx%d" % (Q, W, H),
       "mean_stream_bytes": float(sizes.mean()), "mean_head_bytes": float(heads.mean()), "times_ms": t}
rows = {}
for k, av in AVAIL.items():
    prefix(av)
    torch.cuda.synchronize()
    assert not st2.cpu().numpy().any()
    rows[k] = float(d_rows.cpu().numpy().mean())
res["mean_rows_complete_of_%d" % ((H + 7) // 8)] = rows
full()
prefix(sizes)
torch.cuda.synchronize()
assert not st.cpu().numpy().any() and torch.equal(d_out, d_pre)
dd = t["decode_device"]["median"]
res["prefix_over_decode_device"] = {k: t["prefix_" + k]["median"] / dd for k in AVAIL}

# The fill kernel alone, every row filled: a write-only stream of B x H x W x 4 bytes.
eng.profile(True)
eng.profile_reset()
for _ in range(it):
    prefix(heads)
torch.cuda.synchronize()
stages = eng.profile_read()
eng.profile(False)
fill_ms, launches = stages["k_prefix_fill"]
fill = {"ms_per_launch": fill_ms / launches, "bytes": B * H * W * 4,
        "GBs": B * H * W * 4 / (fill_ms / launches * 1e-3) / 1e9,
        "stage_ms_per_launch_at_head": {k: v[0] / v[1] for k, v in stages.items() if v[1]}}
exe = os.path.join(ROOT, "himg_amd", "bin", "hbm_calib")
if os.path.exists(exe):
    torch.cuda.empty_cache()
    r = subprocess.run([exe, "2"], capture_output=True, text=True, timeout=180)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode == 0 and line:
        c = json.loads(line[-1])
        fill["hbm_calib"] = {"write_only_GBs": c["write_GBs"], "copy_read_plus_write_GBs": c["copy_GBs_rd_plus_wr"]}
        fill["fraction_of_write_only_ceiling"] = fill["GBs"] / c["write_GBs"]
        fill["fraction_of_copy_ceiling"] = fill["GBs"] / c["copy_GBs_rd_plus_wr"]
res["fill_kernel"] = fill
eng.close()
del d_pre, d_frames, d_out, d_in
torch.cuda.empty_cache()



def write(r):
    line = json.dumps(r)
    if os.environ.get("HIMG_PREFIX_TIME_WRITE", "1") == "1":
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "prefix_time.json"), "w") as f:
            f.write(line + "\n")
    return line


write(res)   # (the comparison below takes minutes: what is measured so far is kept)
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
