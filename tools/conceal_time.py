#!/usr/bin/env python3
"""The concealing decode against the full decode, one JSON line (GPU box), written to
profiles/conceal_time.json as well.  B RGBA randtile streams of 4096^2 in HBM, q50 (encoded on the device
beforehand).  decode_conceal_device on
  (a) the clean batch,
  (b) one payload bit flipped in one frame,
  (c) one damaged block row in every frame (eight payload bytes inverted),
  (d) every frame's header chain broken at row rows / 2 (that row's size header says more than the chunk holds),
and decode_device on the clean batch: alternated in one process, device events after warm-up, medians of
`iters` runs with min - max.  (a) is compared with decode_device's output byte for byte.  The repair pass's
own launches on the clean batch come from the context's stage timer: the stages decode_conceal_device runs
beyond decode_device's, the LRES chain's second run as the difference of its stages' sums.

--compare TREE: decode_device alone, and bench.py's headline, at this tree and at the tree in TREE (a
checkout of the parent commit, built), alternated in child processes: the yardstick of (a), and whether
the new forms have leaked into the existing kernels.

args: [batch] [iters] [--compare TREE] [--bench-steps K] [--out FILE]
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
compare, bench_steps = None, 20
out_path = os.path.join(ROOT, "profiles", "conceal_time.json")
for flag in ("--compare", "--bench-steps", "--out"):
    while flag in argv:
        i = argv.index(flag)
        v = argv[i + 1]
        del argv[i:i + 2]
        if flag == "--compare":
            compare = os.path.abspath(v)
        elif flag == "--bench-steps":
            bench_steps = int(v)
        else:
            out_path = os.path.abspath(v)
sys.path.insert(0, child_tree or ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B = int(argv[0]) if len(argv) > 0 else 128
it = int(argv[1]) if len(argv) > 1 else 7
W = H = 4096
Q = 50
ROWS = (H + 7) // 8


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

# Each stream's row index (the host walk), for the damage below.
index = []
for f in range(B):
    _, _, _, off, ln, _ = himg_amd.index_host(d_in[f, :int(sizes[f])].cpu().numpy())
    index.append((off.astype(np.int64), ln.astype(np.int64)))
d_con = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
d_cn = torch.zeros(B, dtype=torch.int32, device="cuda")
d_map = torch.zeros((B, ROWS), dtype=torch.uint8, device="cuda")
st2 = torch.ones(B, dtype=torch.int32, device="cuda")


def conceal(d):
    eng.decode_conceal_device(d, stride, sizes, B, W, H, 4, d_con, d_cn, d_map, st2)


def outcome(d):
    conceal(d)
    torch.cuda.synchronize()
    assert not st2.cpu().numpy().any()
    cn = d_cn.cpu().numpy()
    return {"frames_with_concealed_rows": int((cn > 0).sum()), "concealed_rows": int(cn.sum()), "rows_per_frame": ROWS}


# (b) one bit in the middle of a row's payload of one frame -- the first position the decoder rejects
d_b = d_in.clone()
fb, rb = B // 2, ROWS // 2
for k in range(64):
    pos = int(index[fb][0][rb] + index[fb][1][rb] // 2 + k)
    d_b[fb, pos] ^= 0x10
    if outcome(d_b)["concealed_rows"]:
        break
    d_b[fb, pos] ^= 0x10
# (c) eight inverted bytes in the middle of one row of every frame
d_c = d_in.clone()
for f in range(B):
    r = (7 * f + 3) % ROWS
    pos = int(index[f][0][r] + index[f][1][r] // 2)
    d_c[f, pos:pos + 8] ^= 0xFF
# (d) the size header of row ROWS / 2 of every frame says more than the chunk holds
d_d = d_in.clone()
for f in range(B):
    o, n = int(index[f][0][ROWS // 2]), int(index[f][1][ROWS // 2])
    hdr = 4 if n > 0x7fff else 2
    d_d[f, o - hdr:o] = 0xFF
cases = {"a_clean": d_in, "b_one_bit_one_frame": d_b, "c_one_row_every_frame": d_c, "d_headers_cut_at_half": d_d}

fns = {"decode_device": full}
fns.update({"conceal_" + k: (lambda d=d: conceal(d)) for k, d in cases.items()})
t = timed(fns)
res = {"iters": it, "frames": B, "content": "randtile q%d RGBA %dx%d" % (Q, W, H),
       "mean_stream_bytes": float(sizes.mean()), "times_ms": t,
       "outcomes": {k: outcome(d) for k, d in cases.items()}}
assert res["outcomes"]["a_clean"]["concealed_rows"] == 0
full()
conceal(d_in)
torch.cuda.synchronize()
assert not st.cpu().numpy().any() and torch.equal(d_out, d_con) and not d_map.any()
dd = t["decode_device"]["median"]
res["conceal_over_decode_device"] = {k: t["conceal_" + k]["median"] / dd for k in cases}


def stage_ms(fn):
    eng.profile(True)
    eng.profile_reset()
    for _ in range(it):
        fn()
    torch.cuda.synchronize()
    stages = eng.profile_read()
    eng.profile(False)
    return {k: v[0] / it for k, v in stages.items() if v[1]}


s_full, s_con = stage_ms(full), stage_ms(lambda: conceal(d_in))
lres = ("k_lres_spec", "k_lres_fix", "k_lres_write", "k_lres_finish", "k_lres_unpredict")
own = {k: v for k, v in s_con.items() if k not in s_full}
own["lres_chain_again"] = sum(s_con.get(k, 0.0) for k in lres) - sum(s_full.get(k, 0.0) for k in lres)
res["repair_pass_on_clean_batch"] = {"stage_ms_per_call": own, "sum_ms": float(sum(own.values())),
                                     "decode_device_stage_ms_per_call": s_full, "conceal_stage_ms_per_call": s_con}
eng.close()
del d_con, d_frames, d_out, d_in, d_b, d_c, d_d
torch.cuda.empty_cache()


def write(r):
    line = json.dumps(r)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
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
    par = float(np.median([c["median"] for c in cmp_["decode_device_ms"]["parent"]]))
    a = t["conceal_a_clean"]["median"]
    res["clean_batch_against_parent_decode_device"] = {
        "parent_decode_device_ms": par, "conceal_clean_ms": a, "over_ms": a - par,
        "allowance_ms": res["repair_pass_on_clean_batch"]["sum_ms"]}

print(write(res))
