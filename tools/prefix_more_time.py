#!/usr/bin/env python3
"""The prefix decode continued (decode_prefix_more_device) against the stateless prefix decode and the full
decode, one JSON line (GPU box), written to profiles/prefix_more_time.json as well.  B RGBA randtile streams
of 4096^2 in HBM, q50 (encoded on the device beforehand); everything alternated in one process, device events
after warm-up, medians with min - max.

  chain   ten equal byte steps, 10 % .. 100 % of each stream: the ten incremental calls from a fresh state,
          ten decode_prefix_device calls at the same avails, one decode_device; each step on its own too.
          The chain's last picture is compared with decode_device's, byte for byte.
  floor   a step that completes ONE new row per frame (from 50 % of the stream), and a step with no new
          bytes; the context's stage timer says how much of the latter is the re-run head (parse + LRES
          chain), the resumed walk, and the empty workgroups of the full-height grids.
  host    one stream, the same ten steps through decode_prefix_more against ten decode_prefix calls: bytes
          uploaded, bytes downloaded, host wall time.

--compare TREE: decode_device alone (tools/prefix_time.py's child), and bench.py's headline, at this tree and
at the tree in TREE (a checkout of the parent commit, built), alternated in child processes.

args: [batch] [iters] [--compare TREE] [--bench-steps K]"""
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
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
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import himg_amd  # noqa: E402

B = int(argv[0]) if len(argv) > 0 else 128
it = int(argv[1]) if len(argv) > 1 else 7
W = H = 4096
Q = 50
STEPS = 10
ROW_BYTES = 8 * W * 4


def stats(v):
    return {"min": min(v), "median": float(np.median(v)), "max": max(v), "runs": len(v)}


def ev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


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
d_full = d_frames            # (the source pictures are no longer needed: their buffer is reused)
d_pic = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
d_rows = torch.zeros(B, dtype=torch.int32, device="cuda")
d_state = torch.zeros(B * 16, dtype=torch.uint8, device="cuda")
d_keep = torch.zeros(B * 16, dtype=torch.uint8, device="cuda")
AV = [(sizes.astype(np.uint64) * k // STEPS).astype(np.uint32) for k in range(1, STEPS + 1)]
assert (AV[-1] == sizes).all()


def full():
    eng.decode_device(d_in, stride, sizes, B, W, H, 4, d_full, d_st)


def prefix(av):
    eng.decode_prefix_device(d_in, stride, av, B, W, H, 4, d_pic, d_rows, d_st)


def more(av):
    eng.decode_prefix_more_device(d_in, stride, av, B, W, H, 4, d_state, d_pic, d_rows, d_st)


def ok():
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()


# ---- the chain -------------------------------------------------------------------------------------
t = {"decode_device": [], "more": [[] for _ in AV], "prefix": [[] for _ in AV]}
rows_at = []
for rnd in range(it + 2):   # (two warm-up rounds)
    keep = rnd >= 2
    x = ev_ms(full)
    if keep:
        t["decode_device"].append(x)
    d_state.zero_()
    for k, av in enumerate(AV):
        x = ev_ms(lambda: more(av))
        if keep:
            t["more"][k].append(x)
        if rnd == 0:
            ok()
            rows_at.append(float(d_rows.cpu().numpy().mean()))
    if rnd == 0:
        full()
        ok()
        assert torch.equal(d_full, d_pic), "the chain's picture is not decode_device's"
    for k, av in enumerate(AV):
        x = ev_ms(lambda: prefix(av))
        if keep:
            t["prefix"][k].append(x)
ok()
chain = {"decode_device_ms": stats(t["decode_device"]),
         "more_step_ms": [stats(v) for v in t["more"]], "prefix_step_ms": [stats(v) for v in t["prefix"]],
         "more_sum_ms": stats([sum(v[r] for v in t["more"]) for r in range(it)]),
         "prefix_sum_ms": stats([sum(v[r] for v in t["prefix"]) for r in range(it)]),
         "mean_rows_complete_of_%d" % ((H + 7) // 8): rows_at}
chain["more_sum_over_prefix_sum"] = chain["more_sum_ms"]["median"] / chain["prefix_sum_ms"]["median"]
chain["more_sum_over_decode_device"] = chain["more_sum_ms"]["median"] / chain["decode_device_ms"]["median"]
res = {"iters": it, "frames": B, "content": "randtile q%d RGBA %dx%d" % (Q, W, H),
       "mean_stream_bytes": float(sizes.mean()), "chain_of_%d_equal_byte_steps" % STEPS: chain}

# ---- the floor -------------------------------------------------------------------------------------
# Each frame at half its stream, then at the end of the next row's payload (the host's walk says where).
half = AV[STEPS // 2 - 1]
nxt = []
for f in range(B):
    s = d_in[f, :int(sizes[f])].cpu().numpy()
    p = himg_amd.prefix_peek(s, int(half[f]))
    while himg_amd.prefix_peek(s, p["next_bytes"])["rows_complete"] == p["rows_complete"]:   # (behind a cut header first)
        p = himg_amd.prefix_peek(s, p["next_bytes"])
    nxt.append(p["next_bytes"])
nxt = np.array(nxt, np.uint32)
d_state.zero_()
more(half)
ok()
k_half = d_rows.cpu().numpy().copy()
d_keep.copy_(d_state)
tf = {"one_new_row": [], "no_new_bytes": [], "prefix_at_the_same_bytes": []}
for rnd in range(it + 2):
    d_state.copy_(d_keep)
    a = ev_ms(lambda: more(nxt))
    if rnd == 0:
        ok()
        assert (d_rows.cpu().numpy() == k_half + 1).all()
    d_state.copy_(d_keep)
    b = ev_ms(lambda: more(half))
    c = ev_ms(lambda: prefix(nxt))
    if rnd >= 2:
        tf["one_new_row"].append(a); tf["no_new_bytes"].append(b); tf["prefix_at_the_same_bytes"].append(c)
ok()
floor = {k + "_ms": stats(v) for k, v in tf.items()}
eng.profile(True)
for name, av in (("no_new_bytes", half), ("one_new_row", nxt)):
    eng.profile_reset()
    for _ in range(it):
        d_state.copy_(d_keep)
        more(av)
    torch.cuda.synchronize()
    st = {k: v[0] / v[1] for k, v in eng.profile_read().items() if v[1]}
    walk = sum(v for k, v in st.items() if k == "k_span_rowwalk")
    grids = sum(v for k, v in st.items() if k in ("k_prefix_fill", "k_span_count", "k_span_count_w", "k_dec_span<false>"))
    ends = sum(v for k, v in st.items() if k in ("k_span_gate", "k_span_status"))
    floor["stages_%s_ms_per_launch" % name] = {
        "head_parse_and_lres_chain": sum(st.values()) - walk - grids - ends, "resumed_walk": walk,
        "full_height_grids_fill_count_rows": grids, "gates_and_status": ends, "all": st}
eng.profile(False)
res["floor_from_half_the_stream"] = floor

# ---- the host form ---------------------------------------------------------------------------------
s0 = d_in[0, :int(sizes[0])].cpu().numpy().copy()
av0 = [int(a[0]) for a in AV]
th = {"more": [], "prefix": []}
up = down = 0
for rnd in range(it + 1):
    state, pic = himg_amd.prefix_states(1), None
    t0 = time.perf_counter()
    for a in av0:
        before = state.copy()
        pic, k = eng.decode_prefix_more(s0[:a], state[0:1], pic)
        if rnd == 0:
            if before["started"][0]:
                up += himg_amd.prefix_peek(s0, a)["head_bytes"] + a - int(before["walk_pos"][0])
                down += (min(8 * k, H) - 8 * int(before["rows_done"][0])) * W * 4
            else:
                up += a
                down += H * W * 4
    t1 = time.perf_counter()
    out = None
    for a in av0:
        out, k2 = eng.decode_prefix(s0[:a], out)
    t2 = time.perf_counter()
    if rnd == 0:
        assert np.array_equal(pic, out) and k == k2
    else:
        th["more"].append((t1 - t0) * 1e3); th["prefix"].append((t2 - t1) * 1e3)
res["host_form_one_stream"] = {"stream_bytes": int(sizes[0]), "more_ms": stats(th["more"]), "prefix_ms": stats(th["prefix"]),
                               "more_bytes_uploaded": int(up), "more_bytes_downloaded": int(down),
                               "prefix_bytes_uploaded": int(sum(av0)), "prefix_bytes_downloaded": STEPS * H * W * 4}
eng.close()
del d_pic, d_frames, d_full, d_in
torch.cuda.empty_cache()


def write(r):
    line = json.dumps(r)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "prefix_more_time.json"), "w") as f:
        f.write(line + "\n")
    return line


write(res)   # (the comparison below takes minutes: what is measured so far is kept)
if compare:
    def child(tree):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prefix_time.py"), "--decode-only", tree, str(B), str(it)],
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
