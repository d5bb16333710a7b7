"""GPU (-m gpu): the forms of the decoder's row kernel chosen by environment knobs
(HIMG_PERSIST_ROWS: persistent workgroups or one workgroup per row; HIMG_PREFETCH_ROWS: touch
loads for the next row's packed bytes) decode the same streams to the same pixels as the CPU
oracle.  The knobs are read from the environment when a context is created; every form runs in a
child process with its own environment."""
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = textwrap.dedent("""
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import himg_amd
    import oracle_lib as ol
    eng = himg_amd.Engine(0)
    # (width, height, frames): more grid elements than the GPU has CUs, so that a persistent
    # workgroup takes several; 4096 px (one row per workgroup, compile-time strides), 1920 px
    # (two rows per workgroup), 1000 px (run-time strides, ragged tiles), 3 channels (general form).
    # Narrow rows whose block-row count is one more than a multiple of the rows a workgroup takes
    # (eight at these widths): the frame's last workgroup has ONE row, so most of its wavefronts --
    # those that touch the next row's bytes among them -- have no tile to transform; batches of
    # more than a thousand grid elements, so that every persistent workgroup goes on to further
    # rows behind such a one.
    for w, h, B, ch in ((4096, 64, 40, 4), (1920, 136, 40, 4), (1000, 72, 96, 4), (520, 64, 96, 3),
                        (256, 72, 600, 4), (200, 72, 600, 4), (64, 136, 600, 4), (256, 72, 600, 3)):
        frames = [himg_amd.synth("randtile", s, w, h)[:, :, :ch].copy() for s in range(3)]
        streams = [eng.encode(f, 50, True, channels=ch, pixel_stride=ch) for f in frames]
        want = []
        for s in streams:
            rc, px = ol.oracle_decode(s)
            assert rc == 0
            want.append(px)
        cap = (max(len(s) for s in streams) + 255) // 256 * 256
        d_in = torch.zeros((B, cap), dtype=torch.uint8, device="cuda")
        sizes = np.zeros(B, np.uint32)
        for b in range(B):
            s = streams[b %% 3]
            d_in[b, : len(s)] = torch.from_numpy(np.asarray(s)).cuda()
            sizes[b] = len(s)
        d_pix = torch.empty((B, h, w, ch), dtype=torch.uint8, device="cuda")
        d_st = torch.ones(B, dtype=torch.int32, device="cuda")
        eng.decode_device(d_in, cap, sizes, B, w, h, ch, d_pix, d_st, 0)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any(), (w, h, "status")
        pix = d_pix.cpu().numpy()
        for b in range(B):
            assert np.array_equal(pix[b], want[b %% 3].reshape(h, w, ch)), (w, h, b)
    print("forms ok")
""")


# Damaged frames in a device batch: a frame the decoder rejects (the row workgroups of such a frame
# leave at once; a workgroup whose row fails leaves after the entropy pass) directly in front of a
# good one in the persistent loop.  Verdicts and pixels against the oracle, twice on one engine.
CHILD_DAMAGED = textwrap.dedent("""
    import struct
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import himg_amd
    import oracle_lib as ol
    w, h = %(w)d, %(h)d
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rows, cols = (h + 7) // 8, (w + 7) // 8
    # Rows a workgroup takes at most: one at 4096 pixels, else what the transform has lanes for
    # (two lanes per tile, whole wavefronts), never more than eight -- a lower bound on the grid.
    rpw_max = 1 if w == 4096 else max(1, min(8, 1024 // (((cols + 31) // 32) * 64)))
    gx_min = (rows + rpw_max - 1) // rpw_max
    B = (4 * n_cu + gx_min - 1) // gx_min + 3
    assert gx_min * B >= 4 * n_cu

    def fres_layout(s):
        b, i = bytes(s), 12
        while i + 8 <= len(b):
            sz = struct.unpack("<I", b[i + 4:i + 8])[0]
            if b[i:i + 4] == b"FRES":
                return i + 8
            i += 8 + sz
        raise AssertionError("no FRES chunk")

    good = [ol.oracle_encode(himg_amd.synth("randtile", s, w, h), 50, True) for s in range(3)]
    rng = np.random.RandomState(1000 + w)
    # 3 of each kind, drawn by seed and kept by the ORACLE's verdict alone: of the payload bits two
    # it accepts (other pixels), of the row headers and the trees two each it rejects.
    pool, verdict, kinds = [], [], []
    for kind, need_acc, need_rej in (("payload", 2, 0), ("header", 0, 2), ("tree", 0, 2)):
        kept = 0
        for attempt in range(400):
            if kept == 3:
                break
            src = good[kept]
            _, _, _, off, ln, first = himg_amd.index_host(src)
            bad = src.copy()
            r = int(rng.randint(0, rows))
            if kind == "payload":
                at = int(off[r]) + int(rng.randint(0, int(ln[r])))
            elif kind == "header":
                at = int(off[r]) - 2 + int(rng.randint(0, 2))      # the row's two size bytes
            else:
                t0 = fres_layout(src)
                at = t0 + int(rng.randint(0, first - t0))
            bad[at] ^= 1 << int(rng.randint(0, 8))
            ok = ol.oracle_decode(bad)[0] == 0
            free = 3 - kept - need_acc - need_rej
            if ok and need_acc:
                need_acc -= 1
            elif not ok and need_rej:
                need_rej -= 1
            elif free > 0:
                pass
            else:
                continue
            pool.append(bad); verdict.append(ok); kinds.append(kind); kept += 1
        assert kept == 3, (w, kind)
    assert len(pool) == 9 and sum(verdict) >= 2 and len(verdict) - sum(verdict) >= 4, verdict
    pool = good + pool
    want = []
    for s in pool:
        rc, px = ol.oracle_decode(s)
        want.append(px if rc == 0 else None)
    assert all(x is not None for x in want[:3])
    okv = np.array([x is not None for x in want])
    # The order: seeded; half of the frames good ones, so that a rejected frame stands directly in
    # front of a good one many times -- in the batch, and in whatever stride a workgroup walks it.
    pick = np.where(rng.randint(0, 2, B) == 1, rng.randint(0, 3, B), 3 + rng.randint(0, 9, B))
    pick[:18] = [3 + k // 2 if k %% 2 == 0 else k // 2 %% 3 for k in range(18)]    # each mutation once in front of a good frame
    assert int((~okv[pick[:-1]] & (pick[1:] < 3)).sum()) >= B // 16, "rejected frames in front of good ones"
    cap = (max(len(s) for s in pool) + 255) // 256 * 256
    h_in = np.zeros((len(pool), cap), np.uint8)
    for k, s in enumerate(pool):
        h_in[k, : len(s)] = s
    d_idx = torch.from_numpy(pick.astype(np.int64)).cuda()
    d_in = torch.from_numpy(h_in).cuda()[d_idx].contiguous()
    sizes = np.array([len(pool[k]) for k in pick], np.uint32)
    d_want = torch.from_numpy(np.stack([x if x is not None else np.zeros((h, w, 4), np.uint8) for x in want])).cuda()
    acc = torch.from_numpy(okv[pick]).cuda()
    eng = himg_amd.Engine(0)
    d_pix = torch.empty((B, h, w, 4), dtype=torch.uint8, device="cuda")
    for rnd in range(2):
        d_pix.fill_(0xA5)
        d_st = torch.ones(B, dtype=torch.int32, device="cuda")
        eng.decode_device(d_in, cap, sizes, B, w, h, 4, d_pix, d_st, 0)
        torch.cuda.synchronize()
        st = d_st.cpu().numpy()
        wrong = np.flatnonzero((st == 0) != okv[pick])
        assert wrong.size == 0, (w, h, rnd, "verdicts", wrong[:8], pick[wrong[:8]], st[wrong[:8]])
        same = (d_pix[acc] == d_want[d_idx[acc]]).flatten(1).all(1).cpu().numpy()
        assert same.all(), (w, h, rnd, "pixels", np.flatnonzero(okv[pick])[~same][:8])
    print("damaged ok", w, h, B, kinds, verdict)
""")


@pytest.mark.parametrize("w,h", [(4096, 64), (1920, 136), (1000, 72), (256, 72)])
@pytest.mark.parametrize("persist", ["1", "0", "7"])
def test_damaged_frames_in_a_device_batch(persist, w, h):
    env = dict(os.environ, HIMG_PERSIST_ROWS=persist)
    code = CHILD_DAMAGED % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "w": w, "h": h}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "damaged ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("persist,prefetch", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0"), ("7", "1")])
def test_row_kernel_forms_match_oracle(persist, prefetch):
    env = dict(os.environ, HIMG_PERSIST_ROWS=persist, HIMG_PREFETCH_ROWS=prefetch)
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
