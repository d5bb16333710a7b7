"""GPU (-m gpu): the prefix decode continued -- decode_prefix_more_device (a batch in HBM with a state per frame
in device memory) and decode_prefix_more (a host slice, a host state) against tests/prefix_more_model.py, byte
for byte.  One helper checks every step: before it the whole device picture is a sentinel; after it a resumed
frame holds the oracle's full decode in block rows [k_prev, k_new) and the sentinel everywhere else, a fresh
frame holds the prefix decode's picture, and d_rows, d_status and the state read back are the model's.  No
tolerances."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import himg_amd
import oracle_lib as ol
import prefix_model as pm
import prefix_more_model as mm
import scaled_model as sm
import stream_gate as sg

pytestmark = pytest.mark.gpu

ST_ARG = 1        # a frame's word in the status array for a state that cannot be right (HIMG_ERR_ARG)
ST_SHORT = 5      # ... for a prefix below its first row header (HIMG_ERR_CAPACITY)
SENTINEL = 0x5A


@pytest.fixture
def eng(engine):
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)
    yield engine
    engine.set_option("fix_t2", 0)
    engine.set_option("count_wave", -1)


def _stream(kind, w, h, c=4, q=50, ycbcr=True, seed=0):
    img = himg_amd.synth(kind, seed, w, h)
    if c != img.shape[2]:
        img = np.ascontiguousarray(img[:, :, :c] if c > 1 else img[:, :, 0])
    return np.frombuffer(ol.oracle_encode(img, q, ycbcr), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def _model(kind, w, h, c=4, q=50, ycbcr=True, seed=0, fix=False):
    return pm.Model(_stream(kind, w, h, c, q, ycbcr, seed), fix)


def _states_array(states):
    arr = himg_amd.prefix_states(len(states))
    for f, s in enumerate(states):
        for k, v in s.items():
            arr[k][f] = v
    return arr


class Chain:
    """n pictures of one shape on the device, their states beside them, and the model's states on the host.
    streams[f]: the bytes frame f is fed (default: its model's stream; a damaged copy for the verdict tests)."""

    def __init__(self, eng, models, streams=None):
        self.eng, self.models = eng, models
        self.streams = streams or [m.packed for m in models]
        self.n = len(models)
        self.H, self.W, self.C = models[0].H, models[0].W, models[0].C
        self.pic = self.H * self.W * self.C
        self.stride = (max(len(s) for s in self.streams) + 3 + 255) // 256 * 256
        self.states = [mm.state() for _ in models]
        self.d_state = torch.zeros(self.n * 16, dtype=torch.uint8, device="cuda")
        self.d_out = torch.full((self.n * self.pic + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.d_st = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.d_rows = torch.empty(self.n, dtype=torch.int32, device="cuda")

    def set_states(self, states):
        """Overwrite the device states (and the model's): the impossible ones."""
        self.states = [dict(s) for s in states]
        self.d_state.copy_(torch.from_numpy(_states_array(states).view(np.uint8)))

    def input(self, avails, tail="junk"):
        """Frame f holds streams[f][:avails[f]]; behind them, up to the stride, a pattern or random bytes."""
        if tail == "random":
            buf = np.random.default_rng(99).integers(0, 256, (self.n, self.stride), dtype=np.uint8)
        else:
            buf = np.full((self.n, self.stride), 0xA5, np.uint8)
        for f, s in enumerate(self.streams):
            buf[f, :avails[f]] = s[:avails[f]]
        return torch.from_numpy(buf).cuda()

    def call(self, d_in, avails, stream=0):
        self.eng.decode_prefix_more_device(d_in, self.stride, avails, self.n, self.W, self.H, self.C, self.d_state,
                                           self.d_out, self.d_rows, self.d_st, stream)

    def read(self):
        out = self.d_out.cpu().numpy()
        assert (out[self.n * self.pic:] == SENTINEL).all()
        states = np.frombuffer(self.d_state.cpu().numpy().tobytes(), himg_amd.PREFIX_STATE_DTYPE)
        return (self.d_st.cpu().numpy(), self.d_rows.cpu().numpy(), out[:self.n * self.pic].reshape(self.n, self.H, self.W, self.C),
                states)

    def step(self, avails, tail="junk", sentinel=True, verdicts=None, what=""):
        """One launch, checked.  sentinel: every byte of the pictures is the sentinel before the call (else the
        pictures persist, and a frame without a verdict must hold the prefix decode's whole picture behind it).
        verdicts: {frame: status word} for the frames fed damaged bytes -- that word, d_rows = -1, the state
        unchanged, nothing above block row k_prev touched.  Returns d_rows."""
        verdicts = verdicts or {}
        if sentinel:
            self.d_out.fill_(SENTINEL)
        self.d_st.fill_(-99)
        self.d_rows.fill_(-99)
        self.call(self.input(avails, tail), avails)
        torch.cuda.synchronize()
        st, rows, out, states = self.read()
        for f, (m, a) in enumerate(zip(self.models, avails)):
            old = self.states[f]
            tag = (what, f, a, old)
            code, k, written, new = mm.step(m, old, a)
            if f in verdicts:
                code, k, written, new = pm.FORMAT, -1, None, dict(old)
                assert st[f] == verdicts[f] and st[f] & 15 == 4, (tag, st[f], verdicts[f])
                if sentinel and old["started"]:
                    assert (out[f, :8 * old["rows_done"]] == SENTINEL).all(), tag
            elif code == pm.CAPACITY:
                assert st[f] == ST_SHORT, (tag, st[f])
            elif code == mm.ARG:
                assert st[f] == ST_ARG, (tag, st[f])
            else:
                assert code == 0 and st[f] == 0, (tag, code, st[f])
            assert rows[f] == k, (tag, rows[f], k)
            assert {n_: int(states[n_][f]) for n_ in new} == new, (tag, states[f], new)
            if f not in verdicts:
                if not sentinel:
                    if code == 0:
                        assert np.array_equal(out[f], m.picture(k)), tag
                elif code == 0 and not old["started"]:
                    assert written == (0, m.rows) and np.array_equal(out[f], m.picture(k)), tag
                else:
                    y0, y1 = (8 * written[0], min(8 * written[1], m.H)) if written else (0, 0)
                    assert np.array_equal(out[f, y0:y1], m.full[y0:y1]), tag
                    assert (out[f, :y0] == SENTINEL).all() and (out[f, y1:] == SENTINEL).all(), tag
            self.states[f] = new
        return rows


def _full(eng, streams, W, H, Cn):
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.zeros((n, stride), np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = s
    d_out = torch.full((n * H * W * Cn + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_device(torch.from_numpy(buf).cuda(), stride, [len(s) for s in streams], n, W, H, Cn, d_out, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_out.cpu().numpy()[:n * H * W * Cn].reshape(n, H, W, Cn)


def _prefix_status(eng, streams, avails, W, H, Cn):
    """himg_hip_decode_prefix_device's status words for these bytes: the reference of the verdict tests."""
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5, np.uint8)
    for i, s in enumerate(streams):
        buf[i, :avails[i]] = s[:avails[i]]
    d_out = torch.empty(n * H * W * Cn, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    d_rows = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    eng.decode_prefix_device(torch.from_numpy(buf).cuda(), stride, avails, n, W, H, Cn, d_out, d_rows, d_st)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rows.cpu().numpy()


def test_every_row_end_in_turn_and_skips(eng):
    """64 x 64, 8 rows.  Frame 0: fresh at head_bytes, then every row end in turn.  Frame 1: steps that skip
    rows, one that ends inside a payload (nothing written), one with avail unchanged."""
    m = _model("randtile", 64, 64)
    e = m.row_ends()
    assert len(e) == 9 and e[8] == m.T
    a0 = e
    a1 = [e[0], e[3], e[3] + 5, e[3] + 5, e[7], e[7] + 1, m.T, m.T, m.T]
    want1 = [0, 3, 3, 3, 7, 7, 8, 8, 8]
    for sentinel in (True, False):
        ch = Chain(eng, [m, m])
        for i, (x, y) in enumerate(zip(a0, a1)):
            rows = ch.step([x, y], sentinel=sentinel, what=("step", i, sentinel))
            assert list(rows) == [i, want1[i]]
    # the pictures kept across the whole chain are the full decode's
    st, full = _full(eng, [m.packed, m.packed], 64, 64, 4)
    assert (st == 0).all() and np.array_equal(ch.read()[2], full)


@pytest.mark.parametrize("W,H", [(4096, 32), (2048, 16), (1920, 24)])
def test_row_kernel_forms(eng, W, H):
    """The 512-, 256- and 240-column rows (under HIMG_OPT_FIX_T2, as in test_gpu_prefix): cuts at a row end,
    inside a payload, and at T."""
    eng.set_option("fix_t2", 1)
    m = _model("randtile", W, H, fix=True)
    e = m.row_ends()
    chains = [[e[0], e[1], (e[1] + e[2]) // 2, m.T],
              [(e[0] + e[1]) // 2, e[-2], e[-2], m.T],
              [e[1], m.T, m.T, m.T]]
    ch = Chain(eng, [m] * 3)
    for i in range(4):
        ch.step([c[i] for c in chains], what=(W, H, i))
    assert [s["rows_done"] for s in ch.states] == [m.rows] * 3


@pytest.mark.parametrize("wave", [-1, 0, 1])
def test_more_frames_than_cus(eng, wave):
    """300 frames of 256 x 72 (nine block rows, a single row in the last count group), three launches: fresh,
    resumed, idle and below-head frames side by side."""
    eng.set_option("count_wave", wave)
    ms = [_model("randtile", 256, 72, seed=s) for s in range(3)]
    rng = np.random.default_rng(5)
    n = 300
    models = [ms[f % 3] for f in range(n)]
    chains = []
    for f, m in enumerate(models):
        head, e = m.plan["head_bytes"], m.row_ends()
        a = sorted(int(x) for x in rng.integers(head, m.T + 1, 3))
        kind = f % 5
        if kind == 1:
            a = [head - 1, a[1], a[2]]            # below the head, then fresh, then resumed
        elif kind == 2:
            a = [a[0], a[0], a[2]]                # no new bytes in the second launch
        elif kind == 3:
            a = [11, head - 1, a[2]]              # below the head twice, then fresh
        elif kind == 4:
            a = [e[8], m.T, m.T]                  # the only new row is the last count group's single row
        chains.append(a)
    ch = Chain(eng, models)
    seen = []
    for i in range(3):
        rows = ch.step([c[i] for c in chains], what=(wave, i))
        seen.append(rows.copy())
    assert seen[0][4] == 8 and seen[1][4] == 9 and seen[2][4] == 9
    assert seen[0][1] == -1 and seen[1][3] == -1 and (seen[2] >= 0).all()


@pytest.mark.parametrize("wave", [0, 1])
def test_six_kinds_of_frame_in_one_launch(eng, wave):
    """Six frames of 72 x 40 x 3 (five block rows, q50) in ONE call, under both count kernels: fresh at half the
    stream, resumed with new rows, resumed with no new bytes, below the head (capacity), a state that cannot
    be right (argument), fresh at the whole stream (prefix_more_model.mixed_batch; its verdicts are checked on
    the host in test_prefix_more_host).  The frames share the launch's per-frame words and one gate: each must
    come out as the model says -- status, rows, state, picture, and the sentinel outside a resumed frame's new
    rows -- whatever its neighbours are."""
    eng.set_option("count_wave", wave)
    m = _model("randtile", 72, 40, 3)
    cases = mm.mixed_batch(m)
    want = [mm.step(m, st, a) for st, a, _ in cases]
    assert [x[0] for x in want] == [c[2] for c in cases] == [0, 0, 0, pm.CAPACITY, mm.ARG, 0]
    assert [x[2] for x in want] == [(0, 5), (1, 3), None, None, None, (0, 5)]
    ch = Chain(eng, [m] * 6)
    ch.set_states([c[0] for c in cases])
    rows = ch.step([c[1] for c in cases], what=("mixed", wave))
    assert list(rows) == [1, 3, 2, -1, -1, 5]
    st, _, out, _ = ch.read()
    assert list(st) == [0, 0, 0, ST_SHORT, ST_ARG, 0]
    assert (out[3] == SENTINEL).all() and (out[4] == SENTINEL).all()   # a verdict: nothing of the picture written
    assert ch.states[3] == cases[3][0] and ch.states[4] == cases[4][0]


@pytest.mark.parametrize("W,H,Cn,ycc,fix", [(100, 45, 3, True, False), (37, 19, 1, True, False), (72, 40, 3, False, False),
                                            (40, 8, 4, True, True)])
def test_ragged_shapes_and_few_channels(eng, W, H, Cn, ycc, fix):
    eng.set_option("fix_t2", int(fix))
    m = _model("randtile", W, H, Cn, 90, ycc, 3, fix)
    e = m.row_ends()
    if m.rows == 1:   # one block row, no size header: k goes 0 -> 1 with the chunk's last byte
        steps, want = [e[0], m.T - 1, m.T], [0, 0, 1]
    else:
        steps = sorted({e[0], e[1] + 1, e[2], m.T - 1, m.T})
        want = [m.expect(a)[1] for a in steps]
    ch = Chain(eng, [m])
    got = [int(ch.step([a], what=(W, H, Cn, a))[0]) for a in steps]
    assert got == want and got[-1] == m.rows


def test_four_byte_headers(eng):
    """4096 x 16 rand q100: steps that end between the two halves of a row's 4-byte header, then complete the
    row; random bytes behind avail."""
    m = _model("rand", 4096, 16, q=100, seed=7)
    e = m.row_ends()
    assert e[1] - e[0] > 0x8000 + 4 and len(e) == 3
    ch = Chain(eng, [m, m])
    got = [list(ch.step(a, tail="random", what=a)) for a in
           ([e[0] + 2, e[0]], [e[1], e[1] + 2], [e[1] + 2, e[1] + 3], [m.T, m.T])]
    assert got == [[0, 0], [1, 1], [1, 1], [2, 2]]


def test_below_the_head(eng):
    m = _model("randtile", 64, 64)
    head, e = m.plan["head_bytes"], m.row_ends()
    ch = Chain(eng, [m, m])
    got = [list(ch.step(a, what=a)) for a in ([head - 1, 0], [11, 100], [head, e[4]], [e[4], m.T])]
    assert got == [[-1, -1], [-1, -1], [0, 4], [4, 8]]
    assert ch.states[0] == mm.state(1, 4, e[4], e[4])


def _damaged(m):
    """Three damaged copies of m's stream (64 x 64): row 3's header overwritten so that the walk rejects it; a
    payload byte of row 3 the oracle decoder notices; the chunk cut behind row 5 (fewer blocks than rows).
    Each with the avail of the step that meets the damage."""
    e = m.row_ends()
    hdr = m.packed.copy()
    hdr[e[3]:e[3] + 4] = 0xFF          # a 4-byte header whose length crosses the chunk's end
    pay = None
    for off in range(e[3] + 6, e[4], 7):
        t = m.packed.copy()
        t[off] ^= 0x55
        if ol.oracle_decode(t)[0] != 0:
            pay = t
            break
    assert pay is not None
    o, size = sm.find_chunks(m.packed.tobytes())["FRES"]
    assert o + size == m.T
    cut = m.packed[:e[6]].copy()
    cut[4:8] = np.frombuffer(np.uint32(e[6] - 8).tobytes(), np.uint8)
    cut[o - 4:o] = np.frombuffer(np.uint32(e[6] - o).tobytes(), np.uint8)
    return [(hdr, e[5]), (pay, e[5]), (cut, e[6])]


def test_verdicts_in_the_new_bytes(eng):
    eng.set_option("fix_t2", 1)   # (the cut stream's FRES chunk may be smaller than a block row's symbols: trap T2)
    m = _model("randtile", 64, 64, fix=True)
    e = m.row_ends()
    bad = _damaged(m)
    streams = [m.packed, bad[0][0], m.packed, bad[1][0], bad[2][0], m.packed]
    ch = Chain(eng, [m] * 6, streams)
    assert list(ch.step([e[2]] * 6, what="first")) == [2] * 6   # the damage has not arrived
    avails = [e[5], bad[0][1], e[4], bad[1][1], bad[2][1], m.T]
    ref_st, ref_rows = _prefix_status(eng, streams, avails, 64, 64, 4)
    assert [int(x) & 15 for x in ref_st] == [0, 4, 0, 4, 4, 0] and list(ref_rows) == [5, -1, 4, -1, -1, 8]
    verdicts = {f: int(ref_st[f]) for f in (1, 3, 4)}
    for again in range(2):   # the state is unchanged: the call repeats with the same verdict
        rows = ch.step(avails, verdicts=verdicts, what=("verdict", again))
        assert list(rows) == [5, -1, 4, -1, -1, 8]
        assert [ch.states[f] for f in (1, 3, 4)] == [mm.state(1, 2, e[2], e[2])] * 3


def test_impossible_states(eng):
    m = _model("randtile", 64, 64)
    e, head = m.row_ends(), m.plan["head_bytes"]
    good = mm.state(1, 2, e[2], e[2])
    cases = [(good, e[5]),                                   # a healthy neighbour
             (good, e[2] - 1),                               # avail below avail_seen
             (mm.state(1, -1, e[2], e[2]), e[5]),            # rows_done < 0
             (mm.state(1, m.rows + 1, e[2], e[2]), e[5]),    # rows_done > rows
             (mm.state(1, 0, head - 1, head - 1), e[5]),     # walk_pos below the first row header
             (mm.state(1, 8, m.T + 1, e[2]), m.T),           # walk_pos beyond the chunk's end
             (mm.state(1, 3, e[3], e[1]), e[2]),             # walk_pos beyond avail
             (good, m.T)]                                    # a healthy neighbour
    ch = Chain(eng, [m] * len(cases))
    ch.step([e[2]] * len(cases), what="first")
    ch.set_states([c[0] for c in cases])
    rows = ch.step([c[1] for c in cases], what="impossible")
    assert list(rows) == [5, -1, -1, -1, -1, -1, -1, 8]
    assert ch.states[1:7] == [c[0] for c in cases[1:7]]


def test_argument_errors(eng):
    m = _model("randtile", 64, 64)
    ch = Chain(eng, [m])
    d_in = ch.input([m.T])
    for d_state in (None, ch.d_state.data_ptr() + 4):
        with pytest.raises(himg_amd.HimgError) as err:
            eng.decode_prefix_more_device(d_in, ch.stride, [m.T], 1, 64, 64, 4, d_state, ch.d_out, ch.d_rows, ch.d_st)
        assert err.value.code == himg_amd.HIMG_ERR_ARG
    with pytest.raises(himg_amd.HimgError) as err:   # what decode_prefix_device refuses: a stride below avail
        eng.decode_prefix_more_device(d_in, 256, [m.T], 1, 64, 64, 4, ch.d_state, ch.d_out, ch.d_rows, ch.d_st)
    assert err.value.code == himg_amd.HIMG_ERR_ARG
    torch.cuda.synchronize()
    st, rows, out, states = ch.read()
    assert (out == SENTINEL).all() and states[0] == himg_amd.prefix_states(1)[0]   # nothing launched


def test_two_calls_back_to_back_on_a_callers_stream(eng):
    """Two calls queued on a caller's non-blocking stream with no host wait between them: the second consumes
    the state the first wrote.  The stream is held shut while both are queued (tests/stream_gate.py); the
    results are those of the synchronised chain."""
    m, decoy_m = _model("randtile", 256, 72), _model("randtile", 256, 72, seed=1)
    e = m.row_ends()
    a1, a2 = e[3] + 1, e[7]
    ref = Chain(eng, [m])
    ref.step([a1], sentinel=False)
    ref.step([a2], sentinel=False)
    want = ref.read()

    stride = ref.stride
    real = np.full(stride, 0xA5, np.uint8)
    real[:a2] = m.packed[:a2]
    decoy = np.full(stride, 0xA5, np.uint8)
    decoy[:min(decoy_m.T, stride)] = decoy_m.packed[:stride]
    buf = sg.Buffers(torch, real, decoy, {"out": (ref.pic, SENTINEL), "state": (16, 0), "rows": (4, 0xEE), "st": (4, 0xEE)})
    gate = sg.Gate(log=lambda s: None)
    S = torch.cuda.Stream()

    def queue():
        d = {k: v[0] for k, v in buf.outs.items()}
        for a in (a1, a2):
            eng.decode_prefix_more_device(buf.d_in, stride, [a], 1, 256, 72, 4, d["state"], d["out"], d["rows"], d["st"],
                                          S.cuda_stream)

    # warm-up on the very stream, for the calls' host time
    buf.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        buf.queue_input()
        host = sg.timed_call(queue)
    S.synchronize()
    buf.reset()
    torch.cuda.synchronize()
    opened = gate.shut(S, sg.gate_ms(host))
    with torch.cuda.stream(S):
        buf.queue_input()
        queue()
        buf.queue_collect()
        done = torch.cuda.Event()
        done.record(S)
    still_shut = not opened.query()
    done.synchronize()
    assert still_shut, "the calls waited for the device"
    assert np.array_equal(buf.result("out").reshape(72, 256, 4), want[2][0])
    assert np.array_equal(buf.result("out").reshape(72, 256, 4), m.picture(7))
    assert buf.result("st").view(np.int32)[0] == 0 and buf.result("rows").view(np.int32)[0] == 7
    assert buf.result("state").tobytes() == want[3].tobytes()
    torch.cuda.synchronize()


def test_host_form(eng):
    m = _model("randtile", 100, 45, 3, 90, True, 3)
    e = m.row_ends()
    state = himg_amd.prefix_states(1)
    model_st = mm.state()
    dst = np.full((45, 100, 3), SENTINEL, np.uint8)
    for a in (e[0], e[2] + 1, e[2] + 1, e[3], m.T - 1, m.T):
        piece = m.packed[:a].copy()                       # exactly the bytes present: nothing behind them exists
        code, k, written, model_st = mm.step(m, model_st, a)
        fresh = not state["started"][0]
        if not fresh:
            dst[:] = SENTINEL
        pic, got_k = eng.decode_prefix_more(piece, state[0:1], dst)
        assert pic.ctypes.data == dst.ctypes.data and code == 0 and got_k == k, a
        assert {n_: int(state[n_][0]) for n_ in model_st} == model_st, a
        if fresh:
            assert np.array_equal(dst, m.picture(k)), a
        else:
            y0, y1 = (8 * written[0], min(8 * written[1], 45)) if written else (0, 0)
            assert np.array_equal(dst[y0:y1], m.full[y0:y1]), a
            assert (dst[:y0] == SENTINEL).all() and (dst[y1:] == SENTINEL).all(), a
    # a chain on one persistent picture ends as Engine.decode
    state, dst = himg_amd.prefix_states(1), None
    for a in (e[1], e[1] + 3, e[4], m.T):
        dst, k = eng.decode_prefix_more(m.packed[:a].copy(), state[0:1], dst)
    assert k == m.rows and np.array_equal(dst, eng.decode(m.packed))
    # a too-small dst: HIMG_ERR_CAPACITY with the geometry, nothing decoded, the state unchanged
    import ctypes as C
    L = himg_amd.lib()
    state = himg_amd.prefix_states(1)
    pic, k = eng.decode_prefix_more(m.packed[:e[2]].copy(), state[0:1])
    before, kept = state.copy(), pic.copy()
    w, h, c, kk = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    for dptr, cap in ((None, 0), (pic.ctypes.data, pic.nbytes - 1)):
        rc = L.himg_hip_decode_prefix_more_to(eng._ctx, m.packed.ctypes.data, e[5], state.ctypes.data, dptr, cap,
                                              C.byref(w), C.byref(h), C.byref(c), C.byref(kk))
        assert rc == himg_amd.HIMG_ERR_CAPACITY and (w.value, h.value, c.value, kk.value) == (100, 45, 3, -1)
        assert np.array_equal(state, before) and np.array_equal(pic, kept)
    # a state that cannot be right; below the head
    with pytest.raises(himg_amd.HimgError) as err:
        eng.decode_prefix_more(m.packed[:e[2] - 1].copy(), state[0:1], pic)
    assert err.value.code == himg_amd.HIMG_ERR_ARG and np.array_equal(state, before)
    with pytest.raises(himg_amd.HimgError) as err:
        eng.decode_prefix_more(m.packed[:e[0] - 1].copy(), himg_amd.prefix_states(1)[0:1])
    assert err.value.code == himg_amd.HIMG_ERR_CAPACITY


def test_goldens_in_four_steps(eng):
    """Goldens of at most 64 x 64 RGBA: four equal byte steps ending at T give decode_device's status and
    bytes, under both fix_t2 settings."""
    names = [n for n in gu.cases(max_pixels=64 * 64) if "fixture" in gu.GOLDEN[n] and gu.GOLDEN[n]["channels"] == 4]
    streams = [gu.fixture(gu.GOLDEN[n]) for n in names]
    n = len(streams)
    stride = (max(len(s) for s in streams) + 3 + 255) // 256 * 256
    buf = np.full((n, stride), 0xA5, np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = s
    d_in = torch.from_numpy(buf).cuda()
    for fix in (0, 1):
        eng.set_option("fix_t2", fix)
        st0, out0 = _full(eng, streams, 64, 64, 4)
        d_state = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_out = torch.full((n * 64 * 64 * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        d_rows = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        for q in (1, 2, 3, 4):
            avails = [len(s) * q // 4 for s in streams]
            eng.decode_prefix_more_device(d_in, stride, avails, n, 64, 64, 4, d_state, d_out, d_rows, d_st)
        torch.cuda.synchronize()
        st, rows, out = d_st.cpu().numpy(), d_rows.cpu().numpy(), d_out.cpu().numpy().reshape(n, 64, 64, 4)
        assert np.array_equal(st, st0), (fix, names, st, st0)
        assert (st0 == 0).any()
        for f in range(n):
            if st0[f] == 0:
                assert rows[f] == 8 and np.array_equal(out[f], out0[f]), (fix, names[f])
            else:
                assert rows[f] == -1, (fix, names[f])
