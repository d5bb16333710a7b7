"""Arithmetic and comparisons for tests/test_gpu_far_addresses.py: buffers whose byte offsets pass
2^32.  Pure Python over torch tensors of any device, so tests/test_far_model_host.py runs every
function on CPU tensors with the chunk size and the modulus scaled down.

  - dense_batch: the smallest batch of tight frames with two whole frames beyond the boundary;
  - assert_far: the offsets a test checks do pass 2^32, and one lies in [2^31, 2^32) (the signed case);
  - extent / window_spans: the bytes of windows in pitched pictures (include/himg_hip.h's formula);
  - check_buffer: a WHOLE buffer against its expectation -- the windows' bytes where windows lie, the
    sentinel everywhere else, the tail included -- in chunks, with no full-size temporary;
  - check_dense: tight frames against a few expected frames, frame by frame, and the tail;
  - need_*: the device memory a test takes.

A mismatch is reported with its byte offset, that offset modulo 2^32 and the frame it falls in: a
store that wrapped is then readable from the message.

Test infrastructure only.
"""
import torch

WRAP = 1 << 32                 # where a 32-bit offset wraps
FAR_STRIDE = (1 << 30) + 256   # in_stride / out_stride of the far tests: a multiple of 256
FAR_PITCH = (1 << 30) + 260    # frame_pitch, 4-byte pixels (a multiple of 4, none of 16); + 1: odd, for 3-byte pixels
FAR_ROW_PITCH = (1 << 26) + 4  # row_pitch: y * row_pitch passes 2^32 at y = 64; + 1: odd, for 3-byte pixels
FAR_BATCH = 5                  # frame 4 starts beyond 2^32, frames 2 and 3 in [2^31, 2^32)
TAIL = 64
SENTINEL = 0xA5
CHUNK = 1 << 30
K = 3                          # distinct pictures; frame f holds picture f % K
DENSE = 2048                   # side of the dense tests' RGBA frames
MAX_REPORTS = 6


# ---- arithmetic -----------------------------------------------------------------------------------

def dense_batch(frame_bytes, wrap=WRAP):
    """The smallest batch with batch * frame_bytes >= wrap + 2 * frame_bytes: at least two whole
    frames start at or beyond the boundary."""
    assert frame_bytes > 0
    return -(-wrap // frame_bytes) + 2


def assert_far(offsets, wrap=WRAP, whole_beyond=1):
    """The offsets (of frames, rows or windows) that a test checks: at least `whole_beyond` of them at
    or beyond `wrap`, and at least one in [wrap / 2, wrap)."""
    offsets = list(offsets)
    beyond = [o for o in offsets if o >= wrap]
    signed = [o for o in offsets if wrap // 2 <= o < wrap]
    assert len(beyond) >= whole_beyond, "only %d of %d offsets reach %d (largest %d)" % (
        len(beyond), len(offsets), wrap, max(offsets))
    assert signed, "no offset in [%d, %d)" % (wrap // 2, wrap)
    return beyond, signed


def extent(frame_pitch, row_pitch, pixel_stride, origins, w, h):
    """The bytes that the w x h windows at origins[f] = (x_f, y_f) of picture f reach (himg_hip_dst_extent,
    himg_hip_windows_extent): the largest f * frame_pitch + (y_f + h - 1) * row_pitch + (x_f + w) * pixel_stride."""
    return max(f * frame_pitch + (y + h - 1) * row_pitch + (x + w) * pixel_stride for f, (x, y) in enumerate(origins))


def encoder_clears(w, h, channels):
    """Where the bytes end that the encoder clears in every output slot before it packs (include/himg_hip.h,
    himg_hip_encode_device): the worst-case extent of the low-res chunk -- 172 bytes of head, the low-res
    plane and its 16-fold reduction, a tree's 384 bytes and 64 more, rounded up to 4.  A slot's bytes between
    the end of a shorter stream and this offset are unspecified (zeros); behind it nothing is written."""
    rows, cols = (h + 7) // 8, (w + 7) // 8
    plane = channels * (rows * cols + ((rows + 15) // 16) * ((cols + 15) // 16))
    return (172 + plane + 384 + 64 + 3) & ~3


def window_base(frame_pitch, row_pitch, pixel_stride, f, x, y):
    return f * frame_pitch + y * row_pitch + x * pixel_stride


def window_spans(base, rows, row_pitch):
    """[(offset, bytes)] of a window whose rows (a 2-D uint8 tensor: h x row bytes) lie row_pitch apart
    from `base` on."""
    return [(base + i * row_pitch, rows[i]) for i in range(rows.shape[0])]


def need(buffers, workspace, chunk=CHUNK):
    """Device bytes of a test: its tensors, the library's workspace (measured; it is not torch's), and the
    comparison's temporaries -- an expected chunk, and a difference mask and its cast when a chunk differs."""
    return int(sum(buffers)) + int(workspace) + 3 * chunk


# Workspace of the module's engine: the free-memory drop across the calls that torch's own allocations
# do not explain, measured on an MI355X (rounded up to a GiB).  A context keeps the largest it has seen.
WORKSPACE_FAR = 1 << 30            # five frames of at most 512 x 64: below 0.01 GiB measured
WORKSPACE_DENSE_DECODE = 5 << 30   # 260 frames of 2048 x 2048 x 4, every decode form: 4.80 GiB measured
WORKSPACE_DENSE_ENCODE = 13 << 30  # 258 frames of 2048 x 2048 x 4, front = 1, row_tokens = 1: 12.49 GiB measured


def need_far(*buffers):
    """Section A: the 5 GiB far buffer(s) and small change."""
    return need(buffers, WORKSPACE_FAR)


def need_dense_decode(batch, stream_stride, out_bytes, expected_bytes):
    return need([batch * stream_stride, K * stream_stride, out_bytes + TAIL, expected_bytes],
                WORKSPACE_DENSE_DECODE + WORKSPACE_DENSE_ENCODE)


def need_dense_encode(batch, frame_bytes, out_stride):
    return need([batch * frame_bytes, K * frame_bytes, batch * out_stride + TAIL], WORKSPACE_DENSE_DECODE + WORKSPACE_DENSE_ENCODE)


def conceal_one_row(model, bad, r):
    """conceal_model.expect for a stream whose damage lies inside block row r's payload alone, with ONE
    oracle run instead of one per block row (2048 x 2048 has 256): the headers are the good stream's, so
    every other row is judged with the good payload and holds the good pixels, and row r's own verdict is
    the damaged stream's.  model: prefix_model.Model(good).  tests/test_far_model_host.py holds it against
    conceal_model.expect."""
    import numpy as np

    import oracle_lib as ol
    rc, img = ol.oracle_decode(bad, fix_t2=model.fix_t2)
    out, rowmap = model.full.reshape(model.H, model.W, model.C).copy(), np.zeros(model.rows, np.uint8)
    if rc != 0:
        out[8 * r:8 * r + 8] = model.fill[8 * r:8 * r + 8]
        rowmap[r] = 1
    else:
        out[8 * r:8 * r + 8] = img[8 * r:8 * r + 8]
    return out, rowmap


# ---- comparisons ----------------------------------------------------------------------------------

def where(offset, pitch=None, wrap=WRAP):
    """'byte 4294968320 (= 1024 mod 2^32) of frame 4': pitch = bytes from a frame to the next (None: no frames)."""
    s = "byte %d (= %d mod %d)" % (offset, offset % wrap, wrap)
    if pitch:
        s += " in frame %d" % (offset // pitch)
    return s


def _first_difference(got, want):
    ne = got != want
    i = int(ne.to(torch.uint8).argmax())
    return i, int(ne.sum()), int(got[i]), int(want[i])


def check_buffer(buf, spans, what, pitch=None, sentinel=SENTINEL, chunk=CHUNK, wrap=WRAP):
    """Every byte of the 1-D uint8 tensor `buf`: the spans' bytes ([(offset, 1-D uint8 tensor)], disjoint,
    on buf's device) where spans lie, `sentinel` everywhere else.  Compared in chunks of `chunk` bytes; the
    first difference of every chunk that differs is reported (MAX_REPORTS at the most), so a span that was
    written at its offset modulo `wrap` shows twice: where it landed and where it is missing."""
    n = buf.numel()
    spans = sorted(((int(o), t.reshape(-1)) for o, t in spans), key=lambda s: s[0])
    end = 0
    for o, t in spans:
        assert t.dtype == torch.uint8 and o >= end and o + t.numel() <= n, (what, "span", o, t.numel(), end, n)
        end = o + t.numel()
    scratch = torch.empty(min(chunk, n), dtype=torch.uint8, device=buf.device)
    reports, total, k = [], 0, 0
    for c0 in range(0, n, chunk):
        c1 = min(c0 + chunk, n)
        want = scratch[:c1 - c0]
        want.fill_(sentinel)
        while k < len(spans) and spans[k][0] + spans[k][1].numel() <= c0:
            k += 1
        j = k
        while j < len(spans) and spans[j][0] < c1:
            o, t = spans[j]
            a, e = max(o, c0), min(o + t.numel(), c1)
            want[a - c0:e - c0] = t[a - o:e - o]
            j += 1
        got = buf[c0:c1]
        if torch.equal(got, want):
            continue
        i, cnt, g, w = _first_difference(got, want)
        total += cnt
        if len(reports) < MAX_REPORTS:
            inside = any(o <= c0 + i < o + t.numel() for o, t in spans[k:j])
            reports.append("%s: got %#04x, expected %#04x (%s)" % (where(c0 + i, pitch, wrap), g, w,
                                                                   "a window's byte" if inside else "the sentinel"))
    if reports:
        raise AssertionError("%s: %d of %d bytes differ; the first of each chunk that differs: %s"
                             % (what, total, n, "; ".join(reports)))


def check_dense(buf, frame_bytes, batch, wants, what, sentinel=SENTINEL, wrap=WRAP):
    """Tight frames: frame f of the 1-D uint8 tensor `buf` (batch * frame_bytes + TAIL bytes) against
    wants[f % len(wants)] (uint8 tensors of frame_bytes bytes; or a function of f that returns one), then
    the tail against the sentinel.  A frame that differs is reported with its first differing byte and,
    where it holds one, the number of the expected picture that it does hold."""
    assert buf.numel() == batch * frame_bytes + TAIL, (what, buf.numel(), batch, frame_bytes)
    table = [] if callable(wants) else [w.reshape(-1) for w in wants]
    reports, bad = [], 0
    for f in range(batch):
        got = buf[f * frame_bytes:(f + 1) * frame_bytes]
        want = table[f % len(table)] if table else wants(f).reshape(-1)
        if torch.equal(got, want):
            continue
        bad += 1
        if len(reports) < MAX_REPORTS:
            i, cnt, g, w = _first_difference(got, want)
            holds = [str(k) for k, other in enumerate(table) if torch.equal(got, other)]
            reports.append("frame %d%s, %d bytes, first at %s: got %#04x, expected %#04x"
                           % (f, ", which holds picture %s, not %d" % (holds[0], f % len(table)) if holds else "", cnt,
                              where(f * frame_bytes + i, frame_bytes, wrap), g, w))
    tail = buf[batch * frame_bytes:]
    if not bool((tail == sentinel).all()):
        i = int((tail != sentinel).to(torch.uint8).argmax())
        reports.append("the tail, first at %s: got %#04x" % (where(batch * frame_bytes + i, None, wrap), int(tail[i])))
        bad += 1
    if reports:
        raise AssertionError("%s: %d of %d frames (or the tail) differ: %s" % (what, bad, batch, "; ".join(reports)))
