"""GPU (-m gpu): long codes through the whole encoder.  The pictures of tests/deep_pictures.py have token
histograms whose trees are 22 to 32 levels deep (tests/test_deep_pictures_host.py: what they reach), so
codes of 20 to 32 bits, and run tokens of up to 40 bits with their extra bits, go through k_span_bits,
k_sizes, the size probe and every form of the bit packer: the default engine (k_emit_t<1, true> for a
single wide frame, k_emit_t<1> for a narrow one and for the batch of three), HIMG_EMIT_ROWS=1
(k_emit_t<8>), HIMG_EMIT_ROWS=0 and HIMG_ROW_TOKENS=1 (k_tok -> k_emit_tok<8>).  Judge: the CPU oracle, byte
for byte; the decoders (fused and HIMG_FORCE_UNFUSED=1) then read the deep stream back to the oracle's
pixels."""
import os

import numpy as np
import pytest

import himg_amd
import oracle_lib as ol
import deep_pictures as dp

pytestmark = pytest.mark.gpu

KNOBS = {"default": {}, "emit_rows_1": {"HIMG_EMIT_ROWS": "1"}, "emit_rows_0": {"HIMG_EMIT_ROWS": "0"},
         "row_tokens_1": {"HIMG_ROW_TOKENS": "1"}, "unfused": {"HIMG_FORCE_UNFUSED": "1"}}


@pytest.fixture(scope="module")
def engines():
    """One context per knob, the environment set around its creation only."""
    made = {}
    for name, env in KNOBS.items():
        os.environ.update(env)
        try:
            made[name] = himg_amd.Engine(0)
        finally:
            for k in env:
                del os.environ[k]
    yield made
    for e in made.values():
        e.close()


def _eq(a, b, what):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    assert a.size == b.size, "%s: size %d vs %d" % (what, a.size, b.size)
    d = np.flatnonzero(a != b)
    assert d.size == 0, "%s: %d mismatches, first at %d (gpu=%s oracle=%s)" % (what, d.size, d[0], a[d[0]], b[d[0]])


@pytest.mark.parametrize("name", dp.NAMES)
def test_deep_picture_through_every_emit_form(engines, name):
    import torch
    img, _, want, tr = dp.traced(name)
    h, w, ch = img.shape
    q, ycc = dp.QUALITY, dp.USE_YCBCR
    side = himg_amd.synth("randtile", 3, w, h)                   # an ordinary frame on either side of the deep one
    side_want = ol.oracle_encode(side, q, ycc)
    d_frames = torch.from_numpy(img[None]).cuda()
    for knob in ("default", "emit_rows_1", "emit_rows_0", "row_tokens_1"):
        eng, what = engines[knob], "%s, %s" % (name, knob)
        _eq(eng.encode(img, q, ycc), want, what + ": stream")
        for k in ("lres_len", "fres_len"):
            _eq(eng.debug_read(k, 0, 261 * 4, np.uint32), tr[k], what + ": " + k)
        for k in ("lres_code", "fres_code"):
            _eq(eng.debug_read(k, 0, 261 * 8, np.uint64), tr[k], what + ": " + k)
        _eq(eng.debug_read("fres_row_bytes", 0, tr["rows"] * 4, np.uint32), tr["fres_row_bytes"], what + ": row payload bytes")
        # the size probe
        d_sizes = torch.full((1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_st = torch.full((1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        eng.encode_sizes_device(d_frames, 1, w, h, ch, ch, [q], ycc, d_sizes, d_st)
        torch.cuda.synchronize()
        assert int(d_st[0]) == 0 and int(d_sizes[0]) == want.size, (what, int(d_st[0]), int(d_sizes[0]), want.size)
        # frame 1 of a batch of three
        streams = eng.encode_batch([side, img, side], q, ycc)
        _eq(streams[0], side_want, what + ": batch frame 0")
        _eq(streams[1], want, what + ": batch frame 1 (deep)")
        _eq(streams[2], side_want, what + ": batch frame 2")


@pytest.mark.parametrize("name", dp.NAMES)
def test_deep_stream_decodes_to_the_oracles_pixels(engines, name):
    _, _, want, _ = dp.traced(name)
    rc, pix = ol.oracle_decode(want)
    assert rc == 0, "the oracle reads its own deep stream (tests/golden/deep_reach.json)"
    for knob in ("default", "unfused"):
        _eq(engines[knob].decode(want), pix, "%s, %s decoder: pixels" % (name, knob))
