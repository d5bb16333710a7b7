"""GPU (-m gpu): FRES rows through the token stream (k_tok -> k_emit_tok, what batches take)
against the CPU oracle: final bytes, the slots expanded into symbols again, the histogram --
on shapes and contents that exercise every kind of slot (literals behind 0..255 zeros, runs on
their own incl. the reference's greedy split at 16 662, trailing zeros of a row, dense
iterations staged in two parts) and both paths of the bit packer.  Bar: bit-exact."""
import numpy as np
import pytest

import himg_amd
import oracle_lib as ol
import tok_model as tm

pytestmark = pytest.mark.gpu


def _images(w, h):
    yield "randtile", himg_amd.synth("randtile", 1, w, h)
    yield "rand", himg_amd.synth("rand", 3, w, h)              # dense: iterations beyond the staging buffer
    z = np.zeros((h, w, 4), np.uint8)
    yield "zero", z                                             # a row is ONE run: the split at 16 662
    s = z.copy()
    s[h // 2:, :, :] = himg_amd.synth("rand", 4, w, h)[h // 2:, :, :]
    s[: h // 2, w - 9, 1] = 200                                 # a lone column of detail: runs of hundreds of zeros
    yield "sparse", s


SHAPES = [(512, 64), (1024, 72), (4096, 64), (1920, 136), (200, 72), (2048, 40)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_token_stream_encode_matches_oracle(w, h):
    eng = himg_amd.Engine(0)
    for name, img in _images(w, h):
        for q, ycc in ((50, True), (90, False), (100, True), (10, True)):
            want, tr = ol.oracle_encode(img, q, ycc, trace=True)
            for mode in (1, 2):   # 2: the bit packer's spelled-out path on every step
                eng.set_option("row_tokens", mode)
                got = eng.encode(img, q, ycc)
                assert got.size == want.size and np.array_equal(got, want), (name, q, ycc, mode)
            sym = eng.debug_read("fres_tok_sym", 0, tr["fres_sym"].size)
            assert np.array_equal(sym, tr["fres_sym"]), (name, q, ycc, "slots expanded")
            assert np.array_equal(eng.debug_read("fres_hist", 0, 261 * 4, np.uint32), tr["fres_hist"]), (name, q, ycc)
            _check_slots(eng, 0, tr, w, h, (name, q, ycc))
    eng.close()


def test_token_stream_other_channel_counts():
    """1-3 channels and a pixel stride beyond the channel count go through k_tile_fwd, then the same slots."""
    eng = himg_amd.Engine(0)
    eng.set_option("row_tokens", 1)
    base = himg_amd.synth("randtile", 7, 264, 80)
    for ch, stride in ((1, 1), (2, 2), (3, 3), (3, 4), (1, 4)):
        img = np.ascontiguousarray(base[:, :, :stride])
        want = ol.oracle_encode(img, 50, True, channels=ch, stride=stride)
        got = eng.encode(img, 50, True, channels=ch, pixel_stride=stride)
        assert np.array_equal(got, want), (ch, stride)
    eng.close()


def test_token_stream_is_what_batches_take():
    """The default (-1) chooses the slots by launch size: a batch of >= 8192 block rows takes them, a
    single frame does not; either way the streams are the oracle's."""
    import torch
    eng = himg_amd.Engine(0)
    assert eng.get_option("row_tokens") == -1
    w, h, B = 1024, 512, 128                       # 64 rows x 128 frames = 8192 block rows
    frames = np.stack([himg_amd.synth("randtile", s, w, h) for s in range(B)])
    d_frames = torch.from_numpy(frames).cuda()
    cap = himg_amd.max_packed_size(w, h, 4)
    d_out = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_st = torch.ones(B, dtype=torch.int32, device="cuda")
    eng.profile(True)
    eng.encode_device(d_frames, B, w, h, 4, 4, 50, True, d_out, cap, d_sizes, d_st)
    torch.cuda.synchronize()
    stages = eng.profile_read()
    assert "k_tok" in stages and "k_emit_tok" in stages, sorted(stages)
    assert not d_st.cpu().numpy().any()
    sizes = d_sizes.cpu().numpy()
    for f in (0, 1, B // 2, B - 1):
        want = ol.oracle_encode(frames[f], 50, True)
        assert int(sizes[f]) == want.size and np.array_equal(d_out[f, : want.size].cpu().numpy(), want), f
    # the expanded slots of a frame in the middle of the batch
    _, tr = ol.oracle_encode(frames[B // 2], 50, True, trace=True)
    assert np.array_equal(eng.debug_read("fres_tok_sym", B // 2, tr["fres_sym"].size), tr["fres_sym"])
    eng.profile_reset()
    eng.encode_device(d_frames[:1], 1, w, h, 4, 4, 50, True, d_out, cap, d_sizes, d_st)
    torch.cuda.synchronize()
    stages = eng.profile_read()
    assert "k_tok" not in stages and "k_emit" in stages, sorted(stages)
    eng.close()


def _model_counts(tr, w, h, ch=4):
    lay = himg_amd.tok_layout(w, h, ch, row_tokens=1)
    counts, worst = tm.frame_demand(tr["fres_sym"], tr["rows"], lay["seg"], lay["nseg"], lay["stage"])
    assert tm.padded(counts).max() <= lay["cap"] and worst <= lay["stage"], (w, h, "the model outgrows the product's bound")
    return counts


def _check_slots(eng, frame, tr, w, h, what):
    """What k_tok left for one frame of the last encode: the slots expanded into symbols again, and the
    slot count of every segment against the model's (tests/tok_model.py) -- slot for slot."""
    sym = eng.debug_read("fres_tok_sym", frame, tr["fres_sym"].size)
    assert np.array_equal(sym, tr["fres_sym"]), (what, "slots expanded")
    counts = _model_counts(tr, w, h)
    cnt = eng.debug_read("tok_cnt", frame, counts.size * 4, np.uint32)
    assert np.array_equal(cnt.reshape(counts.shape), counts), (what, "tok_cnt")


WIDE_SHAPES = [(8192, 24), (16384, 24)]


@pytest.mark.parametrize("w,h", WIDE_SHAPES)
def test_token_stream_wide_rows_match_oracle(w, h):
    """The file's pictures at widths nothing forced the token stream at before (a row of the all-zero
    picture is 16 and 32 pieces of a run; the lone column sits behind runs of tens of thousands)."""
    eng = himg_amd.Engine(0)
    eng.profile(True)
    for name, img in _images(w, h):
        for q, ycc in ((50, True), (90, False), (100, True), (10, True)):
            want, tr = ol.oracle_encode(img, q, ycc, trace=True)
            for mode in (1, 2):
                eng.set_option("row_tokens", mode)
                eng.profile_reset()
                got = eng.encode(img, q, ycc)
                stages = eng.profile_read()
                assert "k_tok" in stages and "k_emit_tok" in stages and "k_tok_hist" not in stages, sorted(stages)
                assert got.size == want.size and np.array_equal(got, want), (name, q, ycc, mode)
            _check_slots(eng, 0, tr, w, h, (name, q, ycc))
            assert np.array_equal(eng.debug_read("fres_hist", 0, 261 * 4, np.uint32), tr["fres_hist"]), (name, q, ycc)
    eng.close()


CRAFTED_WIDTHS = [12288, 16384, 20480, 32768]


@pytest.mark.parametrize("w", CRAFTED_WIDTHS)
@pytest.mark.parametrize("variant", tm.VARIANTS)
def test_crafted_wide_rows_match_oracle(variant, w):
    """The pictures of tests/tok_model.py: block rows whose one dense segment sits behind a run of most of a
    row, so that it needs its symbol count plus three slots per 16 662 zeros in front -- more than the 64
    spare slots a segment had whatever the width (16384 pixels: 65 620 against 65 600; 12288 pixels:
    exactly the 49 216).  Forced through the token stream, both paths of the bit packer; a width whose
    half-iteration could outgrow k_tok's stage (himg_dev.h tok_stage_need: 32768 pixels) keeps the kernels
    over the dense plane, forced or not.  Stream, symbols, histogram and the slot counts against the
    oracle and the model; then a device batch of three -- the picture, an ordinary frame, the picture --
    so that slots written past a segment would have a neighbour (the next frame's rows, tok_cnt) to damage;
    then the decode: the reference rejects its own streams of these pictures (trap T2), and so must the
    engine, and with fix_t2 it gives the oracle's pixels."""
    import torch
    h = tm.crafted_height(w)
    img = tm.crafted(variant, w, h)
    lay = himg_amd.tok_layout(w, h, 4, row_tokens=1)
    assert lay["tokens"] == (w <= 20480)
    want, tr = ol.oracle_encode(img, 100, False, trace=True)
    eng = himg_amd.Engine(0)
    eng.profile(True)
    for mode in (1, 2):
        eng.set_option("row_tokens", mode)
        eng.profile_reset()
        got = eng.encode(img, 100, False)
        stages = eng.profile_read()
        if lay["tokens"]:
            assert "k_tok" in stages and "k_emit_tok" in stages and "k_tok_hist" not in stages, sorted(stages)
        else:
            assert "k_tok_hist" in stages and "k_emit" in stages, sorted(stages)
            assert "k_tok" not in stages and "k_emit_tok" not in stages, sorted(stages)
        assert got.size == want.size and np.array_equal(got, want), (variant, w, mode)
        if lay["tokens"]:
            _check_slots(eng, 0, tr, w, h, (variant, w, mode))
        assert np.array_equal(eng.debug_read("fres_sym", 0, tr["fres_sym"].size), tr["fres_sym"]), (variant, w, mode)
        assert np.array_equal(eng.debug_read("fres_hist", 0, 261 * 4, np.uint32), tr["fres_hist"]), (variant, w, mode)
    # a device batch: picture, neighbour, picture
    other = himg_amd.synth("randtile", 5, w, h)
    want_o, tr_o = ol.oracle_encode(other, 100, False, trace=True)
    frames = np.stack([img, other, img])
    d_frames = torch.from_numpy(frames).cuda()
    cap = himg_amd.max_packed_size(w, h, 4)
    d_out = torch.zeros((3, cap), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_st = torch.ones(3, dtype=torch.int32, device="cuda")
    eng.set_option("row_tokens", 1)
    eng.encode_device(d_frames, 3, w, h, 4, 4, 100, False, d_out, cap, d_sizes, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    sizes = d_sizes.cpu().numpy()
    for f, (wb, trf) in enumerate(((want, tr), (want_o, tr_o), (want, tr))):
        assert int(sizes[f]) == wb.size and np.array_equal(d_out[f, : wb.size].cpu().numpy(), wb), (variant, w, "batch", f)
        if lay["tokens"]:
            _check_slots(eng, f, trf, w, h, (variant, w, "batch", f))
        assert np.array_equal(eng.debug_read("fres_hist", f, 261 * 4, np.uint32), trf["fres_hist"]), (variant, w, "batch", f)
    del d_frames, d_out
    # the decode
    rc, _ = ol.oracle_decode(want)
    assert rc == -7, rc
    rc, px = ol.oracle_decode(want, fix_t2=True)
    assert rc == 0
    with pytest.raises(himg_amd.HimgError) as ei:
        eng.decode(want)
    assert ei.value.code == himg_amd.HIMG_ERR_FORMAT
    eng.set_option("fix_t2", 1)
    assert np.array_equal(eng.decode(want), px), (variant, w, "pixels")
    eng.set_option("fix_t2", 0)
    with pytest.raises(himg_amd.HimgError) as ei:
        eng.decode(want)
    assert ei.value.code == himg_amd.HIMG_ERR_FORMAT
    eng.close()


FRONT_SHAPES = [(512, 64), (1024, 72), (4096, 64), (1920, 136), (200, 72), (2048, 40), (8, 8), (64, 1024), (4096, 1032)]


@pytest.mark.parametrize("w,h", FRONT_SHAPES)
def test_front_kernel_matches_oracle(w, h):
    """k_front (box averages, low-res plane and pixel stage in one pass down the frame, what batches
    take) forced on single frames: every product it leaves -- averages, low-res plane, symbols --
    and the stream against the oracle; shapes with one row, one column of tiles, ragged last
    wavefronts, several chunks of block rows (rows >= 96)."""
    eng = himg_amd.Engine(0)
    eng.set_option("front", 1)
    imgs = [("randtile", himg_amd.synth("randtile", 2, w, h)), ("rand", himg_amd.synth("rand", 5, w, h)),
            ("gradn", himg_amd.synth("gradn", 1, w, h))]
    for name, img in imgs:
        for q, ycc in ((50, True), (90, False), (10, True)):
            want, tr = ol.oracle_encode(img, q, ycc, trace=True)
            got = eng.encode(img, q, ycc)
            n_plane = 4 * tr["rows"] * tr["cols"]
            assert np.array_equal(eng.debug_read("avg", 0, n_plane), tr["avg"]), (name, q, ycc, "box averages")
            assert np.array_equal(eng.debug_read("lowres", 0, n_plane), tr["lowres"]), (name, q, ycc, "low-res plane")
            assert np.array_equal(eng.debug_read("fres_sym", 0, tr["fres_sym"].size), tr["fres_sym"]), (name, q, ycc, "symbols")
            assert got.size == want.size and np.array_equal(got, want), (name, q, ycc)
    eng.close()
