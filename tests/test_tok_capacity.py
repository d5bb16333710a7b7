"""CPU: the capacity of a token segment and of k_tok's stage (himg_dev.h tok_seg_pad /
tok_stage_need, read through himg_hip_tok_layout) against the slot model of tests/tok_model.py,
on the crafted pictures that push a segment to its edge and on seeded symbol rows of every
density.  The bound is proven in himg_dev.h; here it is held against what k_tok's rules
count, and the pictures that outgrew the former fixed pad of 64 slots are shown to do so."""
import numpy as np
import pytest

import himg_amd
import oracle_lib as ol
import tok_model as tm

WIDTHS = [2048, 4096, 12288, 16384, 20480, 24576, 32768]
OLD_PAD = 64   # tok_cap was tok_seg + 64 whatever the width


def _layout(w, h=24):
    return himg_amd.tok_layout(w, h, 4, row_tokens=1)


def _crafted_demand(variant, w, q=100):
    h = tm.crafted_height(w)
    img = tm.crafted(variant, w, h)
    _, tr = ol.oracle_encode(img, q, False, trace=True)
    lay = _layout(w, h)
    assert lay["nseg"] == (w // 8 * 256 + lay["seg"] - 1) // lay["seg"]
    counts, worst = tm.frame_demand(tr["fres_sym"], tr["rows"], lay["seg"], lay["nseg"], lay["stage"])
    assert (counts == counts[0]).all(), "every block row of a crafted picture is the same"
    return lay, counts, worst


def _check(lay, counts, worst, what):
    print(what, "seg", lay["seg"], "cap", lay["cap"], "max slots", int(counts.max()), "padded", int(tm.padded(counts).max()),
          "staged", worst, "stage bound", lay["stage_need"], "tokens", lay["tokens"])
    assert tm.padded(counts).max() <= lay["cap"], (what, "a segment outgrows its slots")
    assert worst <= max(lay["stage_need"], lay["stage"]), (what, "a flush outgrows the bound on the stage")
    if lay["tokens"]:
        assert worst <= lay["stage"], (what, "a flush outgrows the stage of a geometry the token path takes")


def test_layout_invariants():
    for w in WIDTHS + [8, 200, 1000, 1920, 8192]:
        lay = _layout(w)
        assert lay["seg"] % tm.ITER == 0 and lay["cap"] % 8 == 0 and lay["cap"] >= lay["seg"] + OLD_PAD
        assert lay["stage"] == tm.STAGE
        assert lay["tokens"] == (lay["stage_need"] <= lay["stage"])
    # the workspace layout of the widths measured so far is what it was
    for w in (512, 1024, 1920, 2048, 4096, 8192):
        assert _layout(w)["cap"] == _layout(w)["seg"] + OLD_PAD


def test_stage_rule_chooses_the_path():
    """Rows whose half-iteration could outgrow the stage keep the dense kernels, forced or not."""
    for rt in (1, 2):
        assert himg_amd.tok_layout(16384, 24, 4, row_tokens=rt)["tokens"]
        assert himg_amd.tok_layout(12288, 24, 4, row_tokens=rt)["tokens"]
        assert himg_amd.tok_layout(20480, 24, 4, row_tokens=rt)["tokens"]      # 1024 + 5 + 117 slots at most
        assert not himg_amd.tok_layout(24576, 24, 4, row_tokens=rt)["tokens"]  # 1024 + 5 + 141
        assert not himg_amd.tok_layout(32768, 16, 4, row_tokens=rt)["tokens"]
    assert himg_amd.tok_layout(16384, 4096, 4, row_tokens=-1, batch=16)["tokens"]     # 8192 block rows
    assert not himg_amd.tok_layout(32768, 4096, 4, row_tokens=-1, batch=16)["tokens"]
    assert not himg_amd.tok_layout(16384, 24, 4, row_tokens=0)["tokens"]


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("variant", tm.VARIANTS)
def test_crafted_pictures_fit_the_bound(variant, w):
    lay, counts, worst = _crafted_demand(variant, w)
    _check(lay, counts, worst, (variant, w))


def test_crafted_pictures_outgrow_the_old_capacity():
    """The recorded demand of the pictures (q100, no colour transform): 12288 pixels need exactly the
    former capacity, 16384 and 32768 pixels more -- the inputs that used to overflow fit now."""
    lay, counts, _ = _crafted_demand("alpha", 12288)
    assert lay["seg"] == 49152 and counts[0, -1] == 49215 and tm.padded(counts).max() == lay["seg"] + OLD_PAD
    lay50, counts50, _ = _crafted_demand("alpha", 12288, q=50)
    assert np.array_equal(counts50, counts)
    lay, counts, worst = _crafted_demand("alpha", 16384)
    assert lay["seg"] == 65536 and counts[0, -1] == 65620
    assert tm.padded(counts).max() == lay["seg"] + OLD_PAD + 24 <= lay["cap"]
    assert worst <= tm.STAGE
    lay, counts, worst = _crafted_demand("alpha", 32768)
    assert lay["seg"] == 131072 and counts[0, -1] == 131240 > lay["seg"] + OLD_PAD
    assert tm.padded(counts).max() <= lay["cap"]
    assert worst == 1024 + 168 > tm.STAGE and not lay["tokens"]   # a dense half behind 7/8 of the row
    # the other pictures at 16384 pixels, all below the former capacity of 65 600
    lay, counts, _ = _crafted_demand("chan2", 16384)
    assert counts[0, 5] == 65596 and counts[0, 7] == 24 and counts[0, 6] == 0
    lay, counts, _ = _crafted_demand("chan0", 16384)
    assert counts[0, 1] == 65548 and counts[0, 7] == 72
    lay, counts, _ = _crafted_demand("fifth", 16384)
    assert counts[0, 7] == 65210
    lay, counts, _ = _crafted_demand("lastcol", 16384)
    assert counts[0, 7] == 209 and not counts[0, :7].any()


def _rows(rb, seg, rng):
    """Seeded symbol rows: every density, and the shapes the proof's worst cases have."""
    for d in list(np.linspace(0.0, 1.0, 21)) + [1e-5, 1e-4, 1e-3, 0.003, 0.56, 0.99, 0.999]:
        yield "density %.5f" % d, np.where(rng.random_sample(rb) < d, rng.randint(1, 256, rb), 0).astype(np.uint8)
    z = np.zeros(rb, np.uint8)
    yield "zero", z
    r = z.copy(); r[-1] = 1
    yield "last symbol", r
    r = z.copy(); r[0] = 1
    yield "first symbol", r
    r = z.copy(); r[rb - 1024:rb - 1] = 7                      # the longest lead, a dense half, one trailing zero
    yield "lead, dense half, trail 1", r
    r = z.copy(); r[rb - 1024 + 1:rb - 1] = 7
    yield "lead + 1, dense half, trail 1", r
    r = z.copy(); r[(rb - 1) // seg * seg:] = 9                # zeros, then a dense last segment
    yield "dense last segment", r
    r[-1] = 0
    yield "dense last segment, trail 1", r
    r = np.full(rb, 3, np.uint8); r[seg - 300:seg] = 0         # a run of more than 255 zeros that ends a segment
    yield "run to the segment's end", r
    r = np.full(rb, 3, np.uint8); r[0:seg - 2048 + 3] = 0; r[5] = 1   # a slot carried into a long lead inside the segment
    yield "carried slot, lead in the segment", r
    for k in (16662, 16663, 2 * 16662, 255, 256, 257):
        r = np.full(rb, 5, np.uint8); r[1:1 + k] = 0
        yield "run of %d" % k, r
        r = z.copy(); r[:rb - k] = 5
        yield "trail of %d" % k, r
    # literals 257 symbols apart: every one behind a run on its own
    r = z.copy(); r[256::257] = 1
    yield "a run on its own in front of every literal", r


@pytest.mark.parametrize("w", WIDTHS)
def test_seeded_rows_fit_the_bound(w):
    lay = _layout(w)
    rb = w // 8 * 256
    rng = np.random.RandomState(w)
    for name, row in _rows(rb, lay["seg"], rng):
        counts, st = tm.row_demand(row, lay["seg"], lay["nseg"], lay["stage"])
        halves = [x for _, x, half in st if half]
        assert not halves or max(halves) <= lay["stage_need"], (w, name, "half an iteration outgrows the bound")
        assert all(x <= lay["stage"] for _, x, half in st if not half), (w, name)
        _check(lay, counts[None, :], max(x for _, x, _ in st), (w, name))


def test_model_counts_a_small_row_by_hand():
    """The model itself on a row small enough to count by hand."""
    row = np.zeros(4096, np.uint8)
    row[10] = 1            # 10 zeros in front: one slot
    row[300] = 2           # 289 zeros: a run on its own (3) + the literal
    row[301] = 3           # one slot
    row[2047] = 4          # 1745 zeros: 3 + 1; the 2048 trailing zeros follow in the second segment: 3
    counts, st = tm.row_demand(row, 2048, 2)
    assert list(counts) == [1 + 4 + 1 + 4, 3]
    assert st == [(0, 10, False), (1, 3, False)]
    assert list(tm.padded(counts)) == [16, 8]
