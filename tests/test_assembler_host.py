"""CPU: the stream assembler (tests/stream_assembler.py) and the assembled streams (tests/assembled_cases.py).

1. The assembler is pinned: the oracle's trace of four pictures, put together again, is the oracle's
   stream byte for byte -- tree order, LSB-first packing, the stale pad bits of the rows' last bytes.
2. The oracle is pinned on every assembled stream: its verdict and pixels are the REAL reference's,
   live when oracle/_ref is built and always through tests/golden/assembled_streams.json (recorded from
   the real reference; `python tests/golden/make_golden_assembled.py` rewrites it).  Ragged shapes and
   the tree of 262 leaves are outside what the reference defines: the oracle judges them alone.  The
   oracle's decode trace returns exactly the symbols that went in.
3. The streams reach what they are for: conditions restated in numpy from the inputs (never measured
   on the engine), so that a later edit of the generators cannot turn them back into easy streams."""
import hashlib
import json
import os

import numpy as np
import pytest

import assembled_cases as ac
import himg_amd
import oracle_lib as ol
import stream_assembler as sa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembled_streams.json")
IDS = [ac.case_id(k) for k in ac.CASES]


_REACH = {}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("w,h,c,q,ycc", [(64, 64, 4, 50, True), (200, 72, 3, 90, True), (136, 40, 1, 30, False),
                                        (512, 64, 4, 100, False)])
def test_assembler_reproduces_the_encoder(w, h, c, q, ycc):
    for kind in ("randtile", "grad"):
        img = himg_amd.synth(kind, 3, w, h)
        img = np.ascontiguousarray(img[:, :, :c] if c > 1 else img[:, :, 0])
        packed, tr = ol.oracle_encode(img, q, ycc, trace=True)
        got = sa.from_trace(w, h, c, ycc and c >= 3, tr)
        assert got.size == packed.size and np.array_equal(got, packed), (kind, got.size, packed.size)


def test_tree_helpers():
    t = sa.balanced(range(261))
    assert sa.tree_bytes(t).size == 359 and len(sa.leaves(t)) == 261 and sa.depth(t) == 9
    assert sa.depth(ac.tree_comb()) == 32 and sa.depth(ac.tree_comb(34)) == 33
    lv = sa.leaves(sa.fixed_length(range(20), 5))
    assert len(lv) == 32 and {n for _, n, _ in lv} == {5}
    # codes are prefix-free and complete: Kraft's sum is one
    for tree in (t, ac.tree_comb(), ac.tree_sub_overflow(), ac.tree_deeper_17(), ac.tree_dup()):
        lv = sa.leaves(tree)
        assert sum(2 ** (40 - n) for _, n, _ in lv) == 2 ** 40
        if len({s for s, _, _ in lv}) == len(lv):
            assert sa.leaves(sa.tree_from_codes(*_table(lv))) == lv


def _table(lv):
    length, code = [0] * 512, [0] * 512
    for s, n, c in lv:
        length[s], code[s] = n, c
    return length, code


def test_token_helpers():
    rng = np.random.default_rng(5)
    row = np.zeros(40000, np.uint8)
    row[[0, 5, 6, 9, 17, 18, 300, 20000]] = (1, 2, 3, 4, 5, 6, 7, 8)
    enc = sa.encoder_tokens(row)
    assert np.array_equal(sa.expand_tokens(enc), row)
    # the greedy rule never puts two run tokens in a row but at a 16 662-zero split
    assert enc[:, 0].tolist() == [1, 257, 2, 3, 256, 4, 258, 5, 6, 260, 7, 260, 260, 8, 260, 260]
    for mode in ("literal", "random", "base"):
        t = sa.split_tokens(row, rng, mode)
        assert np.array_equal(sa.expand_tokens(t), row), mode
    assert (sa.split_tokens(row, rng, "literal")[:, 0] <= 255).all()
    assert (sa.split_tokens(row, rng, "base")[:, 1] == 0).all()


@pytest.mark.parametrize("key", ac.CASES, ids=IDS)
def test_oracle_is_the_reference(golden, key):
    c = ac.case(*key)
    g = golden[c.id]
    assert c.sha() == g["sha256"], "the generator no longer makes the stream that the golden file judged"
    assert g["judge"] == ("reference" if ac.reference_judges(key) else "oracle")
    rc, pix = ol.oracle_decode(c.stream)
    assert (rc == 0) == g["accepted"], (c.id, rc)
    if rc == 0:
        assert hashlib.sha256(pix.tobytes()).hexdigest() == g["pixels_sha256"], c.id
    if ol.have_ref() and ac.reference_judges(key):
        rrc, rpix = ol.ref_decode(c.stream)
        assert (rrc == 0) == (rc == 0), (c.id, rc, rrc)
        if rc == 0:
            assert np.array_equal(pix, rpix), c.id
    rc_fix, pix_fix = ol.oracle_decode(c.stream, fix_t2=True)
    if c.expect == "accept":
        assert rc == 0, (c.id, rc)
    if c.expect == "reject":
        assert rc != 0 and rc_fix != 0, (c.id, rc, rc_fix)
    else:
        assert rc_fix == 0, (c.id, rc_fix)
    if c.expect == "unsupported":
        assert rc == 0, "the reference decodes a tree 33 deep"
    if rc == 0:
        assert np.array_equal(pix, pix_fix), c.id
    # the symbols that went in come back
    if rc_fix == 0:
        ol.oracle().himg_oracle_set_compat_fix(int(rc != 0))
        try:
            trc, dt = ol.oracle_decode_trace(c.stream)
        finally:
            ol.oracle().himg_oracle_set_compat_fix(0)
        assert trc == 0
        assert np.array_equal(dt["lres_sym"], c.lres_sym()), c.id
        assert np.array_equal(dt["fres_sym"], c.fres_sym()), c.id
    r = c.reach()        # while the case is there: building it is the expensive part
    if "lowres_sha256" in r:      # the numpy model of the low-res prediction is the oracle's
        assert rc_fix == 0 and hashlib.sha256(dt["lowres"].tobytes()).hexdigest() == r["lowres_sha256"], c.id
    # trap T2, from the sizes alone
    if c.expect in ("accept", "t2", "unsupported"):
        assert (rc == 0) == c.t2_accepts(), (c.id, rc, c.fres_chunk_size())
    _REACH[c.id] = r
    ac.case.cache_clear()


# ---- reach ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reach():
    for key in ac.CASES:
        if ac.case_id(key) not in _REACH:
            _REACH[ac.case_id(key)] = ac.case(*key).reach()
            ac.case.cache_clear()
    return _REACH


def _of(reach, prefix):
    r = [v for k, v in reach.items() if k.startswith(prefix) and v["expect"] != "reject"]
    assert r, prefix
    return r


def test_reach_transform(reach):
    c = _of(reach, "C-")
    assert sum(r["planes_neither"] for r in c) and sum(r["planes_A_only"] for r in c) and sum(r["planes_B_only"] for r in c)
    assert sum(r["groups32_mixed"] for r in c), "no group of 32 tiles mixes a failing plane with passing ones"
    assert sum(r["wraps_int16"] for r in c), "no dequantised coefficient wraps int16"
    assert any(r["extreme_codes_every_position"] for r in c), "127, -127 and -128 at every scan position"
    for r in c:                      # every table set by itself sends planes down the scalar path
        if "nibbles-0" not in r["id"] and "fmap-identity" not in r["id"] and "shift-11" not in r["id"]:
            assert r["planes_neither"], r["id"]


def test_reach_identity(reach):
    total = {}
    for r in _of(reach, "C-"):
        for k, e in r["identity"].items():
            t = total.setdefault(k, dict.fromkeys(e, 0))
            for f in e:
                t[f] += e[f]
    assert {"B=0 fmap[1] != 1", "B=0 a shift lowered it", "B=1", "B=32", "B=64"} <= set(total), sorted(total)
    for k in ("B=1", "B=32", "B=64"):      # (the codes -B and B - 1 are counted inside wavefronts that pass)
        assert all(total[k].values()), (k, total[k])
    # The lowering of B by the largest shift decides something: on every shape whose kernel form has the
    # identity test there are wavefronts that pass only the UNLOWERED range, hold a plane outside both
    # range conditions and overflow int16 in a row sum -- the packed transform would be wrong for them.
    for shape in ((4096, 16, 4), (2048, 16, 4), (1920, 16, 4), (64, 24, 4), (4352, 16, 4)):
        for kind in ("C-shift-11", "C-nibbles-random"):
            r = reach[ac.case_id((kind,) + shape)]
            assert r["lowering_gap_overflowing"] > 0, (r["id"], r["lowering_gap_wavefronts"])
        assert reach[ac.case_id(("C-nibbles-15",) + shape)]["lowering_gap_wavefronts"] > 0


def test_reach_trees(reach):
    a = {r["id"].split("@")[0]: r for r in _of(reach, "A-") if "@64x24x4" in r["id"]}
    assert a["A-comb32"]["fres"]["depth"] == 32 and a["A-comb32"]["lres"]["depth"] == 32
    assert a["A-balanced261"]["fres"]["leaves"] == 261 and a["A-balanced261"]["fres"]["tree_bytes"] == 359
    so = a["A-sub-overflow"]["fres"]
    assert so["sub_entries_wanted"] > ac.SUB_ENTRIES and so["prefixes_with_subtree"] <= ac.MAX_SLOW
    assert a["A-deeper-17"]["fres"]["depth"] > ac.LUT_BITS + ac.SUB_MAX_BITS
    assert a["A-deeper-17"]["lres"]["depth"] > ac.LUT_BITS + ac.SUB_MAX_BITS
    assert a["A-duplicates"]["fres"]["duplicate_symbols"] == 128
    assert a["A-unused-300"]["fres"]["leaf_above_260"]
    assert a["A-one-leaf"]["fres"]["leaves"] == 1 and a["A-one-leaf-lres"]["lres"]["leaves"] == 1
    for r in _of(reach, "A-"):
        if r["id"].split("@")[0][2:] in ac.TREES_A and r["fres"]["deep_leaves"]:
            assert r["fres"]["deep_leaves_used_in_every_payload"], r["id"]
    assert sum(r["fres"]["deep_leaves"] > 0 for r in _of(reach, "A-")) >= 4 * len(ac.SHAPES)
    # the LRES side of the two trees that are also LRES trees: every deep leaf where the plane has room for all
    # leaves (a plane of 64x24 has 100 symbols), and never fewer than the plane can hold
    for r in _of(reach, "A-"):
        kind, shape = r["id"].split("@")
        if kind in ("A-comb32", "A-deeper-17"):
            lr = r["lres"]
            if shape in ("4096x16x4", "2048x16x4", "1920x16x4", "4352x16x4"):
                assert lr["deep_leaves_used_in_every_payload"], r["id"]
            assert lr["deep_leaves_used_at_least"] >= min(lr["deep_leaves"], 15), (r["id"], lr["deep_leaves_used_at_least"])
    # rows above 32 767 bytes take the four-byte size
    assert any(max(r["fres"]["payload_bits"]) > 8 * 0x7fff for r in _of(reach, "A-comb32"))


def test_reach_tokens(reach):
    for shape in ("@64x24x4", "@4096x16x4"):
        e = [r for r in _of(reach, "B-") if "edges" in r["id"] and shape in r["id"]]
        assert len(e) == 2
        for r in e:
            assert r["run_tokens_in_a_row"] >= 3 and r["rows_ending_in_a_run"] and r["rows_of_literal_zeros"], r["id"]
    for r in (r for r in _of(reach, "B-") if "edges@4096" in r["id"] or "edges@2048" in r["id"]):
        assert all(lo and hi for lo, hi in r["run_extra_min_max"].values()), (r["id"], r["run_extra_min_max"])
    for r in (r for r in _of(reach, "B-") if "edges@64x24" in r["id"]):      # 16 662 zeros do not fit a row of 2048
        assert all(lo for lo, _ in r["run_extra_min_max"].values()), r["id"]
    for r in (r for r in _of(reach, "B-") if "all-runs" in r["id"]):
        assert r["rows_of_long_runs_only"] and not r["t2_accepts"], r["id"]


def test_reach_fixed_length(reach):
    for r in _of(reach, "E-"):
        bits = int(r["id"][2])
        side = "lres" if "lres" in r["id"] else "fres"
        assert r[side]["token_bits"] == [bits], (r["id"], r[side]["token_bits"])
    big = reach[ac.case_id(ac.FIXED_MULTI_CHUNK)]
    assert big["lres"]["payload_bits"][0] > 3 * ac.LRES_CHUNK_BITS and big["lres_chunks"] >= 3


def test_reach_lres(reach):
    d = _of(reach, "D-")
    assert set().union(*(r["predictor_bytes"] for r in d)) == set(range(256))
    for k in ("-128", "-127", "127"):
        assert all(r["lres_deltas"][k] for r in d if "multi-chunk" not in r["id"]), k
    ext = [r for r in d if "lmap-extreme" in r["id"]]
    assert len(ext) == 3 and all(r["lmap_32767_meets_predicted_ge_1"] > 0 for r in ext), "predicted + unmap never leaves int16"
    big = reach[ac.case_id(ac.MULTI_CHUNK)]
    assert big["lres"]["payload_bits"][0] > 3 * ac.LRES_CHUNK_BITS and big["lres_chunks"] >= 3, big["lres"]["payload_bits"]


def test_reach_trap_t2(reach):
    for r in reach.values():
        if r["expect"] == "accept":
            assert r["t2_accepts"] and r["fres_chunk"] > r["row_symbols"], r["id"]


# ---- the container family through the host peeks (no GPU) --------------------------------------------

@pytest.mark.parametrize("kind", ac.KINDS_F)
def test_container_host_peeks(kind):
    """peek, preview_peek, index_host, region_peek and scaled_region_peek walk the chunks on the host:
    with extra chunks, decoys and a long FRMT they find what the decoder's forward search finds."""
    import scaled_model as sm
    c = ac.case("F-" + kind, 64, 24, 4)
    W, H, C = c.W, c.H, c.C
    s = c.stream
    ch = sm.find_chunks(s)
    tree, rows = c.parts["fres_tree"], c.parts["fres_row_tokens"]
    first = ch["FRES"][0] + sa.tree_bytes(tree).size
    lengths = [(int(sa.token_code_lengths(tree, t).sum()) + 7) // 8 for t in rows]
    offsets, at = [], first
    for n in lengths:
        offsets.append(at + 2)
        at += 2 + n
    assert at == ch["FRES"][0] + ch["FRES"][1]
    assert himg_amd._peek(np.ascontiguousarray(s)) == (W, H, C)
    assert himg_amd.preview_peek(s) == (c.cols, c.rows, C, ch["LRES"][0] + ch["LRES"][1])
    for fix in (False, True):
        w, h, cn, off, ln, rows_first = himg_amd.index_host(s, fix)
        assert (w, h, cn, off.tolist(), ln.tolist(), rows_first) == (W, H, C, offsets, lengths, first)
        for rect, (r0, r1) in (((3, 9, 20, 10), (1, 3)), ((0, 0, 64, 24), (0, 3)), ((60, 0, 4, 8), (0, 1))):
            want = {"width": W, "height": H, "num_channels": C, "row0": r0, "row1": r1, "head_bytes": first,
                    "rows_begin": offsets[r0] - 2, "rows_end": offsets[r1 - 1] + lengths[r1 - 1]}
            assert himg_amd.region_peek(s, *rect, fix_t2=fix) == want, rect
            x, y, rw, rh = rect
            for sl in (1, 2):
                f = 1 << sl
                srect = (x // f, y // f, max(1, rw // f), max(1, rh // f))
                full = (f * srect[0], f * srect[1], min(f * srect[2], W - f * srect[0]), min(f * srect[3], H - f * srect[1]))
                assert himg_amd.scaled_region_peek(s, sl, *srect, fix_t2=fix) == himg_amd.region_peek(s, *full, fix_t2=fix)
    for sl in (1, 2):
        assert himg_amd.scaled_size(W, H, sl) == (-(-W >> sl), -(-H >> sl))
    for dtype, size in ((himg_amd.HIMG_DT_F32, 4), (himg_amd.HIMG_DT_F16, 2), (himg_amd.HIMG_DT_BF16, 2)):
        assert himg_amd.tensor_bytes(himg_amd.tensor_desc(dtype, 3), C, W, H) == 3 * W * H * size
