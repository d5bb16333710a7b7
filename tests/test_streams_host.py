"""No GPU: the case table of the stream tests (tests/stream_cases.py) is what tests/test_gpu_streams.py takes
it for -- a decoy that a mis-ordered engine operation would turn into a DIFFERENT result, a damaged stream the
concealing decode really conceals, a prefix that really ends mid-stream, sequences whose calls differ in what
the pinned ring carries, origins inside their pictures -- and the gate helper imports without a GPU."""
import numpy as np
import pytest

import conceal_model as cm
import damage_model as dm
import oracle_lib as ol
import prefix_model as pm
import stream_cases as sc
import stream_gate as sg


@pytest.fixture(scope="module")
def cases():
    return sc.build()


def _streams(case, which):
    """The streams of a decode case's buffer: the real ones by their sizes, the decoys by their RIFF headers."""
    buf = case[which].reshape(-1, case["args"]["in_stride"])
    return [row[: 8 + int(row[4:8].view("<u4")[0])] for row in buf]


def test_every_form_and_shape_is_there(cases):
    ids = {c["id"] for c in cases}
    forms = {}
    for c in cases:
        forms.setdefault(c["shape"], set()).add(c["form"])
    for shape in sc.SHAPES:
        want = set(sc.DECODE_FORMS) if shape in sc.ALL_FORMS_SHAPES else {"decode"}
        if shape in sc.ENCODE_SHAPES:
            want |= set(sc.ENCODE_FORMS)
        assert forms[shape] == want, (shape, forms[shape] ^ want)
    for seq in list(sc.SEQUENCES.values()) + list(sc.TWO_CONTEXTS.values()) + [sc.MOVED]:
        assert set(seq) <= ids, set(seq) - ids
    assert "encode_forced@256x64x4" in ids
    assert all(c["form"] in sc.FORMS for c in cases)
    # 128 block rows: at least 16 x kWalkSegs (4), so that HIMG_WALK_SEGS=4 splits the frame into row ranges
    s = sc.SHAPES["256x1024x4"]
    assert s.B == 1 and (s.H + 7) // 8 >= 16 * 4


def test_real_and_decoy_share_the_geometry_and_differ_in_the_result(cases):
    for c in cases:
        assert c["real"].shape == c["decoy"].shape and c["real"].dtype == c["decoy"].dtype == np.uint8, c["id"]
        W, H, C, B = c["geom"]
        if c["form"] in sc.DECODE_FORMS:
            real, decoy = _streams(c, "real"), _streams(c, "decoy")
            assert len(real) == len(decoy) == B
            for f in range(B):
                assert len(real[f]) == int(c["args"]["sizes"][f]) or c["form"] == "prefix", (c["id"], f)
                rc, pix = ol.oracle_decode(decoy[f], fix_t2=c["fix"])
                if c["id"].startswith("decode_after_conceal"):
                    assert (rc != 0) == (f == 1)    # its decoy is the damaged batch: only that frame differs
                    continue
                assert rc == 0 and pix.shape == (H, W, C), (c["id"], f, rc)
                if c["form"] == "conceal" and f == c["args"]["damaged"]:
                    continue
                rc, mine = ol.oracle_decode(real[f], fix_t2=c["fix"])
                assert rc == 0 and mine.shape == pix.shape and not np.array_equal(mine, pix), (c["id"], f)
        elif c["form"] == "windows":
            assert not np.array_equal(c["real"], c["decoy"]), c["id"]
        else:
            real, decoy = c["real"].reshape(B, H, W, C), c["decoy"].reshape(B, H, W, C)
            q = c["args"].get("quality", 50)
            for f in range(B):
                a, b = ol.oracle_encode(real[f], q, True), ol.oracle_encode(decoy[f], q, True)
                assert not np.array_equal(a, b), (c["id"], f)


def test_the_decoy_changes_every_output(cases):
    """An output that the decoy's picture would fill with the same bytes could not show a read of the decoy:
    the pictures, crops and previews of the decoy differ from the real ones frame by frame."""
    for c in cases:
        if c["form"] in ("decode", "regions", "preview") and not c["id"].startswith("decode_after_conceal"):
            W, H, C, B = c["geom"]
            want = c["outs"]["pix"]["want"]
            for f, s in enumerate(_streams(c, "decoy")):
                if c["form"] == "preview":
                    other = sc.preview_of(s, c["fix"])
                else:
                    other = sc.full_of(s, c["fix"])
                    if c["form"] == "regions":
                        x, y = c["args"]["origins"][f]
                        other = other[y:y + c["args"]["h"], x:x + c["args"]["w"]]
                assert other.shape == want[f].shape and not np.array_equal(other, want[f]), (c["id"], f)


def test_sentinels_differ_from_the_results(cases):
    for c in cases:
        for name, o in c["outs"].items():
            want = o["want"].reshape(-1).view(np.uint8)
            init = o["init"]
            base = np.full(want.size, init, np.uint8) if isinstance(init, int) else np.asarray(init).reshape(-1)
            assert base.size == want.size and not np.array_equal(base, want), (c["id"], name)
            if o["mask"] is not None:
                assert o["mask"].size == want.size and o["mask"].any()


def test_conceal_case_has_a_sound_head_and_a_rejected_row(cases):
    n = 0
    for c in cases:
        if c["form"] != "conceal":
            continue
        n += 1
        f = c["args"]["damaged"]
        bad = _streams(c, "real")[f]
        good = sc.streams(c["shape"], sc.REAL_SEED)[f]
        assert len(bad) == len(good) and 0 < int((bad != good).sum()) <= 1
        _, layout = dm.rows_of(good, c["fix"])
        at = int(np.flatnonzero(bad != good)[0])
        assert any(o - 4 <= at < o for o, _ in layout), "the damage lies in a row's size header"
        assert ol.oracle_decode(bad, fix_t2=c["fix"])[0] != 0            # the full decode rejects the picture ...
        code, _, plan = dm.walk_rows(bad, None, None, c["fix"])
        assert plan["head_bytes"] != 0                                   # ... behind a sound head
        pic, rowmap = cm.expect(pm.Model(good, c["fix"]), bad, c["fix"])
        assert 0 < int(rowmap.sum()) < rowmap.size
        assert np.array_equal(c["outs"]["rowmap"]["want"][f], rowmap)
        assert int(c["outs"]["concealed"]["want"][f]) == int(rowmap.sum())
        assert np.array_equal(c["outs"]["pix"]["want"][f], pic.reshape(c["outs"]["pix"]["want"][f].shape))
        others = [g for g in range(c["geom"][3]) if g != f]
        assert not c["outs"]["rowmap"]["want"][others].any()
    assert n == len(sc.ALL_FORMS_SHAPES)


def test_prefix_case_ends_mid_stream(cases):
    n = 0
    for c in cases:
        if c["form"] != "prefix":
            continue
        n += 1
        rows = (c["geom"][1] + 7) // 8
        for f, s in enumerate(sc.streams(c["shape"], sc.REAL_SEED)):
            avail = int(c["args"]["sizes"][f])
            code, k, pic = pm.Model(s, c["fix"]).expect(avail)
            assert code == pm.OK and 1 <= k <= rows - 1 and avail < len(s), (c["id"], f, code, k)
            assert int(c["outs"]["rows"]["want"][f]) == k
            assert np.array_equal(c["outs"]["pix"]["want"][f], pic)
            full = sc.full_of(s, c["fix"])
            assert np.array_equal(pic[:8 * k], full[:8 * k]) and not np.array_equal(pic[8 * k:], full[8 * k:])
    assert n == len(sc.ALL_FORMS_SHAPES)


def test_six_call_sequence_differs_in_every_size_and_origin(cases):
    by_id = {c["id"]: c for c in cases}
    seq = [by_id[i] for i in sc.SEQUENCES["six_decodes"]]
    assert len(seq) == 6 > 4      # more calls than the pinned ring has slots: the fifth takes slot 0 again
    for a in range(6):
        for b in range(a + 1, 6):
            sa, sb = seq[a]["args"]["sizes"], seq[b]["args"]["sizes"]
            assert (sa != sb).all(), (a, b, sa, sb)
            assert (seq[a]["args"]["origins"] != seq[b]["args"]["origins"]).any(1).all(), (a, b)
            assert not np.array_equal(seq[a]["outs"]["pix"]["want"], seq[b]["outs"]["pix"]["want"])


def test_sequences_alternate_geometries_and_workspace_kinds(cases):
    by_id = {c["id"]: c for c in cases}
    four = [by_id[i] for i in sc.SEQUENCES["four_decodes"]]
    assert [c["form"] for c in four] == ["decode", "preview", "regions", "decode"]
    assert four[0]["geom"] != four[1]["geom"] and four[2]["geom"] != four[3]["geom"]
    assert sc.SEQUENCES["four_decodes_reversed"] == sc.SEQUENCES["four_decodes"][::-1]
    enc = [by_id[i] for i in sc.SEQUENCES["four_encodes"]]
    assert [c["form"] for c in enc] == ["encode", "sizes", "budget", "windows"]
    assert all(enc[k]["geom"] != enc[k + 1]["geom"] for k in range(3))
    con, dec = (by_id[i] for i in sc.SEQUENCES["conceal_then_decode"])
    assert con["geom"] == dec["geom"] and np.array_equal(dec["decoy"], con["real"])
    assert len(sc.SEQUENCES["four_decodes"]) == len(sc.SEQUENCES["four_encodes"]) == 4


def test_origins_lie_inside_their_pictures(cases):
    seen = 0
    for c in cases:
        a = c["args"]
        W, H, C, B = c["geom"]
        if c["form"] in ("scaled_regions",):
            W, H = (W + 1) // 2, (H + 1) // 2
        for key, (pw, ph) in (("origins", (W, H)), ("src_origins", (W, H))):
            if key in a and c["form"] not in ("into", "windows"):
                for x, y in a[key]:
                    assert 0 <= x and 0 <= y and x + a["w"] <= pw and y + a["h"] <= ph, (c["id"], key)
                    seen += 1
        if c["form"] == "region":
            assert 0 <= a["x"] and 0 <= a["y"] and a["x"] + a["w"] <= W and a["y"] + a["h"] <= H
            seen += 1
        for key, desc, (w, h) in (("origins", a.get("dst") if c["form"] == "into" else a.get("src"), (a.get("w", W), a.get("h", H))),
                                  ("dst_origins", a.get("dst"), (a.get("w"), a.get("h")))):
            if desc is not None and key in a and c["form"] in ("into", "regions_into", "windows"):
                for x, y in a[key]:
                    assert 0 <= x and 0 <= y and x + w <= desc["width"] and y + h <= desc["height"], (c["id"], key)
                    seen += 1
                assert c["real"].size >= 0 and desc["row_pitch"] > desc["width"] * desc["pixel_stride"]   # pitched
        if c["form"] == "windows":
            assert any(int(x) & 1 for x, _ in a["origins"]), "an odd origin in a pitched source"
    assert seen >= 60


def test_gate_helper_without_a_gpu():
    assert sg.gate_ms(0.0) == 30.0 and sg.gate_ms(0.001) == 30.0 and sg.gate_ms(0.004) == 80.0
    assert sg.timed_call(lambda: None) >= 0.0
