"""The plain tree model (tests/tree_model.py) against the oracle's own tree builder on the histogram
corpus (tests/tree_cases.py), and proof that the corpus reaches the parts of k_tree it is meant for.

The oracle's make_tree is the judge: it is the code the goldens tie to the real reference.  The model is
what tests/test_gpu_trees.py holds the kernel against.  HIMG_WRITE_GOLDEN=1 rewrites the recorded files
(tests/golden/tree_picture_hists.json, tests/golden/tree_reach.json) instead of comparing with them."""
import collections
import json
import os

import numpy as np

import himg_amd
import oracle_lib as ol
import deep_pictures as dp
import tree_cases as tc
from tree_model import batch_profile, tree_model

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REACH = os.path.join(GOLDEN_DIR, "tree_reach.json")
WRITE = os.environ.get("HIMG_WRITE_GOLDEN", "") == "1"

# name -> (picture, quality, colour lift): what the picture histograms of the corpus are traced from
PICTURES = {
    "randtile_s1_256x128_q50": (lambda: himg_amd.synth("randtile", 1, 256, 128), 50, True),
    "gradn_s4_512x512_q50": (lambda: himg_amd.synth("gradn", 4, 512, 512), 50, True),
    "rand_s7_136x72_q100": (lambda: himg_amd.synth("rand", 7, 136, 72), 100, True),
    "randtile_s6_256x512_q10": (lambda: himg_amd.synth("randtile", 6, 256, 512), 10, True),
    "grad_s0_256x256_q0": (lambda: himg_amd.synth("grad", 0, 256, 256), 0, True),
    "deep_fres_wide": (lambda: dp.picture("fres_wide")[0], dp.QUALITY, dp.USE_YCBCR),
    "deep_fres_narrow": (lambda: dp.picture("fres_narrow")[0], dp.QUALITY, dp.USE_YCBCR),
    "deep_lres": (lambda: dp.picture("lres")[0], dp.QUALITY, dp.USE_YCBCR),
}


def test_model_is_the_oracles_tree_on_the_whole_corpus():
    cases, want = tc.cases(), tc.expected()
    assert len(cases) > 5000
    for (family, sub, hist), (lens, codes, tree, nbytes) in zip(cases, want):
        o_bits, o_code, o_tree, o_n = ol.oracle_tree(hist)
        what = "%s / %s" % (family, sub)
        assert lens == o_bits.tolist(), what
        assert codes == [int(x) for x in o_code], what        # (the corpus stays below 64 bits: the oracle's code words)
        assert nbytes == o_n and tree == o_tree, what
        assert all((l > 0) == (c > 0) for l, c in zip(lens, hist.tolist())), what


def test_picture_histograms_are_the_oracles_and_their_trees_the_streams():
    """The recorded picture histograms are what the oracle traces today; for them the model also equals the
    trace's code table and the tree bytes inside the oracle's stream."""
    rec = {}
    for name, (make, q, ycc) in PICTURES.items():
        packed, tr = ol.oracle_encode(make(), q, ycc, trace=True)
        rec[name] = {"lres_hist": [int(x) for x in tr["lres_hist"]], "fres_hist": [int(x) for x in tr["fres_hist"]]}
        chunks = ol.chunk_payloads(packed)
        for strm, at in (("lres", chunks["LRES"][0]), ("fres", chunks["FRES"][0])):
            lens, codes, tree, nbytes = tree_model(rec[name][strm + "_hist"])
            assert lens == tr[strm + "_len"].tolist(), (name, strm)
            assert codes == [int(x) for x in tr[strm + "_code"]], (name, strm)
            assert nbytes == tr[strm + "_tree_bytes"], (name, strm)
            assert packed[at:at + nbytes].tobytes() == tree, (name, strm)
    if WRITE:
        with open(tc.PICTURE_HISTS, "w") as f:
            json.dump(rec, f, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    with open(tc.PICTURE_HISTS) as f:
        assert json.load(f) == rec
    assert len(tc.picture_cases()) == 2 * len(PICTURES)


def test_corpus_reaches_what_it_is_for():
    """Conditions on the INPUTS, counted with the batched form of the merge (same thresholds and caps as
    the kernel): enough histograms for every way through k_tree's merge, and depths at and beyond the limit."""
    cases, want = tc.cases(), tc.expected()
    n = collections.Counter()
    for (family, sub, hist), (lens, _, _, _) in zip(cases, want):
        p = batch_profile(hist.tolist())
        n["histograms"] += 1
        if p["n"] == 1:
            n["one_symbol"] += 1
        elif p["serial"] == 0:
            n["batches_alone"] += 1
        elif p["rounds"] == 0:
            n["serial_alone"] += 1
        else:
            n["hand_over"] += 1
            n["hand_over_with_leftover"] += int(p["leftover"])
        n["run_grows_in_serial_loop"] += int(p["grew"] > 0)
        n["more_than_64_symbols"] += int(p["n"] > 64)
        n["total_at_int_limit"] += int(int(hist.sum()) == tc.INT_MAX)
        d = max(lens)
        n["depth_32"] += int(d == 32)
        n["depth_33_or_more"] += int(d >= 33)
        n["deepest"] = max(n["deepest"], d)
    assert n["batches_alone"] >= 200 and n["serial_alone"] >= 200 and n["hand_over"] >= 200
    assert n["hand_over_with_leftover"] >= 50
    assert n["depth_32"] >= 1 and n["depth_33_or_more"] >= 1
    assert n["run_grows_in_serial_loop"] >= 200 and n["total_at_int_limit"] >= 10
    assert n["deepest"] < 64            # (the oracle's and the kernel's 64-bit code words hold every code of the corpus)
    rec = dict(sorted(n.items()))
    if WRITE:
        with open(REACH, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    with open(REACH) as f:
        assert json.load(f) == rec
