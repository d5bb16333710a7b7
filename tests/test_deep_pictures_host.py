"""What the deep pictures (tests/deep_pictures.py) reach, by the oracle's trace: the depth of their trees,
how many tokens carry a code of 20 bits or more and in which block rows, the longest token with its extra
bits.  Asserted here and recorded in tests/golden/deep_reach.json (HIMG_WRITE_GOLDEN=1 rewrites it);
tests/test_gpu_deep_codes.py sends the same pictures through every emit form of the encoder."""
import json
import os

import numpy as np

import oracle_lib as ol
import deep_pictures as dp

REACH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deep_reach.json")
WRITE = os.environ.get("HIMG_WRITE_GOLDEN", "") == "1"
DEEP = 20                      # bits of a code that counts as long (the longest of any other encode test: about 19)
EXTRA = {257: 2, 258: 4, 259: 8, 260: 14}


def _row_tokens(row):
    """Token histogram of one block of symbols (literals, and zero runs by the reference's greedy split)."""
    h = dp._zero_tokens(row)
    h[:256] += np.bincount(row[row != 0], minlength=256)
    return h


def _reach(name):
    img, design, packed, tr = dp.traced(name)
    h, w, ch = img.shape
    rows, row_block = tr["rows"], tr["cols"] * ch * 64
    rec = {"width": w, "height": h, "pixels": w * h, "row_block": row_block, "stream_bytes": int(packed.size),
           "lres_depth": int(tr["lres_len"].max()), "fres_depth": int(tr["fres_len"].max())}
    # FRES: the tokens of every block row
    per_row = np.stack([_row_tokens(r) for r in tr["fres_sym"].reshape(rows, row_block)])
    assert np.array_equal(per_row.sum(0), tr["fres_hist"]), name
    deep = tr["fres_len"] >= DEEP
    rec["fres_deep_tokens"] = int(per_row[:, deep].sum())
    rec["fres_deep_rows"] = [int(r) for r in np.flatnonzero(per_row[:, deep].sum(1))]
    bits = tr["fres_len"].astype(int) + np.array([EXTRA.get(s, 0) for s in range(261)])
    rec["fres_longest_token_bits"] = int(bits[tr["fres_hist"] > 0].max())
    # LRES: one block
    lh = _row_tokens(tr["lres_sym"])
    assert np.array_equal(lh, tr["lres_hist"]), name
    rec["lres_deep_tokens"] = int(lh[tr["lres_len"] >= DEEP].sum())
    rc, _ = ol.oracle_decode(packed)
    rec["oracle_decodes_it"] = rc == 0
    return rec


def test_design_is_what_the_oracle_counts():
    """The generator's intended histogram is the traced one: no stray symbol, in either stream."""
    for name, strm in (("fres_wide", "fres"), ("fres_narrow", "fres"), ("lres", "lres")):
        _, design, _, tr = dp.traced(name)
        got = {int(s): int(c) for s, c in enumerate(tr[strm + "_hist"]) if c}
        assert got == design["hist"], name
    for name in ("fres_wide", "fres_narrow"):          # their low-res plane is exactly flat
        assert not dp.traced(name)[3]["lres_sym"][dp.traced(name)[3]["lres_sym"] != 254].any()
        assert (dp.traced(name)[3]["lowres"] == 128).all()


def test_deep_pictures_reach_what_they_are_for():
    rec = {name: _reach(name) for name in dp.NAMES}
    wide, narrow, lres = rec["fres_wide"], rec["fres_narrow"], rec["lres"]
    # FRES, wide: at most 4 Mpixel, 1024 wide at 4 channels (the wide emit form), a code of at least 24 bits
    assert wide["width"] == 1024 and wide["row_block"] == 32768 and wide["pixels"] <= 4 * 2 ** 20
    assert 24 <= wide["fres_depth"] <= 32
    assert wide["fres_depth"] == 32 and wide["fres_longest_token_bits"] >= 40      # what this construction gives: the legal limit
    # FRES, narrow
    assert narrow["row_block"] < 32768 and 20 <= narrow["fres_depth"] <= 32
    assert narrow["fres_depth"] == 28
    # both: at least 16 long tokens over at least 8 block rows
    for r in (wide, narrow):
        assert r["fres_deep_tokens"] >= 16 and len(r["fres_deep_rows"]) >= 8
    # LRES
    assert 20 <= lres["lres_depth"] <= 32 and lres["lres_deep_tokens"] >= 8
    assert lres["lres_depth"] == 22
    for r in rec.values():
        assert r["oracle_decodes_it"]
    if WRITE:
        with open(REACH, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(REACH) as f:
        assert json.load(f) == rec
