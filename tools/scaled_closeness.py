#!/usr/bin/env python3
"""Writes profiles/scaled_closeness.json: how close the scaled decode (its numpy model,
tests/scaled_model.py) is to the shrunken full decode, per picture, quality, colour space and
scale.  CPU only; tests/test_scaled_host.py recomputes the table and compares."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import himg_amd          # noqa: E402
import scaled_model as sm  # noqa: E402


def main():
    rows = sm.closeness_table(himg_amd.synth)
    out = {"what": "M = scaled decode (model), T = rounded box mean of the oracle's full decode, O = box mean of the "
                   "original; RGBA pictures from himg_synth_fill, seed 3; PSNR in dB",
           "asserted": "psnr_M_T > psnr_T_O for q <= 90", "dropped_from_assertion": [], "cases": rows}
    path = os.path.join(ROOT, "profiles", "scaled_closeness.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    dec = [r for r in rows if "psnr_M_T" in r]
    miss = [r for r in dec if r["q"] <= 90 and not r["psnr_M_T"] > r["psnr_T_O"]]
    print("%d cases, %d decodable, %d asserted, %d miss the relation" % (
        len(rows), len(dec), sum(1 for r in dec if r["q"] <= 90), len(miss)))
    for r in miss:
        print(r)


if __name__ == "__main__":
    main()
