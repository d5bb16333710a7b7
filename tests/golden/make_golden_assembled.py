"""Regenerate tests/golden/assembled_streams.json: per assembled stream (tests/assembled_cases.py) the
sha256 of its bytes, who judged it, the verdict and the sha256 of the pixels.  The judge is the REAL
reference (oracle/_ref, which must be built) wherever its behaviour is defined, the oracle elsewhere.

    python tests/golden/make_golden_assembled.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import assembled_cases as ac   # noqa: E402
import oracle_lib as ol        # noqa: E402


def main():
    assert ol.have_ref(), "build oracle/_ref first (make -C oracle)"
    out = {}
    for key in ac.CASES:
        c = ac.case(*key)
        by_ref = ac.reference_judges(key)
        rc, pix = ol.ref_decode(c.stream) if by_ref else ol.oracle_decode(c.stream)
        out[c.id] = {"sha256": c.sha(), "judge": "reference" if by_ref else "oracle", "accepted": rc == 0,
                     "pixels_sha256": hashlib.sha256(pix.tobytes()).hexdigest() if rc == 0 else None}
        ac.case.cache_clear()
    with open(os.path.join(HERE, "assembled_streams.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d streams, %d accepted" % (len(out), sum(v["accepted"] for v in out.values())))


if __name__ == "__main__":
    main()
