"""GPU (-m gpu): the encoder's tree kernel alone (k_tree through himg_hip_debug_trees) on the histogram
corpus of tests/tree_cases.py, against the oracle's own tree builder (oracle_lib.oracle_tree) -- which
tests/test_tree_model_host.py proves equal to the plain model of tests/tree_model.py on every histogram of
the corpus; the model's 15 s of Python are spent there, once, and not here.  One workgroup per histogram,
each histogram in both stream slots of its own frame.  Bar: code lengths, codes, the serialised tree and its
byte count are equal wherever the longest code has at most 32 bits; status 3 (what an encode answers with
HIMG_ERR_UNSUPPORTED) and nothing else where it is longer."""
import numpy as np
import pytest

import oracle_lib as ol
import tree_cases as tc

pytestmark = pytest.mark.gpu

MAX_CODE_LEN = 32
STATUS_TOO_DEEP = 3


@pytest.fixture(scope="module")
def trees(engine):
    """The whole corpus through the kernel in one call."""
    cases = tc.cases()
    return engine.debug_trees(np.stack([h for _, _, h in cases]))


def test_tree_kernel_matches_the_model_on_the_corpus(trees):
    codes, lens, tree, nbytes, status = trees
    cases = tc.cases()
    want = [ol.oracle_tree(h) for _, _, h in cases]
    assert status.shape == (len(cases),)
    bad, legal, too_deep = [], 0, 0
    for i, ((family, sub, hist), (w_lens, w_codes, w_tree, w_n)) in enumerate(zip(cases, want)):
        what = "%s / %s" % (family, sub)
        if max(w_lens) > MAX_CODE_LEN:
            too_deep += 1
            if status[i] != STATUS_TOO_DEEP:
                bad.append("%s: longest code %d bits, status %d" % (what, max(w_lens), status[i]))
            continue
        legal += 1
        if status[i] != 0:
            bad.append("%s: status %d" % (what, status[i]))
            continue
        for slot in range(2):
            where = "%s, slot %d" % (what, slot)
            d = np.flatnonzero(lens[i, slot] != w_lens)
            if d.size:
                bad.append("%s: length of symbol %d is %d, the model's %d" % (where, d[0], lens[i, slot, d[0]], w_lens[d[0]]))
                break
            d = np.flatnonzero(codes[i, slot] != w_codes)
            if d.size:
                bad.append("%s: code of symbol %d is %#x, the model's %#x" % (where, d[0], int(codes[i, slot, d[0]]), int(w_codes[d[0]])))
                break
            if int(nbytes[i, slot]) != w_n:
                bad.append("%s: %d tree bytes, the model's %d" % (where, nbytes[i, slot], w_n))
                break
            got = tree[i, slot]
            if got[:w_n].tobytes() != w_tree or got[w_n:].any():
                d = np.flatnonzero(got != np.frombuffer(w_tree.ljust(got.size, b"\0"), np.uint8))
                bad.append("%s: tree byte %d differs (symbol %d by position)" % (where, d[0], d[0] * 8 // 10))
                break
    assert not bad, "%d of %d histograms differ:\n%s" % (len(bad), len(cases), "\n".join(bad[:20]))
    assert legal > 5000 and too_deep >= 50


def test_a_second_call_does_not_see_the_first(engine, trees):
    """The scratch is reused: a small call after the large one, in another order, gives each histogram the same."""
    codes, lens, tree, nbytes, status = trees
    pick = [len(tc.cases()) - 1, 0, 700, 2500, 4000]
    c2, l2, t2, n2, s2 = engine.debug_trees(np.stack([tc.cases()[i][2] for i in pick]))
    for k, i in enumerate(pick):
        assert s2[k] == status[i] and np.array_equal(l2[k], lens[i]) and np.array_equal(c2[k], codes[i])
        assert np.array_equal(n2[k], nbytes[i]) and np.array_equal(t2[k], tree[i])


def test_bad_arguments(engine):
    import himg_amd
    with pytest.raises(himg_amd.HimgError) as ei:
        engine.debug_trees(np.zeros((0, 261), np.uint32))
    assert ei.value.code == himg_amd.HIMG_ERR_ARG
