"""The planning of a call on an opened-streams handle (himg_amd/csrc/opened_plan.h), driven on the host by
tools/micro/opened_plan_check.cpp, against a small model over seeded sequences of calls.  No GPU: the plan is
plain C++."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, *flags):
    exe = str(tmp_path / "opened_plan_check")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "himg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "micro", "opened_plan_check.cpp"), "-o", exe], check=True)
    return exe


class Model:
    """The rows a handle has counted, as a set; a call's list from it."""

    def __init__(self, n_streams, rows):
        self.n_streams, self.rows, self.counted = n_streams, rows, set()

    def call(self, wins, h, chunk, mark=True):
        touched = {(s, r) for s, _, y in wins for r in range(y // 8, (y + h + 7) // 8)}
        new = sorted(touched - self.counted)
        runs = []
        for s, r in new:   # maximal runs of new rows (an old or untouched row between two is a gap), cut into entries
            if runs and runs[-1][0] == s and runs[-1][2] == r:
                runs[-1][2] = r + 1
            else:
                runs.append([s, r, r + 1])
        entries = []
        for s, a, b in runs:
            for x in range(a, b, chunk):
                entries.append((s, x, min(x + chunk, b)))
        if mark:
            self.counted |= set(new)
        return entries, len(new), touched


def sequences():
    """(n_streams, rows, [(op, h, chunk, windows)]): seeded calls, then the edges."""
    rng = np.random.default_rng(41)
    out = []
    for n_streams, rows in [(1, 9), (3, 9), (5, 40), (2, 1), (4, 2048)]:
        H = 8 * rows - int(rng.integers(0, 8))
        calls = []
        for _ in range(12):
            h = int(rng.integers(1, min(H, 200) + 1))
            n = int(rng.integers(1, 30))
            chunk = int(rng.choice([1, 2, 4, 16]))
            wins = [(int(rng.integers(0, n_streams)), int(rng.integers(0, 50)), int(rng.integers(0, H - h + 1))) for _ in range(n)]
            calls.append(("R" if rng.integers(0, 6) == 0 else "C", h, chunk, wins))
            if rng.integers(0, 3) == 0:
                calls.append(("C", h, chunk, wins))   # the same call again
                calls.append(("C", h, chunk, wins))
        out.append((n_streams, rows, calls))
    # a window at the last block row; one window; a stream that no window names (stream 1 of 3)
    out.append((3, 9, [("C", 17, 1, [(0, 0, 55)]), ("C", 1, 1, [(2, 5, 71)]), ("C", 72, 4, [(0, 0, 0), (2, 0, 0)]),
                       ("C", 72, 4, [(0, 0, 0), (2, 0, 0)])]))
    # 65535 windows over every row of two streams, then again
    many = [(k % 2, 0, (k * 7) % (8 * 600 - 16)) for k in range(65535)]
    out.append((2, 600, [("C", 17, 16, many), ("C", 17, 16, many), ("C", 1, 16, [(1, 0, 8 * 600 - 1)])]))
    return out


def run_and_compare(exe, seqs):
    text = []
    for n_streams, rows, calls in seqs:
        text.append("H %d %d" % (n_streams, rows))
        for op, h, chunk, wins in calls:
            text.append("%s %d %d %d " % (op, len(wins), h, chunk) + " ".join("%d %d %d" % w for w in wins))
    r = subprocess.run([exe], input="\n".join(text) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = iter(r.stdout.splitlines())
    for n_streams, rows, calls in seqs:
        m = Model(n_streams, rows)
        listed, touched_all, prev = [], set(), None
        for op, h, chunk, wins in calls:
            v = [int(x) for x in next(lines).split()]
            n_list, list_rows, counted = v[:3]
            got = [tuple(v[3 + 3 * i:6 + 3 * i]) for i in range(n_list)]
            before = set(m.counted)
            want, n_new, touched = m.call(wins, h, chunk, mark=op == "C")
            assert got == want, (n_streams, rows, op, h, chunk, got[:6], want[:6])
            assert list_rows == n_new and counted == len(m.counted)
            # entries never exceed the chunk, hold only rows the call touches, and none counted before
            for s, a, b in got:
                assert 0 < b - a <= chunk and 0 <= a and b <= rows and 0 <= s < n_streams
                assert all((s, r) in touched and (s, r) not in before for r in range(a, b))
            if op == "C":
                listed += [(s, r) for s, a, b in got for r in range(a, b)]
                touched_all |= touched
                if prev == (h, wins):
                    assert got == []   # a repeated call lists nothing
                prev = (h, wins)
            else:
                assert m.counted == before   # a refused call marks nothing
        # every touched (stream, row) exactly once over the sequence, and no other
        assert len(listed) == len(set(listed)) and set(listed) == touched_all
    assert next(lines, None) is None


def test_sequences_against_the_model(tmp_path):
    seqs = sequences()
    assert any(len(w) == 65535 for _, _, c in seqs for _, _, _, w in c) and any(len(w) == 1 for _, _, c in seqs for _, _, _, w in c)
    run_and_compare(build(tmp_path), seqs)


def test_sanitized_build(tmp_path):
    """The same program under AddressSanitizer and UBSan (a stand-alone host program)."""
    exe = build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    run_and_compare(exe, sequences())
