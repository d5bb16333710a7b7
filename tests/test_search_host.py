"""The encoder's quality search as the device runs it (himg_amd/csrc/search_step.h), driven on the host
by tools/micro/search_check.cpp, against the two models -- for every quality range 0 <= qmin <= qmax
<= 100, where the GPU tests have three.  No GPU: the step is plain C++."""
import os
import subprocess

import budget_model as bm
import target_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGES = [(qmin, qmax) for qmin in range(101) for qmax in range(qmin, 101)]
BIG = 1 << 40
LIMIT = 1000


def build(tmp_path, *flags):
    exe = str(tmp_path / "search_check")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "himg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "micro", "search_check.cpp"), "-o", exe], check=True)
    return exe


def fixed_curves():
    """name -> (budget curve, target curve): values that satisfy LIMIT are <= it."""
    lcg, noise = 12345, []
    for _ in range(101):
        lcg = (lcg * 1103515245 + 12345) & 0x7FFFFFFF
        noise.append(lcg % (2 * LIMIT))   # non-monotone: about half the qualities satisfy the limit
    assert any(a < b for a, b in zip(noise, noise[1:])) and any(a > b for a, b in zip(noise, noise[1:]))
    return {
        "all-fit": ([0] * 101,) * 2,
        "none-fit": ([BIG] * 101,) * 2,
        "at-the-limit": ([LIMIT] * 101,) * 2,
        "one-above": ([LIMIT + 1] * 101,) * 2,
        "noise": (noise, noise),
    }


def cases(with_steps):
    """(the C lines' curves, [(dir, qmin, qmax, limit, curve index)])."""
    curves, out = [], []
    fixed = {}
    for name, pair in fixed_curves().items():
        fixed[name] = (len(curves), len(curves) + 1)
        curves += [list(pair[0]), list(pair[1])]
    # a step at k: budget -- the qualities below k fit; target -- the qualities from k on meet it
    step = {}
    for k in range(102):
        step[k] = (len(curves), len(curves) + 1)
        curves += [[0 if q < k else BIG for q in range(101)], [BIG if q < k else 0 for q in range(101)]]
    # "only at the required end": a step right behind qmin (budget), right at qmax (target)
    for qmin, qmax in RANGES:
        for d in (0, 1):
            for name in fixed:
                out.append((d, qmin, qmax, LIMIT, fixed[name][d]))
            out.append((d, qmin, qmax, LIMIT, step[qmin + 1 if d == 0 else qmax][d]))
            if with_steps:
                for k in range(qmin, qmax + 2):
                    out.append((d, qmin, qmax, LIMIT, step[k][d]))
    return curves, out


def run_and_compare(exe, curves, todo):
    text = "".join("C " + " ".join(map(str, c)) + "\n" for c in curves)
    text += "".join("S %d %d %d %d %d\n" % c for c in todo)
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo)
    models = (bm.search, tm.search)
    for (d, qmin, qmax, limit, ci), line in zip(todo, lines):
        q, probes = models[d](curves[ci].__getitem__, limit, qmin, qmax)
        assert len(probes) <= bm.probe_count(qmin, qmax)
        want = " ".join(map(str, [q] + probes))
        assert line == want, (d, qmin, qmax, ci, line, want)


def test_every_range_against_the_models(tmp_path):
    assert len(RANGES) == 5151
    curves, todo = cases(with_steps=True)
    run_and_compare(build(tmp_path), curves, todo)


def test_sanitized_build(tmp_path):
    """The same program under AddressSanitizer and UBSan (a stand-alone host program), on the curves
    that do not depend on the range."""
    exe = build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    curves, todo = cases(with_steps=False)
    run_and_compare(exe, curves, todo)
