"""GPU (-m gpu): the device entry points on a caller's stream -- a non-blocking torch stream, never the
null stream -- gated and unsynchronised (tests/stream_gate.py): the work runs in the order of that stream
alone, every side stream is joined back into it, no call waits for the device, and consecutive calls queued
with no host wait between them do not disturb each other's workspace, d_sizes or pinned ring slots.  Every
output is compared byte for byte with the CPU reference of its form (tests/stream_cases.py; no tolerances).

Shapes (batch 3 unless stated), the smallest that reach each stream topology:
  256 x 64 x 4     whole-tile RGBA
  200 x 72 x 4     ragged, several rows per workgroup
  520 x 64 x 3     the general form
  4608 x 16 x 4    rows wider than the LDS: the count and window passes run on the side streams
  256 x 1024 x 4   batch 1, 128 block rows: HIMG_WALK_SEGS=4 splits it into four ranges over three side streams
All forms run on 256 x 64 x 4 and 520 x 64 x 3, decode_device on all five, the encode forms on the first three.

The context's knobs are read when it is created, so every set of knobs runs in a child process
(tests/stream_runner.py), one after the other; after a failing child the others are not started.
GPU_MAX_HW_QUEUES=8 in the child: the caller's stream, the null stream and a context's three side streams do
not share a hardware queue, which would serialise them and hide a race.
"""
import os
import pickle
import subprocess
import sys

import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = [
    ("default", {}),
    ("no-side-stream", {"HIMG_SIDE_STREAM": "0"}),
    ("row-ranges", {"HIMG_WALK_SEGS": "4"}),
    ("row-ranges-generic", {"HIMG_WALK_SEGS": "4", "HIMG_FORCE_UNFUSED": "1"}),
]
_failed = []


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """The case table, built once on the host and shared by the children."""
    path = tmp_path_factory.mktemp("streams") / "cases.pkl"
    with open(path, "wb") as f:
        pickle.dump(sc.build(), f, protocol=pickle.HIGHEST_PROTOCOL)
    return str(path)


@pytest.mark.parametrize("name,knobs", KNOBS, ids=[k[0] for k in KNOBS])
def test_entry_points_on_a_gated_stream(table, name, knobs):
    assert not _failed, "not started: the child %r failed before this one" % _failed[0]
    env = {k: v for k, v in os.environ.items() if k not in ("HIMG_SIDE_STREAM", "HIMG_WALK_SEGS", "HIMG_FORCE_UNFUSED")}
    env.update(knobs, GPU_MAX_HW_QUEUES="8")
    _failed.append(name)
    r = subprocess.run([sys.executable, os.path.join(HERE, "stream_runner.py"), table], env=env, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "streams ok" in r.stdout, r.stdout[-12000:] + r.stderr[-4000:]
    _failed.pop()
