"""bench.py's contract, exercised the way the driver runs it: one JSON line on stdout
with the fields the harness reads, for N = 1 and -- launched by bench.py itself, two
ranks sharing the one GPU of the test box (--oversubscribe: gloo + CPU staging for the
collectives, not a measurement) -- for N = 2 in both modes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline"]


def _run(args, timeout=900):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_help_lists_the_contract_flags():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs", "--no-rows", "--rows-timeout"):
        assert flag in r.stdout


@pytest.mark.gpu
def test_single_gpu_line():
    d = _run(["--batch", "4", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-extras", "--no-rows"])
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["value"] > 1000 and d["vs_baseline"] is None
    assert "4096x4096" in d["config"]["workload"] and "bit_exact" in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3


@pytest.mark.gpu
def test_single_gpu_line_with_extras():
    """The --full run's side measurements (copy ceilings incl. the hand-written calibration
    kernels, single-frame latency, host API) on a tiny batch: they must not take the line down."""
    d = _run(["--full", "--batch", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-rows"])
    ex = d["extras"]
    assert ex["hbm_copy_ceiling_GBs"] > 500
    assert ex["single_frame_latency_ms"]["encode"] > 0 and ex["single_frame_latency_ms"]["decode"] > 0
    if os.path.exists(os.path.join(ROOT, "himg_amd", "bin", "hbm_calib")):
        k = ex["hbm_ceiling_kernels_GBs"]
        assert k["read_only"] > 1000 and k["write_only"] > 1000 and k["copy_read_plus_write"] > 1000


@pytest.mark.gpu
def test_two_ranks_self_launched_frames():
    d = _run(["--gpus", "2", "--oversubscribe", "--batch", "2", "--steps", "2", "--warmup", "1",
              "--no-cpu-baseline", "--no-extras", "--no-rows"])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert "2 rank" in d["config"]["parallelism"]


@pytest.mark.gpu
def test_two_ranks_self_launched_rows():
    d = _run(["--gpus", "2", "--oversubscribe", "--mode", "rows", "--width", "1024", "--height", "1024",
              "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-extras"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"


@pytest.mark.gpu
def test_eight_ranks_self_launched_frames_and_rows():
    """`python bench.py --gpus 8` as the driver's 8-GPU box will run it -- the launcher, eight
    ranks, the seed split, the max-over-ranks reduction, then the `rows` leg (row-sharded encode
    and decode of one frame over the same eight ranks) -- executed once before that box is its
    first execution: all ranks share the one GPU here (--oversubscribe: gloo + CPU staging,
    not a measurement), one frame per rank and a 2048 x 2048 frame for the rows leg (256 block
    rows: sixteen-row shares for all eight ranks)."""
    d = _run(["--gpus", "8", "--oversubscribe", "--full", "--batch", "1", "--steps", "1", "--warmup", "1",
              "--no-cpu-baseline", "--no-extras", "--rows-size", "2048x2048", "--rows-timeout", "600"], timeout=1500)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 8 and d["scaling"] == "weak" and d["steps"] == 1
    assert "8 rank" in d["config"]["parallelism"]
    assert d["config"]["bit_exact"]          # every rank's frames checked against the golden table before timing
    rows = d["rows"]
    assert "error" not in rows, rows
    assert "2048x2048" in rows["workload"].replace(" ", "")
    assert rows["bit_exact"] == {"stream": "oracle", "pixels": "oracle"}, rows
    assert rows["encode_ms"]["mean"] > 0 and rows["decode_ms"]["mean"] > 0


# --dump-outputs: what the last timed step returned, modelled here in numpy (independent of bench.py's
# torch code) from the streams and pixels themselves.
def _checksum(b):
    P, acc = (1 << 31) - 1, 0
    for c0 in range(0, b.size, 1 << 22):
        j = np.arange(c0, min(b.size, c0 + (1 << 22)), dtype=np.int64)
        acc = (acc + int((b[c0:c0 + j.size].astype(np.int64) * ((j + 1) * 2654435761 % P)).sum())) % P
    return float(acc)


def _expected_dump(streams, pixels, samples, seed):
    rng = np.random.default_rng(seed)
    flat_pix = np.concatenate([p.ravel() for p in pixels])
    idx = np.arange(flat_pix.size) if flat_pix.size <= samples else np.sort(rng.integers(0, flat_pix.size, samples))
    flat_enc = np.concatenate(streams)
    v = np.arange(flat_enc.size) if flat_enc.size <= samples else np.sort(rng.integers(0, flat_enc.size, samples))
    return {"encoded_sizes": np.array([s.size for s in streams], np.float64),
            "encoded_checksum": np.array([_checksum(s) for s in streams]),
            "decoded_checksum": np.array([_checksum(p.ravel()) for p in pixels]),
            "encoded_sample": flat_enc[v].astype(np.float32),
            "decoded_sample": flat_pix[idx].astype(np.float32)}


def _check_dump(path, want, n_frames):
    for name, w in want.items():
        got = np.load(os.path.join(path, name + ".npy"))
        assert got.dtype in (np.float32, np.float64), name
        assert np.array_equal(got, w), name
    for name in ("encode_status", "decode_status"):
        got = np.load(os.path.join(path, name + ".npy"))
        assert got.dtype == np.float64 and got.shape == (n_frames,) and not got.any(), name
    assert sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path)) <= 64 * 1000 * 1000


@pytest.mark.parametrize("samples", [1 << 22, 1000])
def test_dump_outputs_writes_what_the_step_returned(tmp_path, monkeypatch, samples):
    """CPU: bench.dump_outputs on host tensors, every byte (small batch) and a seeded sample."""
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLES", samples)
    rng = np.random.default_rng(1)
    sizes = [4000, 17, 4999]
    d_out = torch.from_numpy(rng.integers(0, 256, (3, 5000), dtype=np.uint8))
    d_pix = torch.from_numpy(rng.integers(0, 256, (3, 24, 16, 4), dtype=np.uint8))
    zeros = torch.zeros(3, dtype=torch.int32)
    bench.dump_outputs(torch, str(tmp_path), d_out, torch.tensor(sizes, dtype=torch.int32), zeros, d_pix, zeros)
    streams = [d_out[i, :n].numpy() for i, n in enumerate(sizes)]
    _check_dump(str(tmp_path), _expected_dump(streams, list(d_pix.numpy()), samples, bench.DUMP_SEED), 3)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_as_the_oracle_computes_it(tmp_path):
    """A plain run (no --full): the headline fields, none of --full's objects, and a dump that equals
    the oracle's streams and pixels for the same seeded frames."""
    import bench
    import himg_amd
    import oracle_lib as ol
    d = _run(["--batch", "2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d, k
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    for k in ("rows", "extras", "cpu_baseline", "step_ms", "encode_mpx_s"):
        assert k not in d, k
    streams, pixels = [], []
    for seed in (0, 1):
        s = ol.oracle_encode(himg_amd.synth("randtile", seed, 4096, 4096), 50, True)
        rc, p = ol.oracle_decode(s, threads=0)
        assert rc == 0
        streams.append(s)
        pixels.append(p)
    _check_dump(str(tmp_path), _expected_dump(streams, pixels, bench.DUMP_SAMPLES, bench.DUMP_SEED), 2)
