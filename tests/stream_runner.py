"""The child process of tests/test_gpu_streams.py: runs the case table (tests/stream_cases.py, pickled by
the parent) through the stream gate (tests/stream_gate.py) on one set of context knobs, which the parent
puts into this process's environment.

    python stream_runner.py CASES.pkl [PARTS [REPEAT]]        (PARTS: letters of "ABCD", the default)

Parts: A one gated call per case; B sequences on one warm context and one stream with no host wait between
the calls; C two contexts on two streams, issued interleaved; D one context moved from one stream to
another behind the caller's event.  Prints what it measured, then "streams ok"; a mismatch is listed and the
exit status is 1; a HIP error ends the run at once.

Test infrastructure only.
"""
import os
import pickle
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import himg_amd                      # noqa: E402
import stream_cases as sc            # noqa: E402
import stream_gate as sg             # noqa: E402
import tensor_model as tm            # noqa: E402

RING_SLOTS = 4     # the pinned ring that carries h_sizes, origins and qualities (stage_words)


class Job:
    """One case with its buffers: issue() is the engine call, check() the byte comparison."""

    def __init__(self, torch, case):
        self.case, self.id, self.form, self.args = case, case["id"], case["form"], case["args"]
        self.W, self.H, self.C, self.B = case["geom"]
        outs = {name: (o["want"].nbytes, o["init"]) for name, o in case["outs"].items()}
        self.buf = sg.Buffers(torch, case["real"], case["decoy"], outs)
        a = self.args
        self.tensor = tm.DESCS[a["kind"]](a["dtype"], a["co"]) if "kind" in a else None
        self.dst = himg_amd.dst_desc(**a["dst"]) if "dst" in a else None
        self.src = himg_amd.src_desc(**a["src"]) if "src" in a else None
        self.host_s = 0.0

    def o(self, name):
        return self.buf.outs[name][0]

    def issue(self, eng, stream):
        a, d, o = self.args, self.buf.d_in, self.o
        W, H, C, B = self.W, self.H, self.C, self.B
        f = self.form
        dec = (d, a.get("in_stride"), a.get("sizes"), B, W, H, C)
        enc = (d, B, W, H, C, C)
        if f == "decode":
            eng.decode_device(*dec, o("pix"), o("status"), stream)
        elif f == "preview":
            eng.preview_device(*dec, o("pix"), o("status"), stream)
        elif f == "region":
            eng.decode_region_device(*dec, a["x"], a["y"], a["w"], a["h"], o("pix"), o("status"), stream)
        elif f == "regions":
            eng.decode_regions_device(*dec, a["origins"], a["w"], a["h"], o("pix"), o("status"), stream)
        elif f == "scaled":
            eng.decode_scaled_device(*dec, a["scale"], o("pix"), o("status"), stream)
        elif f == "scaled_regions":
            eng.decode_scaled_regions_device(*dec, a["scale"], a["origins"], a["w"], a["h"], o("pix"), o("status"), stream)
        elif f == "tensor":
            eng.decode_tensor_device(*dec, self.tensor, o("pix"), o("status"), stream)
        elif f == "regions_tensor":
            eng.decode_regions_tensor_device(*dec, a["origins"], a["w"], a["h"], self.tensor, o("pix"), o("status"), stream)
        elif f == "into":
            eng.decode_into_device(*dec, o("canvas"), self.dst, a["origins"], o("status"), stream)
        elif f == "regions_into":
            eng.decode_regions_into_device(*dec, a["src_origins"], a["w"], a["h"], o("canvas"), self.dst, a["dst_origins"],
                                           o("status"), stream)
        elif f == "prefix":
            eng.decode_prefix_device(*dec, o("pix"), o("rows"), o("status"), stream)
        elif f == "pyramid":
            pyr = himg_amd.pyramid_desc(o("level0"), o("level1"), o("level2"), o("level3"))
            eng.decode_pyramid_device(*dec, pyr, o("status"), stream)
        elif f == "conceal":
            eng.decode_conceal_device(*dec, o("pix"), o("concealed"), o("rowmap"), o("status"), stream)
        elif f == "rows":
            eng.decode_rows_device(d, int(a["sizes"][0]), W, H, C, a["row0"], a["row1"], o("pix"), o("status"), stream)
        elif f == "encode":
            eng.encode_device(*enc, a["quality"], True, o("out"), a["out_stride"], o("sizes"), o("status"), stream)
        elif f == "encode_q":
            eng.encode_device_q(*enc, a["qualities"], True, o("out"), a["out_stride"], o("sizes"), o("status"), stream)
        elif f == "sizes":
            eng.encode_sizes_device(*enc, a["qualities"], True, o("sizes"), o("status"), stream)
        elif f == "sse":
            eng.encode_sse_device(*enc, a["qualities"], True, o("sse"), o("status"), stream)
        elif f == "budget":
            eng.encode_budget_device(*enc, a["qmin"], a["qmax"], True, a["budgets"], o("out"), a["out_stride"], o("sizes"),
                                     o("quality"), o("status"), stream)
        elif f == "target":
            eng.encode_target_device(*enc, a["qmin"], a["qmax"], True, a["targets"], o("out"), a["out_stride"], o("sizes"),
                                     o("quality"), o("sse"), o("status"), stream)
        elif f == "windows":
            eng.encode_windows_device(d, self.src, B, C, a["origins"], a["w"], a["h"], a["qualities"], True, o("out"),
                                      a["out_stride"], o("sizes"), o("status"), stream)
        else:
            raise KeyError(f)

    def check(self, what):
        """The outputs in pinned memory against the case's bytes: a list of findings (empty: all equal)."""
        bad = []
        for name, spec in self.case["outs"].items():
            got = self.buf.result(name)
            want = spec["want"].reshape(-1).view(np.uint8)
            ne = got != want
            if spec["mask"] is not None:
                ne &= np.repeat(spec["mask"].reshape(-1), want.size // spec["mask"].size)
            if ne.any():
                init = spec["init"]
                untouched = bool((got == (init if isinstance(init, int) else np.asarray(init).reshape(-1))).all())
                at = int(np.flatnonzero(ne)[0])
                bad.append("%s: %s: %s: %d of %d bytes differ, first at %d (got %d, want %d)%s" % (
                    what, self.id, name, int(ne.sum()), want.size, at, got[at], want[at],
                    "; the buffer is as it was before the call" if untouched else ""))
        return bad


class Runner:
    def __init__(self, cases):
        import torch
        self.torch = torch
        self.log = lambda *a: print(*a, flush=True)
        self.gate = sg.Gate(self.log)
        self.S = self.gate.self_check()
        if self.S is None:
            raise SystemExit("inconclusive: no torch stream ran independently of the null stream, so an engine "
                             "operation on the wrong stream could not be seen")
        self.jobs = {c["id"]: Job(torch, c) for c in cases}
        self.engines = {}
        self.warm = set()
        self.findings = []
        self.gates_ms = []
        self.longest = (0.0, None)

    def engine(self, case, which="main"):
        key = (which, bool(case["fix"]), tuple(sorted(case["opts"].items())))
        if key not in self.engines:
            e = himg_amd.Engine(0)
            e.set_option("fix_t2", int(case["fix"]))
            for k, v in case["opts"].items():
                e.set_option(k, v)
            self.engines[key] = e
        return self.engines[key]

    def warm_up(self, job, eng, s):
        """The case ungated on s, twice: the first call reserves (and may wait for the device), the second is
        timed on the host and compared.  Per stream: the HIP runtime sets a hardware queue up for a kernel's
        needs (scratch memory) at the kernel's first launch there, and stalls the host and every queue for it."""
        if (id(eng), job.id, id(s)) in self.warm:
            return
        torch = self.torch
        job.buf.reset()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            job.buf.queue_input()
        job.issue(eng, s.cuda_stream)
        s.synchronize()
        job.host_s = max(job.host_s, sg.timed_call(lambda: job.issue(eng, s.cuda_stream)))
        with torch.cuda.stream(s):
            job.buf.queue_collect()
        s.synchronize()
        self.findings += job.check("warm-up (ungated)")
        if job.host_s > self.longest[0]:
            self.longest = (job.host_s, job.id)
        self.warm.add((id(eng), job.id, id(s)))

    def gated(self, what, steps, gated_streams, closed_upto, moved=False):
        """steps: [(job, engine, stream)] issued in order with no host wait; gated_streams are shut first.
        moved: a step on another stream than the one before waits there for an event recorded behind that one.
        The first closed_upto calls must return while the gate is shut."""
        torch = self.torch
        for job, eng, s in steps:
            self.warm_up(job, eng, s)
        ms = sg.gate_ms(sum(job.host_s for job, _, _ in steps))
        self.gates_ms.append(ms)
        for job, _, _ in steps:
            job.buf.reset()
        torch.cuda.synchronize()
        # ---- from here to the wait: no device-wide synchronise, no .cpu(), nothing on the default stream
        t_shut = time.perf_counter()
        opened = [self.gate.shut(s, ms) for s in gated_streams]
        early, prev, t0, line = [], None, time.perf_counter(), []
        for i, (job, eng, s) in enumerate(steps):
            if moved and prev is not None and prev is not s:
                ev = torch.cuda.Event()
                ev.record(prev)
                s.wait_event(ev)
            with torch.cuda.stream(s):
                job.buf.queue_input()
            t1 = time.perf_counter()
            job.issue(eng, s.cuda_stream)
            t2 = time.perf_counter()
            if i < closed_upto and any(e.query() for e in opened):
                early.append(job.id)
            with torch.cuda.stream(s):
                job.buf.queue_collect()
            line.append("%s: input queued at %.2f ms, call %.2f ms, outputs queued at %.2f ms" % (
                job.id, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t0) * 1e3))
            prev = s
        dones = []
        for s in {id(s): s for _, _, s in steps}.values():
            e = torch.cuda.Event()
            e.record(s)
            dones.append(e)
        for e in dones:
            e.synchronize()
        # ----
        if early:
            self.log("%s: shutting took the host %.2f ms; the device held the gate(s) shut for %s ms; the host's "
                     "timeline behind:\n  %s" % (what, (t0 - t_shut) * 1e3,
                                                 ", ".join("%.1f" % e.shut_at.elapsed_time(e) for e in opened), "\n  ".join(line)))
        for jid in early:
            self.findings.append("%s: %s: the gate (%.0f ms) was open when the call returned: the call waited for "
                                 "the device, or the host was slower than the gate is long" % (what, jid, ms))
        for job, _, _ in steps:
            self.findings += job.check(what)

    def run(self, cases, parts="ABCD", repeat=1):
        S, by_id = self.S, {c["id"]: c for c in cases}
        one = lambda jid, which="main": (self.jobs[jid], self.engine(by_id[jid], which), S)
        S2 = self.torch.cuda.Stream()
        for _ in range(repeat):
            if "A" in parts:   # one gated call per form
                for jid in sc.single_ids(cases):
                    self.gated("A", [one(jid)], [S], 1)
                self.log("A done: %d cases, %d findings" % (len(sc.single_ids(cases)), len(self.findings)))
            if "B" in parts:   # sequences behind one gate
                for name, ids in sc.SEQUENCES.items():
                    self.gated("B %s" % name, [one(j) for j in ids], [S], min(len(ids), RING_SLOTS))
                self.log("B done: %d findings" % len(self.findings))
            if "C" in parts:   # two contexts on two streams, interleaved
                enc = [(self.jobs[j], self.engine(by_id[j], "second"), S2) for j in sc.TWO_CONTEXTS["encode"]]
                dec = [one(j) for j in sc.TWO_CONTEXTS["decode"]]
                steps = [x for pair in zip(enc, dec) for x in pair]
                self.gated("C", steps, [S, S2], 2 * RING_SLOTS)
                self.log("C done: %d findings" % len(self.findings))
            if "D" in parts:   # one context moved from S to S2 behind the caller's event
                a, b = sc.MOVED
                self.gated("D", [one(a), (self.jobs[b], self.engine(by_id[b]), S2)], [S], 2, moved=True)
                self.log("D done: %d findings" % len(self.findings))
        self.log("longest warm call: %.3f ms (%s); gate lengths used: %.0f .. %.0f ms over %d gates" % (
            self.longest[0] * 1e3, self.longest[1], min(self.gates_ms), max(self.gates_ms), len(self.gates_ms)))


def main():
    with open(sys.argv[1], "rb") as f:
        cases = pickle.load(f)
    print("knobs:", {k: v for k, v in os.environ.items() if k.startswith("HIMG_") or k == "GPU_MAX_HW_QUEUES"}, flush=True)
    r = Runner(cases)
    r.run(cases, *(sys.argv[2:3] or ["ABCD"]), repeat=int((sys.argv[3:4] or [1])[0]))
    for x in r.findings:
        print("FINDING", x, flush=True)
    if r.findings:
        return 1
    print("streams ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
