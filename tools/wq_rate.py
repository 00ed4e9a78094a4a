#!/usr/bin/env python3
"""The add with quality sums (-wq) against the add without, and the weighted genotype read-out against the plain
one, warmed, on the headline batch of tools/pile_rate.py (100 Mbp, READS x 150 reads, -b -l 20, every default).  One mapping of
the batch stays on the device.  A plain accumulator takes slamem_pileup_add_device over it and one with quality sums takes
slamem_pileup_add_quals_device, with three quality inputs in turn:
  constant   one value at every letter: two atomics per `=` run, as the counts
  binned     four values in runs, drawn per read as a sequencer bins them (run lengths 1 .. 49)
  every      a different value at every letter: the worst case, an atomic per letter
alternating in one process; per mode the median of REPS (default 5) adds' own device time (HIP events around the add's kernels)
is reported.  The yardstick is the plain add OF THE SAME RUN (quals_over_plain).  Beside the times the atomics per read of the
quality pass for each input, counted on the host from the batch's operations and the quality bytes of a sample of the reads: per
`=` run the changes of level (+ 1 to open, + 1 to close when the last level is not 0), per X letter one when its quality is not 0.
Then the read-outs over the whole text after the adds: slamem_pileup_genotypes_weighted_device against slamem_pileup_genotypes_device
on the same accumulator, the same way.  Prints one JSON line and writes it to profiles/wq_rate.json.  READS / REPS in the
environment as for tools/pile_rate.py."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import aln_rate  # noqa: E402
import map_rate  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = int(os.environ.get("REPS", 5))
SAMPLE = 20_000  # reads whose quality atomics are counted on the host
VALUES = (2, 12, 23, 37)


def quality_inputs(M, L, seed=42):
    """name -> uint8 array of M * L quality bytes (Phred + 33)"""
    rng = np.random.default_rng(seed)
    out = {"constant": np.full(M * L, 33 + 30, dtype=np.uint8)}
    # binned: run boundaries where a geometric-like draw says so (mean run about 25 letters), a new value of the four at each
    cut = rng.random(M * L) < 0.04
    cut[::L] = True  # (a read starts a run)
    vals = np.array(VALUES, dtype=np.uint8)[rng.integers(0, 4, size=int(cut.sum()))]
    out["binned"] = (33 + vals[np.cumsum(cut) - 1]).astype(np.uint8)
    out["every"] = (33 + 2 + (np.arange(M * L, dtype=np.int64) % 2) * 30 + (np.arange(M * L, dtype=np.int64) % 3)).astype(np.uint8)
    return out


def qual_atomics(m, M, L, quals, sample):
    """The atomics of the quality pass over the first `sample` reads, from the definition (a text without N, no mask)."""
    roff = m.roff[: sample + 1].cpu().numpy().astype(np.int64)
    s1 = int(roff[-1])
    segs = m.segs[: s1 * 5].cpu().numpy().view(np.uint32).reshape(-1, 5)
    ooff = m.ooff[: s1 + 1].cpu().numpy().astype(np.int64)
    ops = m.ops[: int(ooff[-1])].cpu().numpy().view(np.uint32)
    rec = m.reads[: 3 * sample].cpu().numpy().view(np.uint32).reshape(-1, 3)
    strand = rec[:, 2] & 0xFF
    total = 0
    for r in range(sample):
        if strand[r] == 0:
            continue
        v = quals[r * L:(r + 1) * L].astype(np.int64) - 33
        v = np.clip(v, 0, 93)
        if strand[r] == 2:
            v = v[::-1]
        for s in range(roff[r], roff[r + 1]):
            q = int(segs[s, 1])
            for op in ops[ooff[s]:ooff[s + 1]]:
                code, k = int(op) & 15, int(op) >> 4
                if code == 7:
                    w = v[q:q + k]
                    if len(w):
                        lv = np.concatenate([[0], w, [0]])
                        total += int((lv[1:] != lv[:-1]).sum())
                    q += k
                elif code == 8:
                    total += int((v[q:q + k] != 0).sum())
                    q += k
                elif code == 1:
                    q += k
    return total / max(sample, 1)


def run(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    cap = 3 * M + 1024
    while True:
        try:
            m = map_rate.MapRunner(idx, M, M * L, cap, cap, 2 * cap + 4096)
            m.run(reads, offsets, 20)
            break
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            cap = max(e.totals[0], e.totals[1], e.totals[2] // 2) + 1024
            del m
    inputs = quality_inputs(M, L)
    qdev = {k: torch.from_numpy(np.concatenate([v, np.zeros(8, dtype=np.uint8)])).to(dev) for k, v in inputs.items()}
    plain, wq = engine.Pileup(idx), engine.Pileup(idx, quals=True)
    lib = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    def add_plain():
        capi.check(lib.slamem_pileup_add_device(plain._h, _ptr(reads), _ptr(offsets), M, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                                _ptr(m.ooff), _ptr(m.reads), 0, stream))

    def add_quals(name):
        capi.check(lib.slamem_pileup_add_quals_device(wq._h, _ptr(reads), _ptr(offsets), M, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                                      _ptr(m.ooff), _ptr(m.reads), 0, None, _ptr(qdev[name]), 33, 0, None, None, stream))
    modes = {"plain": add_plain}
    modes.update({k: (lambda k=k: add_quals(k)) for k in inputs})
    ms = {k: [] for k in modes}
    for call in modes.values():  # warm-up
        timed(call)
    for _ in range(REPS):
        for k, call in modes.items():
            ms[k].append(timed(call))
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    sample = min(SAMPLE, M)
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", "reps": REPS, "atomics_sample_reads": sample,
           "plain": {"add_ms": med(ms["plain"]), "add_ms_range": rng(ms["plain"])}}
    for k in inputs:
        out[k] = {"add_ms": med(ms[k]), "add_ms_range": rng(ms[k]), "quals_over_plain": round(med(ms[k]) / max(med(ms["plain"]), 1e-9), 3),
                  "quality_atomics_per_read": round(qual_atomics(m, M, L, inputs[k], sample), 2)}
    # the read-outs over the whole text, on the accumulator with quality sums as the adds left it
    params = engine._gt_params(2, 20, 30, 4, 20, engine.WQ_COSTS)
    room = 1 << 22
    pos = torch.empty(room, dtype=torch.int64, device=dev)
    rows = torch.empty((room, 6), dtype=torch.int32, device=dev)
    gts = torch.empty(room * engine.GENOTYPE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    qsums = torch.empty((room, 4), dtype=torch.int32, device=dev)
    import ctypes as C
    total = C.c_uint64()

    def read_plain():
        rc = lib.slamem_pileup_genotypes_device(wq._h, 0, n, C.byref(params), room, _ptr(pos), _ptr(rows), _ptr(gts), C.byref(total), stream)
        if rc != capi.SLAMEM_ERR_CAPACITY:
            capi.check(rc)

    def read_weighted():
        rc = lib.slamem_pileup_genotypes_weighted_device(wq._h, 0, n, C.byref(params), room, _ptr(pos), _ptr(rows), _ptr(gts), _ptr(qsums),
                                                         C.byref(total), stream)
        if rc != capi.SLAMEM_ERR_CAPACITY:
            capi.check(rc)
    reads_out = {"genotypes": read_plain, "weighted": read_weighted}
    rms = {k: [] for k in reads_out}
    for call in reads_out.values():
        timed(call)
    for _ in range(REPS):
        for k, call in reads_out.items():
            rms[k].append(timed(call))
            out.setdefault("selected", {})[k] = int(total.value)
    out["readout"] = {k: {"ms": med(v), "ms_range": rng(v)} for k, v in rms.items()}
    out["readout"]["weighted_over_genotypes"] = round(med(rms["weighted"]) / max(med(rms["genotypes"]), 1e-9), 3)
    plain.close()
    wq.close()
    idx.close()
    return out


if __name__ == "__main__":
    line = json.dumps(run(int(os.environ.get("READS", 10_000_000))))
    print(line)
    out = os.environ.get("WQ_RATE_OUT", os.path.join(ROOT, "profiles", "wq_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
