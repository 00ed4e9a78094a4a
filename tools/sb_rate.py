#!/usr/bin/env python3
"""The add with strand counts (-sb) against the add without, warmed, on the headline batch of tools/pile_rate.py
(100 Mbp, READS x 150 reads, -b -l 20, every default).  One mapping of the batch stays on the device; the two accumulators -- one
plain, one with strands enabled -- take slamem_pileup_add_device over it in turn, alternating in one process, and per mode the
median of REPS (default 5) adds' own device time (HIP events around the add's two kernels) is reported.  The yardstick of the
stranded add is the plain add OF THE SAME RUN (strands_over_plain); beside the times the atomics of the batch (two per `=` run,
one per X letter, D row and I operation), of which the reads of strand 1 issue theirs twice.
Prints one JSON line and writes it to profiles/sb_rate.json.  READS / REPS in the environment as for tools/pile_rate.py."""
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
import pile_rate  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = int(os.environ.get("REPS", 5))


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
    piles = {"plain": engine.Pileup(idx), "strands": engine.Pileup(idx, strands=True)}
    lib = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def add(pile):
        e0.record()
        capi.check(lib.slamem_pileup_add_device(pile._h, _ptr(reads), _ptr(offsets), M, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                                _ptr(m.ooff), _ptr(m.reads), 0, stream))
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))
    ms = {k: [] for k in piles}
    for p in piles.values():  # warm-up
        add(p)
    for _ in range(REPS):
        for k, p in piles.items():
            ms[k].append(add(p))
    rec = m.reads[: 3 * M].view(-1, 3)
    strand = rec[:, 2] & 0xFF
    counts = pile_rate.op_counts(m, M)
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", "reps": REPS, "reads_forward": int((strand == 1).sum().item()),
           "reads_reverse": int((strand == 2).sum().item()), "atomics": counts["atomics"], "atomics_per_read": counts["atomics_per_read"],
           "plain": {"add_ms": med(ms["plain"]), "add_ms_range": rng(ms["plain"])},
           "strands": {"add_ms": med(ms["strands"]), "add_ms_range": rng(ms["strands"])},
           "strands_over_plain": round(med(ms["strands"]) / max(med(ms["plain"]), 1e-9), 3)}
    for p in piles.values():
        p.close()
    idx.close()
    return out


if __name__ == "__main__":
    line = json.dumps(run(int(os.environ.get("READS", 10_000_000))))
    print(line)
    out = os.environ.get("SB_RATE_OUT", os.path.join(ROOT, "profiles", "sb_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
