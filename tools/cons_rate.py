#!/usr/bin/env python3
"""The consensus read-out of the pileup (-cons) against what it replaces, warmed, on the headline shape of
tools/pile_rate.py: the headline reads piled on 100 Mbp, events enabled.  In one process, the medians of REPS calls (HIP events
around the device calls, the wall clock around the host route) of
  consensus    slamem_pileup_consensus_device over the whole table at the default depth (4) into device memory, in chunks of
               16 M rows
  counts       slamem_pileup_counts_device over the same rows into a device buffer, in the same chunks: the dense read-out of
               the same rows, 24 bytes written a row against 1
  host_route   slamem_pileup_counts_host of the whole table in the same chunks and slamem_pileup_events_host of the whole text:
               what a host needs in its memory before it can start on the same answer (wall clock; the loop over the rows is not
               in it)
with the bytes of the consensus, its five statistics and the ratios consensus / counts and host_route / consensus.  The
consensus reads what counts reads and writes a twenty-fourth of it, so consensus_over_counts should not be above 1 in the same
run.  Prints one JSON line and writes it to profiles/cons_rate.json.  READS / REPS in the environment as for tools/aln_rate.py."""
import ctypes as C
import json
import os
import sys
import time

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
REPS = aln_rate.REPS
CHUNK = pile_rate.CHUNK
MIN_DEPTH = 4


def pile_batch(idx, q_dev, off_dev, nq, qbytes, cap):
    c = cap
    while True:
        try:
            m = map_rate.MapRunner(idx, nq, qbytes, c, c, 2 * c + 4096)
            m.run(q_dev, off_dev, 20)
            break
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            c = max(e.totals[0], e.totals[1], e.totals[2] // 2) + 1024
            del m
    pile = engine.Pileup(idx, events=True)
    capi.check(capi.lib().slamem_pileup_add_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                                   _ptr(m.ooff), _ptr(m.reads), 0, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    del m
    return pile


def time_modes(idx, pile):
    L = capi.lib()
    n = idx.n
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total, stats = C.c_uint64(), (C.c_uint64 * 5)()
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    out = {"rows": n}
    k = min(CHUNK, n)
    seq = torch.empty(k + k // 8 + 4096, dtype=torch.uint8, device=dev)
    ms, size, sums = [], 0, [0] * 5
    for rep in range(REPS + 1):  # (the first one warms)
        size, sums = 0, [0] * 5
        e0.record()
        for a in range(0, n, CHUNK):
            capi.check(L.slamem_pileup_consensus_device(pile._h, a, min(CHUNK, n - a), MIN_DEPTH, seq.numel(), _ptr(seq), None, 0, None,
                                                        stats, C.byref(total), stream))
            size += int(total.value)
            sums = [x + int(y) for x, y in zip(sums, stats)]
        e1.record()
        e1.synchronize()
        if rep:
            ms.append(float(e0.elapsed_time(e1)))
    del seq
    moved = 2 * 29 * n + size  # the table read twice (4 bytes of diff, 24 of counters and the flag byte a row), the bytes written
    out["consensus"] = {"bytes": size, "stats": sums, "ms_median": med(ms), "ms_range": rng(ms), "bytes_per_row": round(moved / n, 2),
                        "gb_per_s": round(moved / 1e6 / max(med(ms), 1e-9), 1)}
    out_dev = torch.zeros((k, 6), dtype=torch.int32, device=dev)
    ms = []
    for rep in range(REPS + 1):
        e0.record()
        for a in range(0, n, CHUNK):
            capi.check(L.slamem_pileup_counts_device(pile._h, a, min(CHUNK, n - a), _ptr(out_dev), stream))
        e1.record()
        e1.synchronize()
        if rep:
            ms.append(float(e0.elapsed_time(e1)))
    del out_dev
    out["counts"] = {"ms_median": med(ms), "ms_range": rng(ms), "bytes_per_row": 52, "gb_per_s": round(n * 52 / 1e6 / max(med(ms), 1e-9), 1)}
    host = np.zeros((k, 6), dtype=np.uint32)
    ms = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        for a in range(0, n, CHUNK):
            capi.check(L.slamem_pileup_counts_host(pile._h, a, min(CHUNK, n - a), host.ctypes.data))
        ev, _ = pile.events()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
    out["host_route"] = {"ms_median": med(ms), "ms_range": rng(ms), "events": len(ev), "bytes_per_row": 24}
    out["consensus_over_counts"] = round(out["consensus"]["ms_median"] / max(out["counts"]["ms_median"], 1e-9), 3)
    out["host_route_over_consensus"] = round(out["host_route"]["ms_median"] / max(out["consensus"]["ms_median"], 1e-9), 1)
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    pile = pile_batch(idx, reads, offsets, M, M * L, 3 * M + 1024)
    del reads, offsets
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20, events enabled", **time_modes(idx, pile)}
    pile.close()
    idx.close()
    return out


if __name__ == "__main__":
    res = {"reps": REPS, "min_depth": MIN_DEPTH, "headline": headline(int(os.environ.get("READS", 10_000_000)))}
    line = json.dumps(res)
    print(line)
    out = os.environ.get("CONS_RATE_OUT", os.path.join(ROOT, "profiles", "cons_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
