#!/usr/bin/env python3
"""The depth read-out of the pileup (-depth) against the read-out it spares, warmed, on the headline shape of
tools/sites_rate.py: the headline reads piled on 100 Mbp.  In one process, alternating, the medians of REPS calls (HIP events around
the device calls) of
  exact    slamem_pileup_depth_runs_device over the whole table without levels, into a device buffer of the size it asked for
  levels   the same with the levels 1,4,30
  counts   slamem_pileup_counts_device over the same rows into a device buffer, in chunks of 16 M rows
with the runs written, the bytes moved per row, the bandwidth that makes, and the ratios exact / counts and levels / counts.  What
to expect: depth_runs reads the 28 bytes a row that counts_device reads, twice, and writes 16 bytes a run where counts_device writes
24 bytes a row.  Prints one JSON line and writes it to profiles/depth_rate.json.  READS / REPS in the environment as for
tools/aln_rate.py."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import aln_rate  # noqa: E402
import pile_rate  # noqa: E402
import sites_rate  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = aln_rate.REPS
CHUNK = pile_rate.CHUNK
LEVELS = (1, 4, 30)


def time_modes(idx, pile):
    L = capi.lib()
    n = idx.n
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = C.c_uint64()
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    modes = {"exact": (None, 0), "levels": ((C.c_uint32 * len(LEVELS))(*LEVELS), len(LEVELS))}
    bufs, ms = {}, {"exact": [], "levels": [], "counts": []}
    for name, (lv, k) in modes.items():  # the sizes first
        rc = L.slamem_pileup_depth_runs_device(pile._h, 0, n, lv, k, 1, 0, None, None, 0, None, C.byref(total), stream)
        if rc not in (capi.SLAMEM_OK, capi.SLAMEM_ERR_CAPACITY):
            capi.check(rc)
        bufs[name] = torch.empty((max(1, int(total.value)), 2), dtype=torch.int64, device=dev)
    out_dev = torch.zeros((min(CHUNK, n), 6), dtype=torch.int32, device=dev)
    for rep in range(REPS + 1):  # (the first round warms; the three alternate)
        for name, (lv, k) in modes.items():
            e0.record()
            capi.check(L.slamem_pileup_depth_runs_device(pile._h, 0, n, lv, k, 1, bufs[name].shape[0], _ptr(bufs[name]), None, 0, None,
                                                         C.byref(total), stream))
            e1.record()
            e1.synchronize()
            if rep:
                ms[name].append(float(e0.elapsed_time(e1)))
        e0.record()
        for a in range(0, n, CHUNK):
            capi.check(L.slamem_pileup_counts_device(pile._h, a, min(CHUNK, n - a), _ptr(out_dev), stream))
        e1.record()
        e1.synchronize()
        if rep:
            ms["counts"].append(float(e0.elapsed_time(e1)))
    out = {"rows": n}
    for name in modes:
        runs = int(bufs[name].shape[0])
        moved = 2 * 28 * n + 16 * runs  # the table read twice (4 bytes of diff and 24 of counters a row), 16 bytes written a run
        out[name] = {"runs": runs, "ms_median": med(ms[name]), "ms_range": rng(ms[name]), "bytes_per_row": round(moved / n, 2),
                     "gb_per_s": round(moved / 1e6 / max(med(ms[name]), 1e-9), 1)}
    out["counts"] = {"ms_median": med(ms["counts"]), "ms_range": rng(ms["counts"]), "bytes_per_row": 52,
                     "gb_per_s": round(n * 52 / 1e6 / max(med(ms["counts"]), 1e-9), 1)}
    for name in modes:
        out[name + "_over_counts"] = round(out[name]["ms_median"] / max(out["counts"]["ms_median"], 1e-9), 3)
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    pile = sites_rate.pile_batch(idx, reads, offsets, M, M * L, 3 * M + 1024)
    del reads, offsets
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", **time_modes(idx, pile)}
    pile.close()
    idx.close()
    return out


if __name__ == "__main__":
    res = {"reps": REPS, "levels": list(LEVELS), "headline": headline(int(os.environ.get("READS", 10_000_000)))}
    line = json.dumps(res)
    print(line)
    out = os.environ.get("DEPTH_RATE_OUT", os.path.join(ROOT, "profiles", "depth_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
