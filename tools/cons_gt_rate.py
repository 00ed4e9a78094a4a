#!/usr/bin/env python3
"""The consensus by genotype likelihood beside the plurality consensus it stands next to, warmed, on
the headline shape of tools/cons_rate.py: the headline reads piled on 100 Mbp with events and quality sums enabled (every letter
at quality 30).  In one process, alternating the three, the medians of REPS calls (HIP events around the device calls) of
  plurality   slamem_pileup_consensus_device over the whole table at the default depth (4) into device memory, in chunks of
              16 M rows
  genotype    slamem_pileup_consensus_gt_device over the same rows, ploidy 2, -gt's default costs, least GQ 20
  weighted    the same with the quality sums (-wq's costs): a second accumulator read beside the first
with the bytes and the statistics of each and the ratios genotype / plurality and weighted / plurality.  No ratio is fixed in
advance: the figure to read the two against is the plurality read-out of the same run.  Prints one JSON line and writes it to
profiles/cons_gt_rate.json.  READS / REPS in the environment as for tools/aln_rate.py."""
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
import map_rate  # noqa: E402
import pile_rate  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = int(os.environ.get("REPS", 5))
CHUNK = pile_rate.CHUNK
MIN_DEPTH, MIN_GQ, QUALITY = 4, 20, 30


def pile_batch(idx, q_dev, off_dev, nq, qbytes, cap):
    """The batch mapped and piled with events and quality sums, every letter at QUALITY."""
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
    pile = engine.Pileup(idx, events=True, quals=True)
    quals = torch.full((qbytes + 8,), 33 + QUALITY, dtype=torch.uint8, device=dev)
    capi.check(capi.lib().slamem_pileup_add_quals_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                                         _ptr(m.ooff), _ptr(m.reads), 0, None, _ptr(quals), 33, 0, None, None,
                                                         torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    del m, quals
    return pile


def time_modes(idx, pile):
    L = capi.lib()
    n = idx.n
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = C.c_uint64()
    k = min(CHUNK, n)
    seq = torch.empty(k + k // 8 + 4096, dtype=torch.uint8, device=dev)
    row = engine._gt_params(2, 20, 30, MIN_DEPTH, 0)
    params = {"genotype": capi.ConsGtParams(row, row, MIN_DEPTH, MIN_GQ, 0),
              "weighted": capi.ConsGtParams(engine._gt_params(2, 20, 30, MIN_DEPTH, 0, engine.WQ_COSTS), row, MIN_DEPTH, MIN_GQ, 1)}
    modes = ("plurality", "genotype", "weighted")
    ms = {m: [] for m in modes}
    seen = {}
    for rep in range(REPS + 1):  # (the first round warms; the three alternate inside a round)
        for mode in modes:
            stats = (C.c_uint64 * (5 if mode == "plurality" else 8))()
            size, sums = 0, [0] * len(stats)
            e0.record()
            for a in range(0, n, CHUNK):
                cnt = min(CHUNK, n - a)
                if mode == "plurality":
                    rc = L.slamem_pileup_consensus_device(pile._h, a, cnt, MIN_DEPTH, seq.numel(), _ptr(seq), None, 0, None, stats,
                                                          C.byref(total), stream)
                else:
                    rc = L.slamem_pileup_consensus_gt_device(pile._h, a, cnt, C.byref(params[mode]), seq.numel(), _ptr(seq), None, 0, None,
                                                             stats, C.byref(total), stream)
                capi.check(rc)
                size += int(total.value)
                sums = [x + int(y) for x, y in zip(sums, stats)]
            e1.record()
            e1.synchronize()
            if rep:
                ms[mode].append(float(e0.elapsed_time(e1)))
            seen[mode] = (size, sums)
    out = {"rows": n}
    for mode in modes:
        med = round(float(np.median(ms[mode])), 3)
        out[mode] = {"bytes": seen[mode][0], "stats": seen[mode][1], "ms_median": med,
                     "ms_range": [round(float(np.min(ms[mode])), 3), round(float(np.max(ms[mode])), 3)]}
    for mode in modes[1:]:
        out[mode + "_over_plurality"] = round(out[mode]["ms_median"] / max(out["plurality"]["ms_median"], 1e-9), 3)
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    pile = pile_batch(idx, reads, offsets, M, M * L, 3 * M + 1024)
    del reads, offsets
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20, events and quality sums enabled", **time_modes(idx, pile)}
    pile.close()
    idx.close()
    return out


if __name__ == "__main__":
    res = {"reps": REPS, "min_depth": MIN_DEPTH, "min_gq": MIN_GQ, "headline": headline(int(os.environ.get("READS", 10_000_000)))}
    line = json.dumps(res)
    print(line)
    out = os.environ.get("CONS_GT_RATE_OUT", os.path.join(ROOT, "profiles", "cons_gt_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
