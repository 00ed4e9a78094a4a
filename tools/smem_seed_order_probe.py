#!/usr/bin/env python3
"""K8s time (seed_ms), search_total_ms and the filter time of the headline batch (100 Mbp, 10 M x 150 bp reads, -b -l 20) per
mode and per mode of the call before it: does a -smem call's search cost what a -mem call's does?  Prints one JSON object."""
import collections
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from slamem_amd import engine  # noqa: E402

dev = torch.device("cuda:0")
M, L = 10_000_000, 150
ref = engine.synth_reference(100_000_000, 42, dev)
idx = engine.Index.build(ref, dev)
reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
off = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
mats = {"mem": engine.Matcher(idx, M, True, 3 * M + 1024, M * L),
        "smem": engine.Matcher(idx, M, True, 3 * M + 1024, M * L, smem=True),
        "mem2": engine.Matcher(idx, M, True, 3 * M + 1024, M * L)}
for m in mats.values():
    m.run(reads, off, 20)
seq = ["mem", "smem"] * 8 + ["mem", "mem2"] * 8 + ["smem", "smem"] * 4 + ["mem", "mem"] * 4 + ["mem2", "smem"] * 8
res = collections.defaultdict(list)
prev = None
for name in seq:
    mats[name].run(reads, off, 20)
    t = engine.timings()
    res[f"{name} after {prev}"].append((round(t["seed_ms"], 3), round(t["search_total_ms"], 3), round(t["mum_filter_ms"], 3)))
    prev = name
print(json.dumps({k: {"n": len(v), "seed_med": statistics.median(x[0] for x in v), "total_med": statistics.median(x[1] for x in v),
                      "filter_med": statistics.median(x[2] for x in v)} for k, v in res.items()}, indent=0))
