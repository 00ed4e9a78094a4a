#!/usr/bin/env python3
"""The genotype read-out of the pileup (-gt) against the read-out it stands beside, warmed, on the headline shape
of tools/pile_rate.py: the headline reads piled on 100 Mbp.  In one process, alternating, the medians of REPS calls (HIP events
around the device calls) of
  genotypes    slamem_pileup_genotypes_device over the whole table at the defaults (ploidy 2, error 20, prior 30, depth 4, QUAL 20)
  sites        slamem_pileup_sites_device over the whole table at its defaults (mode 1, depth 4, 20 percent)
with the rows selected, the bytes moved per row and the ratio genotypes / sites.  Both read the table twice; genotypes writes 88
bytes a selected row where sites writes 33.  Prints one JSON line and writes it to profiles/gt_rate.json.  READS / REPS in the
environment as for tools/aln_rate.py."""
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
import sites_rate  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = aln_rate.REPS


def time_both(idx, pile):
    L = capi.lib()
    n = idx.n
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = C.c_uint64()
    params = engine._gt_params(2, 20, 30, 4, 20)

    def gt_call(cap, pos, rows, out):
        return L.slamem_pileup_genotypes_device(pile._h, 0, n, C.byref(params), cap, pos, rows, out, C.byref(total), stream)

    def sites_call(cap, pos, rows, out):
        return L.slamem_pileup_sites_device(pile._h, 0, n, engine.SITES_VARIANT, 4, 20, cap, pos, rows, out, C.byref(total), stream)
    runs = {}
    for name, call, width in (("genotypes", gt_call, engine.GENOTYPE_DTYPE.itemsize), ("sites", sites_call, 1)):
        rc = call(0, None, None, None)  # (the size first)
        if rc not in (capi.SLAMEM_OK, capi.SLAMEM_ERR_CAPACITY):
            capi.check(rc)
        cap = max(1, int(total.value))
        runs[name] = dict(call=call, cap=cap, selected=int(total.value), width=width, ms=[],
                          pos=torch.empty(cap, dtype=torch.int64, device=dev), rows=torch.empty((cap, 6), dtype=torch.int32, device=dev),
                          out=torch.empty(cap * width, dtype=torch.uint8, device=dev))
    for rep in range(REPS + 1):  # (the first round warms; the two alternate)
        for name, r in runs.items():
            e0.record()
            capi.check(r["call"](r["cap"], _ptr(r["pos"]), _ptr(r["rows"]), _ptr(r["out"])))
            e1.record()
            e1.synchronize()
            if rep:
                r["ms"].append(float(e0.elapsed_time(e1)))
    out = {"rows": n}
    for name, r in runs.items():
        med = round(float(np.median(r["ms"])), 3)
        moved = 2 * 28 * n + (32 + r["width"]) * r["selected"]  # the table read twice, pos + counters + the record written a selected row
        out[name] = {"selected_rows": r["selected"], "ms_median": med, "ms_range": [round(min(r["ms"]), 3), round(max(r["ms"]), 3)],
                     "bytes_per_row": round(moved / n, 2), "gb_per_s": round(moved / 1e6 / max(med, 1e-9), 1)}
    out["genotypes_over_sites"] = round(out["genotypes"]["ms_median"] / max(out["sites"]["ms_median"], 1e-9), 3)
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    pile = sites_rate.pile_batch(idx, reads, offsets, M, M * L, 3 * M + 1024)
    del reads, offsets
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", **time_both(idx, pile)}
    pile.close()
    idx.close()
    return out


if __name__ == "__main__":
    res = {"reps": REPS, "headline": headline(int(os.environ.get("READS", 10_000_000)))}
    line = json.dumps(res)
    print(line)
    out = os.environ.get("GT_RATE_OUT", os.path.join(ROOT, "profiles", "gt_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
