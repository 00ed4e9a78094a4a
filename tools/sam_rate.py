#!/usr/bin/env python3
"""The MD pass of -sam against -paf and the pile add, warmed, on the two shapes of tools/pile_rate.py (-b -l 20, every default):
the headline reads and the 5 Mbp genome pair.  The modes alternate in one process; per shape the medians of REPS calls of
  paf    slamem_find_maps_device: search_total_ms and mum_filter_ms (the filter behind K9)
  md     slamem_maps_md_device behind the same call on the same stream: md_ms, its own device time (HIP events around it; the
         call's closing copy of the total is inside)
  add    slamem_pileup_add_device over the same outputs: add_ms, as tools/pile_rate.py times it
The yardstick of the MD pass is the pile add OF THE SAME RUN (md_over_add): the add walks the same operations once per segment and
issues atomics on top.  Beside the times: entries per mapped read, and the segments and operations of the wave path.  Prints one
JSON line and writes it to profiles/sam_rate.json.  READS / REPS / SHAPES in the environment as for tools/aln_rate.py."""
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
REPS = aln_rate.REPS


def run_modes(idx, q_dev, off_dev, nq, qbytes, cap):
    c = cap
    while True:
        try:
            m = map_rate.MapRunner(idx, nq, qbytes, c, c, 2 * c + 4096)
            m.run(q_dev, off_dev, 20)  # warm-up
            break
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            c = max(e.totals[0], e.totals[1], e.totals[2] // 2) + 1024
            del m
    nseg, nops = int(m.totals[1]), int(m.totals[2])
    pile = engine.Pileup(idx)
    L = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    edits = int(m.segs[: nseg * 5].view(-1, 5)[:, 4].to(torch.int64).sum().item()) if nseg else 0
    md_cap = edits + nseg  # the sure bound
    need = C.c_uint64()
    capi.check(L.slamem_maps_md_workspace_bytes(nseg, nq, C.byref(need)))
    ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
    md = torch.zeros(md_cap + 1, dtype=torch.int32, device=dev)
    moff = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    seq = torch.zeros(nseg + 1, dtype=torch.int32, device=dev)
    prim = torch.zeros(nq + 1, dtype=torch.int32, device=dev)
    total = C.c_uint64()

    def md_pass():
        e0.record()
        capi.check(L.slamem_maps_md_device(idx._h, _ptr(m.segs), nseg, _ptr(m.roff), nq, _ptr(m.ops), _ptr(m.ooff), _ptr(md), md_cap,
                                           _ptr(moff), _ptr(seq), _ptr(prim), _ptr(ws), need.value, stream, C.byref(total)))
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    def add():
        e0.record()
        capi.check(L.slamem_pileup_add_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                              _ptr(m.ooff), _ptr(m.reads), 0, stream))
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))
    md_pass()
    add()  # warm-up
    paf_total, paf_filter, md_ms, add_ms = [], [], [], []
    for _ in range(REPS):
        torch.cuda.synchronize()
        m.run(q_dev, off_dev, 20)
        t = engine.timings()
        paf_total.append(t["search_total_ms"])
        paf_filter.append(t["mum_filter_ms"])
        md_ms.append(md_pass())
        add_ms.append(add())
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    per_seg = (m.ooff[1: nseg + 1] - m.ooff[:nseg]) if nseg else torch.zeros(0, dtype=torch.int64, device=dev)
    wave = per_seg > engine.SAM_LANE_OPS
    counts = pile_rate.op_counts(m, nq)
    out = {"segments": nseg, "operations": nops, "md_entries": int(total.value), "md_capacity": md_cap,
           "entries_per_read": round(int(total.value) / counts["reads_mapped"], 3),
           "wave_segments": int(wave.sum().item()), "wave_operations": int(per_seg[wave].sum().item()) if nseg else 0,
           "paf": {"search_total_ms": med(paf_total), "filter_ms": med(paf_filter), "filter_ms_range": rng(paf_filter)},
           "md_ms": med(md_ms), "md_ms_range": rng(md_ms), "add_ms": med(add_ms), "add_ms_range": rng(add_ms),
           "md_over_add": round(med(md_ms) / max(med(add_ms), 1e-9), 3),
           "md_over_paf_filter": round(med(md_ms) / max(med(paf_filter), 1e-9), 3), "reads_mapped": counts["reads_mapped"]}
    pile.close()
    del m
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", **run_modes(idx, reads, offsets, M, M * L, 3 * M + 1024)}
    idx.close()
    return out


def genome_pair(n=5_000_000, seed=5):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=n)
    for _ in range(40):  # (the pair of tools/aln_rate.py)
        a, b = (int(x) for x in rng.integers(0, n - 3000, size=2))
        ref[b:b + 2000] = ref[a:a + 2000]
    q = ref.copy()
    mut = rng.random(n) < 0.015
    q[mut] = rng.choice(acgt, size=int(mut.sum()))
    for _ in range(20):
        a, b = (int(x) for x in rng.integers(0, n - 3000, size=2))
        q[b:b + 1000] = q[a:a + 1000]
    idx = engine.Index.build(torch.from_numpy(ref).to(dev), dev)
    qd = torch.zeros((n + 15) // 8 * 8, dtype=torch.uint8, device=dev)
    qd[:n] = torch.from_numpy(q).to(dev)
    od = torch.tensor([0, n], dtype=torch.int64, device=dev)
    out = {"shape": f"{n // 1_000_000} Mbp pair, one mutated query with duplications, -b -l 20",
           **run_modes(idx, qd, od, 1, n, n // 8 + 1024)}
    idx.close()
    return out


if __name__ == "__main__":
    shapes = os.environ.get("SHAPES", "genome_pair,headline").split(",")
    res = {"reps": REPS}
    if "genome_pair" in shapes:
        res["genome_pair"] = genome_pair()
    if "headline" in shapes:
        res["headline"] = headline(int(os.environ.get("READS", 10_000_000)))
    line = json.dumps(res)
    print(line)
    out = os.environ.get("SAM_RATE_OUT", os.path.join(ROOT, "profiles", "sam_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
