#!/usr/bin/env python3
"""-paf against -mem, -chain and -aln, warmed, on the two shapes of tools/aln_rate.py (-b -l 20, every default): the headline
reads and the 5 Mbp genome pair.  The four modes alternate in one process; per shape and mode the medians of REPS calls of the
call's wall time, search_total_ms and mum_filter_ms (the filter behind K9).  The yardstick of the -paf filter is the -aln filter
plus the -chain filter of the same run (paf_over_aln_plus_chain; the margin is 1.2 x); paf_over_aln is the ratio to -aln alone.
With them the reads per strand and quality class.  Prints one JSON line and writes it to profiles/map_rate.json.  READS / REPS /
SHAPES in the environment as for tools/aln_rate.py."""
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
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = aln_rate.REPS
MODES = (("mem", {}), ("chain", {"chain": True}), ("aln", "aln"), ("paf", "paf"))


class MapRunner(aln_rate.AlnRunner):
    """slamem_find_maps_device with buffers allocated once."""

    def __init__(self, idx, nq, qbytes, cap, scap, ocap):
        super().__init__(idx, nq, qbytes, cap, scap, ocap)
        need = C.c_uint64()
        capi.check(capi.lib().slamem_find_maps_workspace_bytes(nq, 1, qbytes, cap, ocap, engine.EDITS_DEFAULT, C.byref(need)))
        self.ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        self.roff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        self.reads = torch.zeros((nq + 1) * 3, dtype=torch.int32, device=dev)

    def run(self, q_dev, off_dev, min_len):
        rc = capi.lib().slamem_find_maps_device(self.idx._h, _ptr(q_dev), _ptr(off_dev), self.nq, self.qbytes, min_len, 1, 0, 0,
                                                engine.XDROP_DEFAULT, engine.EDITS_DEFAULT, self.cap, _ptr(self.segs), self.scap,
                                                _ptr(self.roff), _ptr(self.ops), self.ocap, _ptr(self.ooff), _ptr(self.reads),
                                                _ptr(self.ws), self.ws.numel(), None, self.totals)
        if rc != capi.SLAMEM_OK:
            e = capi.SlamemError(rc, capi.lib().slamem_last_error_message().decode(errors="replace"))
            e.totals = tuple(int(t) for t in self.totals)
            raise e
        return int(self.totals[1])


def run_modes(idx, q_dev, off_dev, nq, qbytes, cap):
    mats = {}
    for name, kw in MODES:
        c = cap
        while True:
            try:
                if kw == "aln":
                    m = aln_rate.AlnRunner(idx, nq, qbytes, c, c, 2 * c + 4096)
                elif kw == "paf":
                    m = MapRunner(idx, nq, qbytes, c, c, 2 * c + 4096)
                else:
                    m = engine.Matcher(idx, nq, True, c, qbytes, **kw)
                m.run(q_dev, off_dev, 20)  # warm-up
                break
            except capi.SlamemError as e:
                if e.code != capi.SLAMEM_ERR_CAPACITY:
                    raise
                c = (max(e.totals[0], e.totals[1], e.totals[2] // 2) if isinstance(kw, str) else int(m.last_total)) + 1024
                del m
        mats[name] = m
    ms = {name: [] for name, _ in MODES}
    dev_ms = {name: ([], []) for name, _ in MODES}
    found = {}
    for _ in range(REPS):
        for name, _ in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            found[name] = int(mats[name].run(q_dev, off_dev, 20))
            ms[name].append((time.perf_counter() - t0) * 1e3)
            t = engine.timings()
            dev_ms[name][0].append(t["search_total_ms"])
            dev_ms[name][1].append(t["mum_filter_ms"])
    out = {}
    for name, _ in MODES:
        out[name] = {"found": found[name], "search_total_ms": round(float(np.median(dev_ms[name][0])), 3),
                     "search_total_ms_range": [round(float(np.min(dev_ms[name][0])), 3), round(float(np.max(dev_ms[name][0])), 3)],
                     "filter_ms": round(float(np.median(dev_ms[name][1])), 3),
                     "filter_ms_range": [round(float(np.min(dev_ms[name][1])), 3), round(float(np.max(dev_ms[name][1])), 3)],
                     "ms_median": round(float(np.median(ms[name])), 3), "ms_min": round(float(np.min(ms[name])), 3)}
    base = out["aln"]["filter_ms"] + out["chain"]["filter_ms"]
    p = mats["paf"]
    rec = p.reads[: 3 * nq].view(-1, 3)
    strand, mapq = rec[:, 2] & 0xFF, (rec[:, 2] >> 8) & 0xFF
    out.update(segments=found["paf"], operations=int(p.totals[2]), aln_segments=found["aln"],
               reads_forward=int((strand == 1).sum().item()), reads_reverse=int((strand == 2).sum().item()),
               reads_unmapped=int((strand == 0).sum().item()), reads_mapq60=int((mapq == 60).sum().item()),
               reads_mapq0_mapped=int(((mapq == 0) & (strand != 0)).sum().item()),
               aln_plus_chain_filter_ms=round(base, 3), paf_over_aln_plus_chain=round(out["paf"]["filter_ms"] / max(base, 1e-9), 3),
               paf_over_aln=round(out["paf"]["filter_ms"] / max(out["aln"]["filter_ms"], 1e-9), 3))
    del mats
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
    out = os.environ.get("MAP_RATE_OUT", os.path.join(ROOT, "profiles", "map_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
