#!/usr/bin/env python3
"""-pile against -paf, warmed, on the two shapes of tools/map_rate.py (-b -l 20, every default): the headline reads and the 5 Mbp
genome pair.  The two modes alternate in one process; per shape the medians of REPS calls of
  paf    slamem_find_maps_device: the call's wall time, search_total_ms and mum_filter_ms (the filter behind K9)
  pile   the same call and slamem_pileup_add_device behind it on the same stream: the call pair's wall time, and add_ms, the
         add's own device time (HIP events around its two kernels)
and once per shape the whole-table read-out (slamem_pileup_counts_device into a device buffer, in chunks of 16 M rows).  The
yardstick of the add is the -paf filter OF THE SAME RUN (add_over_paf_filter).  Beside the times the counts that explain the cost,
per contributing read: `=` runs, letters under X, rows under D, I operations, hence the atomics the difference array issues (two
per `=` run, one per X letter, D row and I operation) against the letters a letter-wise kernel would issue one atomic for.
Prints one JSON line and writes it to profiles/pile_rate.json.  READS / REPS / SHAPES in the environment as for
tools/aln_rate.py."""
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
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = aln_rate.REPS
CHUNK = 16 << 20


def op_counts(m, nq):
    """Per contributing read (every mapped read: min_mapq 0): `=` runs, X letters, D rows, I operations, aligned letters."""
    nops = int(m.totals[2])
    ops = m.ops[:nops].to(torch.int64) & 0xFFFFFFFF
    code, length = ops & 15, ops >> 4
    rec = m.reads[: 3 * nq].view(-1, 3)
    mapped = max(1, int(((rec[:, 2] & 0xFF) != 0).sum().item()))
    eq_runs = int((code == 7).sum().item())
    eq_letters = int(length[code == 7].sum().item())
    x_letters = int(length[code == 8].sum().item())
    d_rows = int(length[code == 2].sum().item())
    i_ops = int((code == 1).sum().item())
    atomics = 2 * eq_runs + x_letters + d_rows + i_ops
    return {"reads_mapped": mapped, "eq_runs_per_read": round(eq_runs / mapped, 3), "x_letters_per_read": round(x_letters / mapped, 3),
            "d_rows_per_read": round(d_rows / mapped, 3), "i_ops_per_read": round(i_ops / mapped, 3),
            "atomics_per_read": round(atomics / mapped, 3),
            "letterwise_atomics_per_read": round((eq_letters + x_letters + d_rows + i_ops) / mapped, 3), "atomics": atomics}


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
    pile = engine.Pileup(idx)
    L = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def add():
        e0.record()
        capi.check(L.slamem_pileup_add_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                              _ptr(m.ooff), _ptr(m.reads), 0, stream))
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))
    add()  # warm-up
    paf_ms, paf_total, paf_filter, pile_ms, add_ms = [], [], [], [], []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segments = int(m.run(q_dev, off_dev, 20))
        paf_ms.append((time.perf_counter() - t0) * 1e3)
        t = engine.timings()
        paf_total.append(t["search_total_ms"])
        paf_filter.append(t["mum_filter_ms"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.run(q_dev, off_dev, 20)
        add_ms.append(add())
        pile_ms.append((time.perf_counter() - t0) * 1e3)
    # the whole table, in chunks, into a device buffer
    n = idx.n
    out_dev = torch.zeros((min(CHUNK, n), 6), dtype=torch.int32, device=dev)
    read_ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in range(0, n, CHUNK):
            capi.check(L.slamem_pileup_counts_device(pile._h, a, min(CHUNK, n - a), _ptr(out_dev), stream))
        torch.cuda.synchronize()
        read_ms.append((time.perf_counter() - t0) * 1e3)
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    out = {"segments": segments, "operations": int(m.totals[2]),
           "paf": {"ms_median": med(paf_ms), "ms_min": round(float(np.min(paf_ms)), 3), "search_total_ms": med(paf_total),
                   "filter_ms": med(paf_filter), "filter_ms_range": rng(paf_filter)},
           "pile": {"ms_median": med(pile_ms), "ms_min": round(float(np.min(pile_ms)), 3), "add_ms": med(add_ms), "add_ms_range": rng(add_ms)},
           "add_over_paf_filter": round(med(add_ms) / max(med(paf_filter), 1e-9), 3),
           "readout_rows": n, "readout_ms": med(read_ms), "readout_ms_range": rng(read_ms),
           "readout_gb_per_s": round(n * 48 / 1e6 / max(med(read_ms), 1e-9), 1)}
    counts = op_counts(m, nq)
    out.update(counts)
    out["atomics_per_us"] = round(counts["atomics"] / max(med(add_ms) * 1e3, 1e-9), 1)
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
    out = os.environ.get("PILE_RATE_OUT", os.path.join(ROOT, "profiles", "pile_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
