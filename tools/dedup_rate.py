#!/usr/bin/env python3
"""-dedup against the plain add, warmed, on the two shapes of tools/pile_rate.py (-b -l 20, every default): the headline reads and
the 5 Mbp genome pair.  One mapping per shape (slamem_find_maps_device, as tools/map_rate.py runs it); then, alternating in one
process, the medians of REPS calls, each timed with HIP events on the stream the kernels run on:
  add        slamem_pileup_add_device over the batch: the yardstick, the add without the filter in the same run (and, as a
             cross-check that it did not move, against add_ms of profiles/pile_rate.json)
  dedup_add  slamem_pileup_add_dedup_device over the batch on a freshly reset accumulator: k_dup_claim, k_dup_mark and the pile
             kernels behind them
  pile_kept  slamem_pileup_add_device over the records dedup_add left in reads_keep: the pile kernels behind the pair, alone
  pair       dedup_add - pile_kept of the same repetition: k_dup_claim and k_dup_mark (the C interface enqueues the pair and the
             pile kernels in one call, so the pair's events cannot be placed from outside; the difference of two event timings of
             the same repetition stands in for them)
Beside the times the filter's counters (candidates, duplicates, no room) and the table's slots.  Prints one JSON line and writes
it to profiles/dedup_rate.json.  READS / REPS / SHAPES in the environment as for tools/aln_rate.py."""
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
REPS = aln_rate.REPS


def run_modes(idx, q_dev, off_dev, nq, qbytes, cap):
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
    plain, pile = engine.Pileup(idx), engine.Pileup(idx, dedup=True)
    keep = torch.zeros((nq + 1) * 3, dtype=torch.int32, device=dev)
    dup = torch.zeros(nq + 1, dtype=torch.uint8, device=dev)
    L = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        e0.record()
        capi.check(call())
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))
    batch = (_ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops), _ptr(m.ooff))
    add = lambda acc, recs: timed(lambda: L.slamem_pileup_add_device(acc._h, *batch, _ptr(recs), 0, stream))  # noqa: E731
    dedup = lambda: timed(lambda: L.slamem_pileup_add_dedup_device(pile._h, *batch, _ptr(m.reads), 0, None, _ptr(keep), _ptr(dup), stream))  # noqa: E731
    add(plain, m.reads)  # warm-up
    dedup()
    add(pile, keep)
    stats = None
    add_ms, dedup_ms, kept_ms, pair_ms = [], [], [], []
    for _ in range(REPS):
        add_ms.append(add(plain, m.reads))
        pile.reset()  # (a second dedup add of the same batch would find every read a duplicate)
        d = dedup()
        if stats is None:
            stats = pile.dedup_stats()
        k = add(pile, keep)
        dedup_ms.append(d)
        kept_ms.append(k)
        pair_ms.append(d - k)
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    out = {"reads": nq, "segments": int(m.totals[1]), **stats,
           "duplicate_share": round(stats["duplicates"] / max(stats["candidates"], 1), 5),
           "add_ms": med(add_ms), "add_ms_range": rng(add_ms), "dedup_add_ms": med(dedup_ms), "dedup_add_ms_range": rng(dedup_ms),
           "pile_kept_ms": med(kept_ms), "pile_kept_ms_range": rng(kept_ms), "pair_ms": med(pair_ms), "pair_ms_range": rng(pair_ms),
           "dedup_over_add": round(med(dedup_ms) / max(med(add_ms), 1e-9), 3),
           "pair_ns_per_read": round(med(pair_ms) * 1e6 / max(nq, 1), 2)}
    plain.close()
    pile.close()
    del m
    return out


def headline(M):
    n, Lr = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, Lr, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * Lr
    out = {"shape": f"100 Mbp, {M} x {Lr} reads, -b -l 20", **run_modes(idx, reads, offsets, M, M * Lr, 3 * M + 1024)}
    idx.close()
    return out


def genome_pair(n=5_000_000, seed=5):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=n)
    for _ in range(40):  # (the pair of tools/aln_rate.py and tools/pile_rate.py)
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
    parent = os.path.join(ROOT, "profiles", "pile_rate.json")
    if os.path.exists(parent):  # the add of the run that measured -pile, for the cross-check
        with open(parent) as f:
            was = json.loads(f.readline())
        res["pile_rate_add_ms"] = {k: was[k]["pile"]["add_ms"] for k in ("genome_pair", "headline") if k in was}
    line = json.dumps(res)
    print(line)
    out = os.environ.get("DEDUP_RATE_OUT", os.path.join(ROOT, "profiles", "dedup_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
