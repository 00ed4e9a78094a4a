#!/usr/bin/env python3
"""The sparse read-out of the pileup (-sites) against what it replaces, warmed, on the two shapes of
tools/pile_rate.py: the headline reads piled on 100 Mbp and the 5 Mbp genome pair.  Per shape, in one process, the medians of REPS
calls (HIP events around the device calls, the wall clock around the host route) of
  sites        slamem_pileup_sites_device over the whole table at the defaults (mode 1, depth 4, 20 percent)
  nonzero      the same in mode 0
  counts       slamem_pileup_counts_device over the whole table into a device buffer, in chunks of 16 M rows
  host_route   slamem_pileup_counts_host of the whole table in chunks of 16 M rows and the spec's rule in numpy on each chunk:
               the only way to the same answer without the new call (one pass, wall clock; its answer is compared with sites')
with the rows selected, the bytes moved per row, the bandwidth that makes, and the ratios sites / counts and host_route / sites.
Prints one JSON line and writes it to profiles/sites_rate.json.  READS / REPS / SHAPES in the environment as for
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
import pile_rate  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = aln_rate.REPS
CHUNK = pile_rate.CHUNK
MIN_DEPTH, MIN_PCT = 4, 20


def variant_rule_numpy(rows, letters, first):
    """The rule of mode 1 at the defaults on a chunk of the table (rows: m x 6 uint32, letters: the text's m letters):
    (positions, masks)."""
    if len(rows) > (1 << 20):  # (numpy's temporaries: a million rows at a time)
        parts = [variant_rule_numpy(rows[a:a + (1 << 20)], letters[a:a + (1 << 20)], first + a) for a in range(0, len(rows), 1 << 20)]
        return np.concatenate([p for p, _ in parts]), np.concatenate([m for _, m in parts])
    c = rows.astype(np.int64)
    d = c[:, :5].sum(axis=1)
    own = np.full(len(c), 4, dtype=np.int64)
    up = letters & 0xDF
    for k, ch in enumerate(b"ACGT"):
        own[up == ch] = k
    ok = (c > 0) & (100 * c >= MIN_PCT * d[:, None])
    ok[np.arange(len(c))[own < 4], own[own < 4]] = False
    mask = (ok * (1 << np.arange(6))).sum(axis=1)
    mask[(own == 4) | (d < MIN_DEPTH)] = 0
    sel = np.nonzero(mask)[0]
    return sel + first, mask[sel].astype(np.uint8)


def time_modes(idx, pile, text_host):
    L = capi.lib()
    n = idx.n
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = C.c_uint64()
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    out = {"rows": n}
    for name, mode in (("sites", engine.SITES_VARIANT), ("nonzero", engine.SITES_NONZERO)):
        rc = L.slamem_pileup_sites_device(pile._h, 0, n, mode, MIN_DEPTH, MIN_PCT, 0, None, None, None, C.byref(total), stream)
        if rc not in (capi.SLAMEM_OK, capi.SLAMEM_ERR_CAPACITY):
            capi.check(rc)
        cap = max(1, int(total.value))
        pos = torch.empty(cap, dtype=torch.int64, device=dev)
        rows = torch.empty((cap, 6), dtype=torch.int32, device=dev)
        alleles = torch.empty(cap, dtype=torch.uint8, device=dev)
        ms = []
        for rep in range(REPS + 1):  # (the first one warms)
            e0.record()
            capi.check(L.slamem_pileup_sites_device(pile._h, 0, n, mode, MIN_DEPTH, MIN_PCT, cap, _ptr(pos), _ptr(rows), _ptr(alleles),
                                                    C.byref(total), stream))
            e1.record()
            e1.synchronize()
            if rep:
                ms.append(float(e0.elapsed_time(e1)))
        m = int(total.value)
        moved = 2 * 28 * n + 33 * m  # the table read twice (4 bytes of diff and 24 of counters a row), 33 bytes written a selected row
        out[name] = {"selected_rows": m, "ms_median": med(ms), "ms_range": rng(ms), "bytes_per_row": round(moved / n, 2),
                     "gb_per_s": round(moved / 1e6 / max(med(ms), 1e-9), 1)}
        if name == "sites":
            sites_pos = pos[:m].cpu().numpy().view(np.uint64)
            sites_mask = alleles[:m].cpu().numpy()
        del pos, rows, alleles
    out_dev = torch.zeros((min(CHUNK, n), 6), dtype=torch.int32, device=dev)
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
    host = np.zeros((min(CHUNK, n), 6), dtype=np.uint32)
    ms, copy_ms = [], []
    for rep in (1,):  # (seconds on the headline: one pass, not warmed -- the host's work dwarfs what warming would change)
        t0 = time.perf_counter()
        tc = 0.0
        got_pos, got_mask = [], []
        for a in range(0, n, CHUNK):
            k = min(CHUNK, n - a)
            t1 = time.perf_counter()
            capi.check(L.slamem_pileup_counts_host(pile._h, a, k, host.ctypes.data))
            tc += time.perf_counter() - t1
            p, m_ = variant_rule_numpy(host[:k], text_host[a:a + k], a)
            got_pos.append(p)
            got_mask.append(m_)
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
            copy_ms.append(tc * 1e3)
    same = bool(np.array_equal(np.concatenate(got_pos).astype(np.uint64), sites_pos) and np.array_equal(np.concatenate(got_mask), sites_mask))
    out["host_route"] = {"ms": med(ms), "counts_host_ms": med(copy_ms), "same_answer": same}
    out["sites_over_counts"] = round(out["sites"]["ms_median"] / max(out["counts"]["ms_median"], 1e-9), 3)
    out["host_route_over_sites"] = round(out["host_route"]["ms"] / max(out["sites"]["ms_median"], 1e-9), 1)
    return out


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
    pile = engine.Pileup(idx)
    capi.check(capi.lib().slamem_pileup_add_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                                   _ptr(m.ooff), _ptr(m.reads), 0, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    del m
    return pile


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    pile = pile_batch(idx, reads, offsets, M, M * L, 3 * M + 1024)
    del reads, offsets
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", **time_modes(idx, pile, ref.cpu().numpy())}
    pile.close()
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
    pile = pile_batch(idx, qd, od, 1, n, n // 8 + 1024)
    out = {"shape": f"{n // 1_000_000} Mbp pair, one mutated query with duplications, -b -l 20", "min_depth_used": 1}
    # (one read: the depth is 1, so the defaults would select nothing; the pair is read at depth 1)
    global MIN_DEPTH
    keep, MIN_DEPTH = MIN_DEPTH, 1
    out.update(time_modes(idx, pile, ref))
    MIN_DEPTH = keep
    pile.close()
    idx.close()
    return out


if __name__ == "__main__":
    shapes = os.environ.get("SHAPES", "genome_pair,headline").split(",")
    res = {"reps": REPS, "min_depth": MIN_DEPTH, "min_pct": MIN_PCT}
    if "genome_pair" in shapes:
        res["genome_pair"] = genome_pair()
    if "headline" in shapes:
        res["headline"] = headline(int(os.environ.get("READS", 10_000_000)))
    line = json.dumps(res)
    print(line)
    out = os.environ.get("SITES_RATE_OUT", os.path.join(ROOT, "profiles", "sites_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
