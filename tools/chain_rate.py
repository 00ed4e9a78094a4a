#!/usr/bin/env python3
"""-chain against -mem and -smem, warmed, on the two shapes of tools/smem_rate.py (-b -l 20): the headline reads (100 Mbp
reference, 10 M reads of 150 letters) and a genome pair (a 5 Mbp reference with planted duplications against one mutated 5 Mbp
copy that carries duplications of its own).  Per shape and mode (-mem, -smem, -chain with the default gap): the call's wall
time (median of REPS calls, the modes alternating), the device times of the calls (medians of search_total_ms and of
mum_filter_ms: the filter behind K9), the rows found, the largest strand block; and a check that the -chain rows are an
in-order subsequence of the -mem rows of their block.  Prints one JSON line.  READS / REPS in the environment change the
sizes."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402

dev = torch.device("cuda:0")
REPS = int(os.environ.get("REPS", 5))
MODES = (("mem", {}), ("smem", {"smem": True}), ("chain", {"chain": True}))


def run_modes(idx, q_dev, off_dev, nq, qbytes, cap):
    ms = {name: [] for name, _ in MODES}
    dev_ms = {name: ([], []) for name, _ in MODES}
    res = {}
    mats = {}
    for name, kw in MODES:
        c = cap
        while True:  # room for the -mem list (every mode needs it)
            m = engine.Matcher(idx, nq, True, c, qbytes, **kw)
            try:
                m.run(q_dev, off_dev, 20)  # warm-up
                break
            except capi.SlamemError as e:
                if e.code != capi.SLAMEM_ERR_CAPACITY:
                    raise
                c = int(m.last_total) + 1024
                del m
        mats[name] = m
    for _ in range(REPS):
        for name, _ in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tot = mats[name].run(q_dev, off_dev, 20)
            ms[name].append((time.perf_counter() - t0) * 1e3)
            t = engine.timings()
            dev_ms[name][0].append(t["search_total_ms"])
            dev_ms[name][1].append(t["mum_filter_ms"])
            res[name] = {"found": int(tot), "search_total_ms": round(float(np.median(dev_ms[name][0])), 3),
                         "filter_ms": round(float(np.median(dev_ms[name][1])), 3)}
    out = {}
    rows = {}
    for name, _ in MODES:
        m = mats[name]
        tot = res[name]["found"]
        r = m.mems[:tot].cpu().numpy().view(np.uint32).reshape(-1, 3)
        b = m.block_offsets.cpu().numpy().view(np.uint64).astype(np.int64)
        rows[name] = (r, b)
        out[name] = dict(res[name], ms_median=round(float(np.median(ms[name])), 3), ms_min=round(float(np.min(ms[name])), 3),
                         largest_block=int(np.diff(b).max()) if len(b) > 1 else 0)
    out["chain_filter_over_smem_filter"] = round(out["chain"]["filter_ms"] / max(out["smem"]["filter_ms"], 1e-6), 3)
    out["chain_in_order_subsequence"] = in_order_subsequence(rows["chain"], rows["mem"])
    del mats
    return out


def in_order_subsequence(sub, full):
    """Every row of `sub` is a row of the same block in `full`, and their order is kept."""
    (r1, b1), (r0, b0) = sub, full
    if len(b1) != len(b0) or np.any(np.diff(b1) > np.diff(b0)):
        return False
    blk0 = np.repeat(np.arange(len(b0) - 1), np.diff(b0))
    blk1 = np.repeat(np.arange(len(b1) - 1), np.diff(b1))
    key0 = np.stack([blk0, r0[:, 0], r0[:, 1], r0[:, 2]], axis=1).astype(np.int64)
    key1 = np.stack([blk1, r1[:, 0], r1[:, 1], r1[:, 2]], axis=1).astype(np.int64)
    order = np.lexsort(key0.T[::-1])
    k0 = key0[order]
    v0 = k0.view([("", np.int64)] * 4).ravel()
    v1 = key1.view([("", np.int64)] * 4).ravel()
    at = np.searchsorted(v0, v1)
    if np.any(at >= len(v0)) or not np.array_equal(v0[np.minimum(at, len(v0) - 1)], v1):
        return False
    pos = order[at]  # place of each row of `sub` in `full`
    same_block = blk1[1:] == blk1[:-1]
    return bool(np.all(pos[1:][same_block] > pos[:-1][same_block]))


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
    for _ in range(40):  # duplications in the reference: 2 kbp elements copied elsewhere
        a, b = (int(x) for x in rng.integers(0, n - 3000, size=2))
        ref[b:b + 2000] = ref[a:a + 2000]
    q = ref.copy()
    mut = rng.random(n) < 0.015
    q[mut] = rng.choice(acgt, size=int(mut.sum()))
    for _ in range(20):  # ... and in the query
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
    res = {"reps": REPS, "genome_pair": genome_pair(), "headline": headline(int(os.environ.get("READS", 10_000_000)))}
    print(json.dumps(res))
