#!/usr/bin/env python3
"""-ext against -mem, warmed, on the two shapes of tools/chain_rate.py (-b -l 20, default penalty and drop): the headline reads
(100 Mbp reference, 10 M reads of 150 letters) and a genome pair (a 5 Mbp reference with planted duplications against one
mutated 5 Mbp copy that carries duplications of its own).  Per shape and mode: the call's wall time (median of REPS calls, the
modes alternating in one process), the device times (medians of search_total_ms, seed_ms and mum_filter_ms: the filter behind
K9), rows in / rows out, the mean mismatches and the mean length of a row; K8s's line requests of the same batch (seed_windows
+ seed_compares of slamem_search_stats) per millisecond of seed_ms beside the filter's (one request per row and side, and the
64-letter text units its rows walked) per millisecond of mum_filter_ms.  Prints one JSON line.  READS / REPS in the environment
change the sizes, SHAPES (genome_pair,headline) which shapes run."""
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
MODES = (("mem", {}), ("ext", {"ext": True}))


def run_modes(idx, q_dev, off_dev, nq, qbytes, cap):
    ms = {name: [] for name, _ in MODES}
    dev_ms = {name: ([], [], []) for name, _ in MODES}
    found, mats = {}, {}
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
            found[name] = int(mats[name].run(q_dev, off_dev, 20))
            ms[name].append((time.perf_counter() - t0) * 1e3)
            t = engine.timings()
            for k, key in enumerate(("search_total_ms", "seed_ms", "mum_filter_ms")):
                dev_ms[name][k].append(t[key])
    out = {}
    for name, _ in MODES:
        out[name] = {"found": found[name], "search_total_ms": round(float(np.median(dev_ms[name][0])), 3),
                     "seed_ms": round(float(np.median(dev_ms[name][1])), 3),
                     "filter_ms": round(float(np.median(dev_ms[name][2])), 3),
                     "ms_median": round(float(np.median(ms[name])), 3), "ms_min": round(float(np.min(ms[name])), 3)}
    e = mats["ext"]
    tot = found["ext"]
    rows = e.mems[:tot].cpu().numpy().view(np.uint32).reshape(-1, 3)
    mm = e.mismatches[:tot].cpu().numpy().view(np.uint32)
    rows_in = found["mem"]
    # text units the rows walked: every -mem row walks its segment less its seed; the segments of dropped rows are those of
    # the kept ones, so (rows in / rows out) x the kept rows' letters is the estimate
    mem_rows = mats["mem"].mems[:rows_in].cpu().numpy().view(np.uint32).reshape(-1, 3)
    walked_letters = float(rows[:, 2].astype(np.float64).mean() if tot else 0.0) * rows_in - float(mem_rows[:, 2].astype(np.float64).sum())
    units = max(walked_letters, 0.0) / 64.0 + 2.0 * rows_in
    st = engine.search_stats(mats["mem"], q_dev, off_dev, 20)
    k8s_requests = int(st.get("seed_windows", 0)) + int(st.get("seed_compares", 0))
    f_ms, s_ms = out["ext"]["filter_ms"], out["mem"]["seed_ms"]
    out.update(rows_in=rows_in, rows_out=tot, mean_mismatches=round(float(mm.mean()) if tot else 0.0, 4),
               mean_length=round(float(rows[:, 2].mean()) if tot else 0.0, 2),
               largest_block_in=int(np.diff(mats["mem"].block_offsets.cpu().numpy()).max()),
               k8s_line_requests=k8s_requests, k8s_requests_per_ms=round(k8s_requests / max(s_ms, 1e-6), 1),
               filter_line_requests=2 * rows_in, filter_requests_per_ms=round(2 * rows_in / max(f_ms, 1e-6), 1),
               filter_text_units_estimate=int(units), filter_us_per_row=round(1e3 * f_ms / max(rows_in, 1), 4),
               filter_us_per_text_unit=round(1e3 * f_ms / max(units, 1.0), 6))
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
    shapes = os.environ.get("SHAPES", "genome_pair,headline").split(",")
    res = {"reps": REPS}
    if "genome_pair" in shapes:
        res["genome_pair"] = genome_pair()
    if "headline" in shapes:
        res["headline"] = headline(int(os.environ.get("READS", 10_000_000)))
    print(json.dumps(res))
