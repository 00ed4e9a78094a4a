#!/usr/bin/env python3
"""The cost of the indel events of -vcf, warmed, modelled on tools/pile_rate.py: slamem_pileup_add_device into an
accumulator with events enabled against the same call into one without, alternating in one process; per batch the medians of
REPS calls (HIP events around the add's kernels), then the `events` read-out of the whole text and `rows_at` at the events' anchor
rows.  Two batches over the 100 Mbp reference of the headline:
  headline  READS x 150 reads with substitutions only (no I, no D): what the screening costs when there is nothing to record
  indels    INDEL_READS reads of the same generator, each with one deleted or one inserted letter 60 to 89 letters in (the
            construction of tests/test_gpu_chain.indel_reads at scale): what recording costs
The yardstick is the add without events OF THE SAME RUN (DESIGN.md 4.16 recorded 4.79 ms on the headline).  Prints one JSON line
and writes it to profiles/events_rate.json.  READS / INDEL_READS / REPS / SHAPES in the environment."""
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
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = aln_rate.REPS


def mapped(idx, q_dev, off_dev, nq, qbytes, cap):
    c = cap
    while True:
        try:
            m = map_rate.MapRunner(idx, nq, qbytes, c, c, 2 * c + 4096)
            m.run(q_dev, off_dev, 20)
            return m
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            c = max(e.totals[0], e.totals[1], e.totals[2] // 2) + 1024
            del m


def run_batch(idx, q_dev, off_dev, nq, qbytes, cap):
    m = mapped(idx, q_dev, off_dev, nq, qbytes, cap)
    plain, with_ev = engine.Pileup(idx), engine.Pileup(idx, events=True)
    L = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def add(pile):
        e0.record()
        capi.check(L.slamem_pileup_add_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                              _ptr(m.ooff), _ptr(m.reads), 0, stream))
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))
    add(plain), add(with_ev)  # warm-up
    with_ev.reset()
    t_plain, t_ev = [], []
    for rep in range(REPS):
        t_plain.append(add(plain))
        if rep:
            with_ev.reset()  # (every timed add meets an empty table, as a first batch does)
        t_ev.append(add(with_ev))
    n = idx.n
    total, sk = C.c_uint64(), (C.c_uint64 * 3)()
    rc = L.slamem_pileup_events_device(with_ev._h, 0, n, 1, 0, None, sk, C.byref(total), stream)  # (the count alone)
    if rc != capi.SLAMEM_ERR_CAPACITY:
        capi.check(rc)
    need = int(total.value)
    buf = torch.empty(max(need, 1) * 32, dtype=torch.uint8, device=dev)
    t_read, t_rows = [], []
    for _ in range(REPS):
        e0.record()
        capi.check(L.slamem_pileup_events_device(with_ev._h, 0, n, 1, need, _ptr(buf), sk, C.byref(total), stream))
        e1.record()
        e1.synchronize()
        t_read.append(float(e0.elapsed_time(e1)))
    ev = buf[:need * 32].cpu().numpy().view(engine.EVENT_DTYPE)
    pos = torch.from_numpy(np.maximum(ev["pos"].astype(np.int64) - 1, 0)).to(dev)
    rows = torch.zeros((max(need, 1), 6), dtype=torch.int32, device=dev)
    for _ in range(REPS if need else 0):
        e0.record()
        capi.check(L.slamem_pileup_rows_at_device(with_ev._h, _ptr(pos), need, _ptr(rows), stream))
        e1.record()
        e1.synchronize()
        t_rows.append(float(e0.elapsed_time(e1)))
    med = lambda v: round(float(np.median(v)), 3) if len(v) else None  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)] if len(v) else None  # noqa: E731
    ops = m.ops[:int(m.totals[2])].to(torch.int64) & 15
    out = {"reads": nq, "segments": int(m.totals[1]), "operations": int(m.totals[2]),
           "i_ops": int((ops == 1).sum().item()), "d_ops": int((ops == 2).sum().item()),
           "add_ms": med(t_plain), "add_ms_range": rng(t_plain), "add_with_events_ms": med(t_ev), "add_with_events_ms_range": rng(t_ev),
           "events_over_plain": round(med(t_ev) / max(med(t_plain), 1e-9), 3),
           "slots": None, "distinct_events": need, "observations": int(ev["fwd"].astype(np.int64).sum() + ev["rev"].astype(np.int64).sum()),
           "skipped": [int(v) for v in sk], "events_readout_ms": med(t_read), "events_readout_ms_range": rng(t_read),
           "rows_at_ms": med(t_rows), "rows_at_ms_range": rng(t_rows)}
    want = max(65536, n // 16)
    out["slots"] = 1 << (want - 1).bit_length()
    plain.close()
    with_ev.close()
    del m
    return out


def with_indels(reads, M, L, seed):
    """Every even read loses the letter at `at`, every odd read gets a random letter in front of it; at in [60, 90)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    R = reads.view(M, L)
    at = torch.randint(60, 90, (M, 1), generator=g, device=dev)
    half = M // 2
    col = torch.arange(L + 1, device=dev).unsqueeze(0)
    dele = torch.gather(R[:half], 1, (col[:, :L - 1] + (col[:, :L - 1] >= at[:half]).long()))
    ins = torch.gather(R[half:], 1, (col - (col > at[half:]).long()).clamp(max=L - 1))
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (M - half,), generator=g, device=dev)]
    ins.scatter_(1, at[half:], letters.unsqueeze(1))
    q = torch.cat([dele.reshape(-1), ins.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    lens = torch.cat([torch.full((half,), L - 1, dtype=torch.int64, device=dev), torch.full((M - half,), L + 1, dtype=torch.int64, device=dev)])
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    return q, off, int(off[-1].item())


if __name__ == "__main__":
    n, L = 100_000_000, 150
    M = int(os.environ.get("READS", 10_000_000))
    MI = int(os.environ.get("INDEL_READS", 2_000_000))
    shapes = os.environ.get("SHAPES", "headline,indels").split(",")
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    res = {"reps": REPS, "reference": n}
    if "headline" in shapes:
        reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
        offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
        res["headline"] = run_batch(idx, reads, offsets, M, M * L, 3 * M + 1024)
        del reads, offsets
    if "indels" in shapes:
        reads = engine.synth_reads(ref, 0, MI, L, 0.02, 43, 50)
        q, off, qbytes = with_indels(reads, MI, L, 7)
        res["indels"] = run_batch(idx, q, off, MI, qbytes, 4 * MI + 1024)
    idx.close()
    line = json.dumps(res)
    print(line)
    out = os.environ.get("EVENTS_RATE_OUT", os.path.join(ROOT, "profiles", "events_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
