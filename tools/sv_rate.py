#!/usr/bin/env python3
"""The cost of the junctions of -sv, warmed, modelled on tools/events_rate.py: slamem_pileup_add_device into an
accumulator with junctions enabled against the same call into one without, alternating in one process; per batch the medians of
REPS calls (HIP events around the add's kernels), then the `junctions` read-out of the whole text.  Two batches over the 100 Mbp
reference of the headline:
  headline  READS x 150 reads with substitutions only: nearly every read is one segment, so this is what the screening costs when
            there is nothing to record
  planted   SV_READS reads of 520 letters, each two stretches of 260 reference letters that lie 200 rows apart (a 200-letter
            deletion with more letters on either side than it is long, as the chain of 4.12 needs): what recording costs, the
            read-out, and how many junctions fall into each skipped counter
The yardstick is the add without junctions OF THE SAME RUN; PARENT_ADD_MS in the environment records the parent commit's plain add
of the same session beside it (tools/events_rate.py of the parent gives it as headline.add_ms).  Prints one JSON line and writes it
to profiles/sv_rate.json.  READS / SV_READS / REPS / SHAPES in the environment."""
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
import events_rate  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = aln_rate.dev
REPS = int(os.environ.get("REPS", 5))


def run_batch(idx, q_dev, off_dev, nq, qbytes, cap):
    m = events_rate.mapped(idx, q_dev, off_dev, nq, qbytes, cap)
    plain, with_sv = engine.Pileup(idx), engine.Pileup(idx, junctions=True)
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
    add(plain), add(with_sv)  # warm-up
    with_sv.reset()
    t_plain, t_sv = [], []
    for rep in range(REPS):
        t_plain.append(add(plain))
        if rep:
            with_sv.reset()  # (every timed add meets an empty table, as a first batch does)
        t_sv.append(add(with_sv))
    n = idx.n
    total, sk = C.c_uint64(), (C.c_uint64 * 4)()
    rc = L.slamem_pileup_junctions_device(with_sv._h, 0, n, 1, 1, 0, None, sk, C.byref(total), stream)  # (the count alone)
    if rc != capi.SLAMEM_ERR_CAPACITY:
        capi.check(rc)
    need = int(total.value)
    buf = torch.empty(max(need, 1) * 24, dtype=torch.uint8, device=dev)
    t_read = []
    for _ in range(REPS):
        e0.record()
        capi.check(L.slamem_pileup_junctions_device(with_sv._h, 0, n, 1, 1, need, _ptr(buf), sk, C.byref(total), stream))
        e1.record()
        e1.synchronize()
        t_read.append(float(e0.elapsed_time(e1)))
    jn = buf[:need * 24].cpu().numpy().view(engine.JUNCTION_DTYPE)
    med = lambda v: round(float(np.median(v)), 3) if len(v) else None  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)] if len(v) else None  # noqa: E731
    want = max(65536, n // 64)
    out = {"reads": nq, "segments": int(m.totals[1]), "reads_of_several_segments": int((torch.diff(m.roff[:nq + 1]) > 1).sum().item()),
           "add_ms": med(t_plain), "add_ms_range": rng(t_plain), "add_with_junctions_ms": med(t_sv), "add_with_junctions_ms_range": rng(t_sv),
           "junctions_over_plain": round(med(t_sv) / max(med(t_plain), 1e-9), 3), "slots": 1 << (want - 1).bit_length(),
           "distinct_junctions": need, "observations": int(jn["fwd"].astype(np.int64).sum() + jn["rev"].astype(np.int64).sum()),
           "deletions_of_200": int(((jn["kind"] == 0) & (jn["len"] == 200)).sum()),
           "skipped": {"balanced": int(sk[0]), "no_room": int(sk[1]), "not_acgt": int(sk[2]), "slop_or_mismatches": int(sk[3])},
           "junctions_readout_ms": med(t_read), "junctions_readout_ms_range": rng(t_read)}
    plain.close()
    with_sv.close()
    del m
    return out


def with_deletions(ref, M, n, seed, flank=260, gap=200):
    """M reads of 2 * flank letters: rows [s, s + flank) and [s + flank + gap, s + 2 flank + gap) of the reference."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    s = torch.randint(0, n - 2 * flank - gap, (M, 1), generator=g, device=dev)
    col = torch.arange(2 * flank, device=dev).unsqueeze(0)
    at = s + col + (col >= flank).long() * gap
    q = torch.cat([ref[at.reshape(-1)], torch.zeros(16, dtype=torch.uint8, device=dev)])
    off = torch.arange(M + 1, dtype=torch.int64, device=dev) * (2 * flank)
    return q, off, M * 2 * flank


if __name__ == "__main__":
    n, L = 100_000_000, 150
    M = int(os.environ.get("READS", 10_000_000))
    MS = int(os.environ.get("SV_READS", 1_000_000))
    shapes = os.environ.get("SHAPES", "headline,planted").split(",")
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    parent = os.environ.get("PARENT_ADD_MS")
    res = {"reps": REPS, "reference": n, "parent_add_ms": float(parent) if parent else None}
    if "headline" in shapes:
        reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
        offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
        res["headline"] = run_batch(idx, reads, offsets, M, M * L, 3 * M + 1024)
        del reads, offsets
    if "planted" in shapes:
        q, off, qbytes = with_deletions(ref, MS, n, 7)
        res["planted"] = run_batch(idx, q, off, MS, qbytes, 4 * MS + 1024)
    idx.close()
    line = json.dumps(res)
    print(line)
    out = os.environ.get("SV_RATE_OUT", os.path.join(ROOT, "profiles", "sv_rate.json"))
    with open(out, "w") as f:
        f.write(line + "\n")
