#!/usr/bin/env python3
"""-aln against -mem, -chain and -ext, warmed, on the two shapes of tools/chain_rate.py (-b -l 20, every default): the headline
reads and the 5 Mbp genome pair.  The four modes alternate in one process; per shape and mode the medians of REPS calls of the
call's wall time, search_total_ms and mum_filter_ms (the filter behind K9).  The yardstick of the -aln filter is the sum of the
-chain and -ext filters of the same run (aln_over_chain_plus_ext).  Gaps that take the wave kernel are counted on the host from
the -chain rows and the letters by the kernel's own rule (|a - b| <= 31 and not: a == b <= 64 with at most two differing
letters), on the device; with them
microseconds per wave gap (the whole filter less the -chain filter of the run, which -aln contains, divided by them: an upper
estimate, it holds the pack and the other gap passes too) and wave gaps per block.  Prints one JSON line.  READS / REPS / SHAPES in the environment as for tools/ext_rate.py."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = torch.device("cuda:0")
REPS = int(os.environ.get("REPS", 5))
MODES = (("mem", {}), ("chain", {"chain": True}), ("ext", {"ext": True}), ("aln", None))


class AlnRunner:
    """slamem_find_alns_device with buffers allocated once (what engine.Matcher is for the other modes)."""

    def __init__(self, idx, nq, qbytes, cap, scap, ocap):
        self.idx, self.nq, self.qbytes, self.cap, self.scap, self.ocap = idx, nq, qbytes, cap, scap, ocap
        need = C.c_uint64()
        capi.check(capi.lib().slamem_find_alns_workspace_bytes(nq, 1, qbytes, cap, ocap, engine.EDITS_DEFAULT, C.byref(need)))
        self.ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        self.segs = torch.zeros((scap + 1) * 5, dtype=torch.int32, device=dev)
        self.ops = torch.zeros(ocap + 1, dtype=torch.int32, device=dev)
        self.ooff = torch.zeros(scap + 2, dtype=torch.int64, device=dev)
        self.boff = torch.zeros(2 * nq + 1, dtype=torch.int64, device=dev)
        self.totals = (C.c_uint64 * 3)()

    def run(self, q_dev, off_dev, min_len):
        rc = capi.lib().slamem_find_alns_device(self.idx._h, _ptr(q_dev), _ptr(off_dev), self.nq, self.qbytes, min_len, 1, 0, 0,
                                                engine.XDROP_DEFAULT, engine.EDITS_DEFAULT, self.cap, _ptr(self.segs), self.scap,
                                                _ptr(self.boff), _ptr(self.ops), self.ocap, _ptr(self.ooff), _ptr(self.ws),
                                                self.ws.numel(), None, self.totals)
        if rc != capi.SLAMEM_OK:
            e = capi.SlamemError(rc, capi.lib().slamem_last_error_message().decode(errors="replace"))
            e.totals = tuple(int(t) for t in self.totals)
            raise e
        return int(self.totals[1])


_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b


def wave_gaps(rows, boff, q_dev, off_dev, t_dev, E=31):
    """(gaps, wave gaps, blocks with a gap) by the kernel's own rule, from the -chain rows and the letters, on the device: a gap
    between two consecutive rows of a block goes to the wave kernel iff |a - b| <= E and not (a == b == 0) and not (a == b <= 64
    with at most two differing letters).  rows: (n, 3) int64 tensor; boff: per strand block (two per record); the strand of
    an odd block is the record's reverse complement."""
    n = rows.shape[0]
    nb = boff.shape[0] - 1
    cnt = boff[1:] - boff[:-1]
    blk = torch.repeat_interleave(torch.arange(nb, device=dev), cnt)
    p, q, ln = rows[:, 0], rows[:, 1], rows[:, 2]
    has = torch.zeros(n, dtype=torch.bool, device=dev)
    has[:-1] = blk[:-1] == blk[1:]  # row g has row g + 1 of its block in front of it in the strand
    g = torch.nonzero(has).flatten()
    eqj, epj = q[g + 1] + ln[g + 1], p[g + 1] + ln[g + 1]
    o = torch.clamp(torch.maximum(eqj - q[g], epj - p[g]), min=0)
    a, b = q[g] + o - eqj, p[g] + o - epj
    near = (a - b).abs() <= E
    cand = near & (a == b) & (a <= 64) & (a > 0)
    k = torch.nonzero(cand).flatten()
    rec, rev = blk[g[k]] // 2, (blk[g[k]] % 2) == 1
    start, length = off_dev[rec], off_dev[rec + 1] - off_dev[rec]
    comp = torch.from_numpy(_COMP).to(dev)
    mism = torch.zeros(k.shape[0], dtype=torch.int32, device=dev)
    for t in range(64):
        live = a[k] > t
        x = eqj[k] + t  # in the scanned strand
        at = torch.where(rev, start + length - 1 - x, start + x)
        at = torch.where(live, at, start)
        ql = q_dev[at]
        ql = torch.where(rev, comp[ql.long()], ql)
        tl = t_dev[torch.where(live, epj[k] + t, epj[k])]
        mism += (live & ((ql & 0xDF) != (tl & 0xDF))).int()
    inline = torch.zeros_like(near)
    inline[k] = mism <= 2
    inline |= near & (a == 0) & (b == 0)
    return int(g.shape[0]), int((near & ~inline).sum().item()), int((cnt > 1).sum().item())


def run_modes(idx, q_dev, off_dev, nq, qbytes, cap, t_dev):
    mats = {}
    for name, kw in MODES:
        c = cap
        while True:
            try:
                m = AlnRunner(idx, nq, qbytes, c, c, 2 * c + 4096) if kw is None else engine.Matcher(idx, nq, True, c, qbytes, **kw)
                m.run(q_dev, off_dev, 20)  # warm-up
                break
            except capi.SlamemError as e:
                if e.code != capi.SLAMEM_ERR_CAPACITY:
                    raise
                c = (max(e.totals[0], e.totals[1], e.totals[2] // 2) if kw is None else int(m.last_total)) + 1024
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
                     "ms_median": round(float(np.median(ms[name])), 3), "ms_min": round(float(np.min(ms[name])), 3)}
    base = out["chain"]["filter_ms"] + out["ext"]["filter_ms"]
    ch = mats["chain"]
    rows = ch.mems[:found["chain"]].view(torch.int32).view(-1, 3).long() & 0xFFFFFFFF
    gaps, wave, blocks = wave_gaps(rows, ch.block_offsets.long(), q_dev, off_dev, t_dev)
    chain_only = out["chain"]["filter_ms"]
    a = mats["aln"]
    out.update(segments=found["aln"], operations=int(a.totals[2]), edits=int(a.segs[: 5 * found["aln"]].view(-1, 5)[:, 4].sum().item()),
               chain_plus_ext_filter_ms=round(base, 3), aln_over_chain_plus_ext=round(out["aln"]["filter_ms"] / max(base, 1e-9), 3),
               gaps=gaps, wave_gaps=wave, blocks_with_gaps=blocks, wave_gaps_per_block=round(wave / max(blocks, 1), 3),
               us_per_wave_gap_upper=round(1e3 * max(out["aln"]["filter_ms"] - chain_only, 0.0) / max(wave, 1), 3))
    del mats
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", **run_modes(idx, reads, offsets, M, M * L, 3 * M + 1024, ref)}
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
           **run_modes(idx, qd, od, 1, n, n // 8 + 1024, torch.from_numpy(ref).to(dev))}
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
