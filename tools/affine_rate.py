#!/usr/bin/env python3
"""-affine 4,6,2 against unit cost, warmed, on the two shapes of tools/aln_rate.py (-b -l 20, every default):
the headline reads and the 5 Mbp genome pair.  The two costs alternate in one process; per shape and cost the medians of REPS
calls of search_total_ms and mum_filter_ms of slamem_find_alns_device (the -aln filter behind K9; the yardstick of the affine
filter is the unit-cost filter of the same run, affine_over_unit), the gaps that k_aln_geom lists for the wave kernel (counted on
the device from the -chain rows and the letters by the kernel's own rule: |a - b| <= 31 and not a == b <= 64 with at most 2, or
at most 2 (o + e) / x = 4, differing letters), segments, operations, edits, the I and D operations among them, and the indel
events of one Pileup(events=True) add of the same batch mapped at that cost (with the observations that found no room).  -mem's
search_total_ms of the same process goes with them, to be held against the parent commit's.  Prints one JSON line and writes it
to profiles/affine_rate.json.  READS / REPS / SHAPES in the environment as for tools/aln_rate.py."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = torch.device("cuda:0")
REPS = int(os.environ.get("REPS", 5))
COSTS = (("unit", None), ("affine_4_6_2", (4, 6, 2)))

_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b


class Runner:
    """slamem_find_alns_device / slamem_find_maps_device at one max_edits word, buffers allocated once."""

    def __init__(self, idx, nq, qbytes, cap, word, maps):
        self.idx, self.nq, self.qbytes, self.cap, self.word, self.maps = idx, nq, qbytes, cap, word, maps
        self.scap, self.ocap = cap, 2 * cap + 4096
        L = capi.lib()
        need = C.c_uint64()
        capi.check((L.slamem_find_maps_workspace_bytes if maps else L.slamem_find_alns_workspace_bytes)(nq, 1, qbytes, cap, self.ocap, word,
                                                                                                          C.byref(need)))
        self.ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        self.segs = torch.zeros((self.scap + 1) * 5, dtype=torch.int32, device=dev)
        self.ops = torch.zeros(self.ocap + 1, dtype=torch.int32, device=dev)
        self.ooff = torch.zeros(self.scap + 2, dtype=torch.int64, device=dev)
        self.boff = torch.zeros(2 * nq + 1, dtype=torch.int64, device=dev)
        self.reads = torch.zeros((nq + 1) * 12, dtype=torch.uint8, device=dev)
        self.totals = (C.c_uint64 * 3)()

    def run(self, q_dev, off_dev, min_len=20):
        L = capi.lib()
        head = (self.idx._h, _ptr(q_dev), _ptr(off_dev), self.nq, self.qbytes, min_len, 1, 0, 0, engine.XDROP_DEFAULT, self.word, self.cap,
                _ptr(self.segs), self.scap, _ptr(self.boff), _ptr(self.ops), self.ocap, _ptr(self.ooff))
        if self.maps:
            rc = L.slamem_find_maps_device(*head, _ptr(self.reads), _ptr(self.ws), self.ws.numel(), None, self.totals)
        else:
            rc = L.slamem_find_alns_device(*head, _ptr(self.ws), self.ws.numel(), None, self.totals)
        if rc != capi.SLAMEM_OK:
            e = capi.SlamemError(rc, L.slamem_last_error_message().decode(errors="replace"))
            e.totals = tuple(int(t) for t in self.totals)
            raise e
        return int(self.totals[1])


def fitted(make, cap, q_dev, off_dev):
    """A runner whose capacities hold the batch (one warm-up call, grown on SLAMEM_ERR_CAPACITY)."""
    while True:
        m = make(cap)
        try:
            m.run(q_dev, off_dev)
            return m
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            cap = max(e.totals[0], e.totals[1], e.totals[2] // 2) + 1024
            del m


def listed_gaps(rows, boff, q_dev, off_dev, t_dev, inline_d, E=31):
    """(gaps, listed gaps) by k_aln_geom's rule, on the device (tools/aln_rate.py's count with the inline tier as a parameter)."""
    n = rows.shape[0]
    cnt = boff[1:] - boff[:-1]
    blk = torch.repeat_interleave(torch.arange(boff.shape[0] - 1, device=dev), cnt)
    p, q, ln = rows[:, 0], rows[:, 1], rows[:, 2]
    has = torch.zeros(n, dtype=torch.bool, device=dev)
    has[:-1] = blk[:-1] == blk[1:]
    g = torch.nonzero(has).flatten()
    eqj, epj = q[g + 1] + ln[g + 1], p[g + 1] + ln[g + 1]
    o = torch.clamp(torch.maximum(eqj - q[g], epj - p[g]), min=0)
    a, b = q[g] + o - eqj, p[g] + o - epj
    near = (a - b).abs() <= E
    k = torch.nonzero(near & (a == b) & (a <= 64) & (a > 0)).flatten()
    rec, rev = blk[g[k]] // 2, (blk[g[k]] % 2) == 1
    start, length = off_dev[rec], off_dev[rec + 1] - off_dev[rec]
    comp = torch.from_numpy(_COMP).to(dev)
    mism = torch.zeros(k.shape[0], dtype=torch.int32, device=dev)
    for t in range(64):
        live = a[k] > t
        x = eqj[k] + t
        at = torch.where(live, torch.where(rev, start + length - 1 - x, start + x), start)
        ql = q_dev[at]
        ql = torch.where(rev, comp[ql.long()], ql)
        tl = t_dev[torch.where(live, epj[k] + t, epj[k])]
        mism += (live & ((ql & 0xDF) != (tl & 0xDF))).int()
    inline = torch.zeros_like(near)
    inline[k] = mism <= inline_d
    inline |= near & (a == 0) & (b == 0)
    return int(g.shape[0]), int((near & ~inline).sum().item())


def indel_events(idx, m, q_dev, off_dev, nq):
    """The indel events of one add of the mapped batch to an empty Pileup(events=True): (events, observations without room)."""
    pile = engine.Pileup(idx, events=True)
    L = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    capi.check(L.slamem_pileup_add_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.boff), _ptr(m.ops), _ptr(m.ooff),
                                          _ptr(m.reads), 0, stream))
    total, sk = C.c_uint64(), (C.c_uint64 * 3)()
    rc = L.slamem_pileup_events_device(pile._h, 0, idx.n, 1, 0, None, sk, C.byref(total), stream)  # (the count alone)
    if rc != capi.SLAMEM_ERR_CAPACITY:
        capi.check(rc)
    torch.cuda.synchronize()
    pile.close()
    return int(total.value), [int(v) for v in sk]


def run_costs(idx, q_dev, off_dev, nq, qbytes, cap, t_dev):
    words = {name: engine.EDITS_DEFAULT if costs is None else engine.aln_word(31, costs) for name, costs in COSTS}
    alns = {name: fitted(lambda c, w=words[name]: Runner(idx, nq, qbytes, c, w, False), cap, q_dev, off_dev) for name, _ in COSTS}
    mem = engine.Matcher(idx, nq, True, alns["unit"].cap, qbytes)
    mem.run(q_dev, off_dev, 20)
    t = {name: ([], []) for name, _ in COSTS}
    t_mem = []
    for _ in range(REPS):
        mem.run(q_dev, off_dev, 20)
        t_mem.append(engine.timings()["search_total_ms"])
        for name, _ in COSTS:
            alns[name].run(q_dev, off_dev)
            tm = engine.timings()
            t[name][0].append(tm["search_total_ms"])
            t[name][1].append(tm["mum_filter_ms"])
    ch = engine.Matcher(idx, nq, True, alns["unit"].cap, qbytes, chain=True)  # (the -mem rows fit there, so do the chains')
    nchain = int(ch.run(q_dev, off_dev, 20))
    rows = ch.mems[:nchain].view(torch.int32).view(-1, 3).long() & 0xFFFFFFFF
    out = {"mem_search_total_ms": round(float(np.median(t_mem)), 3),
           "mem_search_total_ms_range": [round(float(np.min(t_mem)), 3), round(float(np.max(t_mem)), 3)]}
    for name, costs in COSTS:
        a = alns[name]
        nseg, nops = a.run(q_dev, off_dev), int(a.totals[2])
        codes = a.ops[:nops] & 15
        gaps, listed = listed_gaps(rows, ch.block_offsets.long(), q_dev, off_dev, t_dev, 2 if costs is None else 2 * (costs[1] + costs[2]) // costs[0])
        m = fitted(lambda c, w=words[name]: Runner(idx, nq, qbytes, c, w, True), a.cap, q_dev, off_dev)
        events, no_room = indel_events(idx, m, q_dev, off_dev, nq)
        del m
        out[name] = {"filter_ms": round(float(np.median(t[name][1])), 3),
                     "filter_ms_range": [round(float(np.min(t[name][1])), 3), round(float(np.max(t[name][1])), 3)],
                     "search_total_ms": round(float(np.median(t[name][0])), 3), "gaps": gaps, "listed_gaps": listed, "segments": nseg,
                     "operations": nops, "edits": int(a.segs[: 5 * nseg].view(-1, 5)[:, 4].sum().item()),
                     "indel_operations": int(((codes == 1) | (codes == 2)).sum().item()), "indel_events": events,
                     "indel_observations_without_room": no_room}
    out["affine_over_unit"] = round(out["affine_4_6_2"]["filter_ms"] / max(out["unit"]["filter_ms"], 1e-9), 3)
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", **run_costs(idx, reads, offsets, M, M * L, 3 * M + 1024, ref)}
    idx.close()
    return out


def genome_pair(n=5_000_000, seed=5):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=n)
    for _ in range(40):
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
           **run_costs(idx, qd, od, 1, n, n // 8 + 1024, torch.from_numpy(ref).to(dev))}
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
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "affine_rate.json"), "w") as f:
        f.write(line + "\n")
