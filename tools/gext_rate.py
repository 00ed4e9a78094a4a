#!/usr/bin/env python3
"""-gext 8 beside -affine 4,6,2 alone, warmed, on the two shapes of tools/affine_rate.py (-b -l 20, every
default): the headline reads and the 5 Mbp genome pair.  With and without the band alternate in one process; per shape and band
the medians of REPS calls of search_total_ms and mum_filter_ms of slamem_find_alns_device_gext (the -aln filter behind K9; the
yardstick of the filter with the band is the filter without it of the same run, gext_over_affine -- no target is fixed), the ends
that k_aln_geom listed for k_aln_wave_ends and the ends that kernel replaced (slamem_find_alns_end_counts_device), segments,
operations, edits, the I and D operations among them, and the indel events of one Pileup(events=True) add of the same batch
mapped with that band.  -mem's search_total_ms of the same process goes with them; PARENT=<a built checkout of the parent
commit> runs the same -mem measurement there, in a process of its own, to hold against it.  Prints one JSON line and writes it to
profiles/gext_rate.json.  READS / REPS / SHAPES in the environment as for tools/aln_rate.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.environ.get("GEXT_RATE_ROOT"):  # (the child that measures -mem in another checkout)
    ROOT = os.environ["GEXT_RATE_ROOT"]
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from slamem_amd import capi, engine  # noqa: E402
from slamem_amd.engine import _ptr  # noqa: E402

dev = torch.device("cuda:0")
REPS = int(os.environ.get("REPS", 5))
COSTS = (4, 6, 2)
BANDS = (("affine", 0), ("gext_8", 8))
MEM_ONLY = bool(os.environ.get("GEXT_RATE_ROOT"))


class Runner:
    """slamem_find_alns_device_gext / slamem_find_maps_device_gext at one band, buffers allocated once."""

    def __init__(self, idx, nq, qbytes, cap, band, maps):
        self.idx, self.nq, self.qbytes, self.cap, self.band, self.maps = idx, nq, qbytes, cap, band, maps
        self.word = engine.aln_word(31, COSTS)
        self.scap, self.ocap = cap, 2 * cap + 4096
        L = capi.lib()
        need = C.c_uint64()
        capi.check((L.slamem_find_maps_workspace_bytes_gext if maps else L.slamem_find_alns_workspace_bytes_gext)(
            nq, 1, qbytes, cap, self.ocap, self.word, band, C.byref(need)))
        self.ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        self.segs = torch.zeros((self.scap + 1) * 5, dtype=torch.int32, device=dev)
        self.ops = torch.zeros(self.ocap + 1, dtype=torch.int32, device=dev)
        self.ooff = torch.zeros(self.scap + 2, dtype=torch.int64, device=dev)
        self.boff = torch.zeros(2 * nq + 1, dtype=torch.int64, device=dev)
        self.reads = torch.zeros((nq + 1) * 12, dtype=torch.uint8, device=dev)
        self.totals = (C.c_uint64 * 3)()

    def run(self, q_dev, off_dev, min_len=20):
        L = capi.lib()
        head = (self.idx._h, _ptr(q_dev), _ptr(off_dev), self.nq, self.qbytes, min_len, 1, 0, 0, engine.XDROP_DEFAULT, self.word, self.band,
                self.cap, _ptr(self.segs), self.scap, _ptr(self.boff), _ptr(self.ops), self.ocap, _ptr(self.ooff))
        if self.maps:
            rc = L.slamem_find_maps_device_gext(*head, _ptr(self.reads), _ptr(self.ws), self.ws.numel(), None, self.totals)
        else:
            rc = L.slamem_find_alns_device_gext(*head, _ptr(self.ws), self.ws.numel(), None, self.totals)
        if rc != capi.SLAMEM_OK:
            e = capi.SlamemError(rc, L.slamem_last_error_message().decode(errors="replace"))
            e.totals = tuple(int(t) for t in self.totals)
            raise e
        return int(self.totals[1])

    def end_counts(self):
        """(ends listed, ends replaced) of the last run."""
        out = (C.c_uint64 * 2)()
        capi.check(capi.lib().slamem_find_alns_end_counts_device(self.nq, 1, self.qbytes, self.cap, self.ocap, self.word, self.band,
                                                                 _ptr(self.ws), None, out))
        return int(out[0]), int(out[1])


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


def mem_times(idx, q_dev, off_dev, nq, qbytes, cap):
    mem = engine.Matcher(idx, nq, True, cap, qbytes)
    while True:
        try:
            mem.run(q_dev, off_dev, 20)
            break
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            cap = int(mem.last_total) + 1024
            mem = engine.Matcher(idx, nq, True, cap, qbytes)
    t = []
    for _ in range(REPS):
        mem.run(q_dev, off_dev, 20)
        t.append(engine.timings()["search_total_ms"])
    return {"mem_search_total_ms": round(float(np.median(t)), 3),
            "mem_search_total_ms_range": [round(float(np.min(t)), 3), round(float(np.max(t)), 3)]}


def run_bands(idx, q_dev, off_dev, nq, qbytes, cap):
    out = mem_times(idx, q_dev, off_dev, nq, qbytes, cap)
    if MEM_ONLY:
        return out
    alns = {name: fitted(lambda c, z=band: Runner(idx, nq, qbytes, c, z, False), cap, q_dev, off_dev) for name, band in BANDS}
    t = {name: ([], []) for name, _ in BANDS}
    for _ in range(REPS):
        for name, _ in BANDS:
            alns[name].run(q_dev, off_dev)
            tm = engine.timings()
            t[name][0].append(tm["search_total_ms"])
            t[name][1].append(tm["mum_filter_ms"])
    for name, band in BANDS:
        a = alns[name]
        nseg, nops = a.run(q_dev, off_dev), int(a.totals[2])
        listed, replaced = a.end_counts()
        codes = a.ops[:nops] & 15
        m = fitted(lambda c, z=band: Runner(idx, nq, qbytes, c, z, True), a.cap, q_dev, off_dev)
        events, no_room = indel_events(idx, m, q_dev, off_dev, nq)
        del m
        out[name] = {"filter_ms": round(float(np.median(t[name][1])), 3),
                     "filter_ms_range": [round(float(np.min(t[name][1])), 3), round(float(np.max(t[name][1])), 3)],
                     "search_total_ms": round(float(np.median(t[name][0])), 3), "ends_listed": listed, "ends_replaced": replaced,
                     "segments": nseg, "operations": nops, "edits": int(a.segs[: 5 * nseg].view(-1, 5)[:, 4].sum().item()),
                     "indel_operations": int(((codes == 1) | (codes == 2)).sum().item()), "indel_events": events,
                     "indel_observations_without_room": no_room}
    out["gext_over_affine"] = round(out["gext_8"]["filter_ms"] / max(out["affine"]["filter_ms"], 1e-9), 3)
    return out


def headline(M):
    n, L = 100_000_000, 150
    ref = engine.synth_reference(n, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", **run_bands(idx, reads, offsets, M, M * L, 3 * M + 1024)}
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
    out = {"shape": f"{n // 1_000_000} Mbp pair, one mutated query with duplications, -b -l 20", **run_bands(idx, qd, od, 1, n, n // 8 + 1024)}
    idx.close()
    return out


def measure():
    shapes = os.environ.get("SHAPES", "genome_pair,headline").split(",")
    res = {"reps": REPS}
    if "genome_pair" in shapes:
        res["genome_pair"] = genome_pair()
    if "headline" in shapes:
        res["headline"] = headline(int(os.environ.get("READS", 10_000_000)))
    return res


if __name__ == "__main__":
    res = measure()
    if MEM_ONLY:
        print(json.dumps(res))
        sys.exit(0)
    parent = os.environ.get("PARENT")
    if parent:  # the parent commit's -mem, in a fresh process of that checkout (this file, its package)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GEXT_RATE_ROOT=os.path.abspath(parent)),
                           stdout=subprocess.PIPE, timeout=1200)
        res["parent_mem"] = json.loads(r.stdout.decode().strip().split("\n")[-1]) if r.returncode == 0 else f"failed ({r.returncode})"
    else:
        res["parent_mem"] = "not measured (PARENT=<a built checkout of the parent commit>)"
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gext_rate.json"), "w") as f:
        f.write(line + "\n")
