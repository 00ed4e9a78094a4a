#!/usr/bin/env python3
"""The cost of the low-quality mask in -pile's add, warmed, modelled on tools/pile_rate.py: the headline batch (100
Mbp, READS x 150 reads at 2 % substitutions, half of them reverse, -b -l 20) is mapped once and then added REPS times in each of
three ways, alternating in one process, HIP events around the add's kernels:
  unmasked      slamem_pileup_add_device (the yardstick: profiles/pile_rate.json, headline.pile.add_ms, of the same session)
  empty_mask    slamem_pileup_add_masked_device with a mask that has no bit set (the masked kernels, the table of `unmasked`)
  illumina_mask the same with about 2 % of the letters low, clustered at the reads' ends as given: the last letters of every
                read, a geometric number of them with mean 3 (the shape of an Illumina run's qualities)
and k_lowq_pack over the batch's quality bytes.  Beside the times, per mapped read, the atomics each way issues -- two per
stretch of an `=` run between excluded letters, one per counted X letter, D row and I operation -- walked on the host over the
first SAMPLE reads.  Prints one JSON line and writes it to profiles/lowq_rate.json (LOWQ_RATE_OUT)."""
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
SAMPLE = 20000


def sample_atomics(m, nq, L, low):
    """Atomics per mapped read of the first `nq` reads (all of length L): low is None or a bool array over their letters."""
    roff = m.roff[: nq + 1].cpu().numpy()
    nseg = int(roff[-1])
    segs = m.segs[: nseg * 5].cpu().numpy().view(np.uint32).reshape(-1, 5)
    ooff = m.ooff[: nseg + 1].cpu().numpy()
    ops = m.ops[: int(ooff[-1])].cpu().numpy().view(np.uint32)
    strand = m.reads[: 3 * nq].cpu().numpy().view(np.uint32).reshape(-1, 3)[:, 2] & 0xFF
    atomics = mapped = 0
    for r in range(nq):
        if strand[r] == 0:
            continue
        mapped += 1
        bits = None if low is None else (low[r * L:(r + 1) * L][::-1] if strand[r] == 2 else low[r * L:(r + 1) * L])
        for s in range(int(roff[r]), int(roff[r + 1])):
            q = int(segs[s, 1])
            for op in ops[int(ooff[s]):int(ooff[s + 1])]:
                code, k = int(op) & 15, int(op) >> 4
                if code == 7:
                    if bits is None:
                        atomics += 2
                    else:
                        b = np.concatenate([[True], bits[q:q + k], [True]])
                        atomics += 2 * int((b[:-1] & ~b[1:]).sum())  # a stretch starts behind every excluded letter
                elif code == 8:
                    atomics += k if bits is None else int((~bits[q:q + k]).sum())
                elif code == 2:
                    atomics += k
                elif code == 1:
                    atomics += 1
                if code in (7, 8, 1):
                    q += k
    return round(atomics / max(1, mapped), 3), mapped


def main():
    M, L = int(os.environ.get("READS", 10_000_000)), 150
    ref = engine.synth_reference(100_000_000, 42, dev)
    idx = engine.Index.build(ref, dev)
    reads = engine.synth_reads(ref, 0, M, L, 0.02, 42, 50)
    offsets = torch.arange(M + 1, dtype=torch.int64, device=dev) * L
    c = 3 * M + 1024
    while True:
        try:
            m = map_rate.MapRunner(idx, M, M * L, c, c, 2 * c + 4096)
            m.run(reads, offsets, 20)
            break
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            c = max(e.totals[0], e.totals[1], e.totals[2] // 2) + 1024
            del m
    # qualities: 40 everywhere, 2 on the last t letters of every read, t geometric with mean 3 (2 % of 150 letters)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    tail = torch.empty(M, device=dev).geometric_(1.0 / 3.0, generator=g).clamp_(max=L).to(torch.int64)
    pos = torch.arange(L, device=dev).unsqueeze(0)
    low = pos >= (L - tail).unsqueeze(1)
    quals = torch.where(low, torch.tensor(33 + 2, dtype=torch.uint8, device=dev), torch.tensor(33 + 40, dtype=torch.uint8, device=dev)).reshape(-1).contiguous()
    words = (M * L + 63) // 64
    mask = torch.zeros(words, dtype=torch.int64, device=dev)
    empty = torch.zeros(words, dtype=torch.int64, device=dev)
    Lb = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        capi.check(fn())
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))
    pack = lambda: Lb.slamem_pack_lowq_device(_ptr(quals), M * L, 20, 33, _ptr(mask), stream)  # noqa: E731
    timed(pack)
    pack_ms = [timed(pack) for _ in range(REPS)]
    low_share = float(low.sum().item()) / (M * L)
    pile = engine.Pileup(idx)
    args = (_ptr(reads), _ptr(offsets), M, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops), _ptr(m.ooff), _ptr(m.reads), 0)
    ways = {"unmasked": lambda: Lb.slamem_pileup_add_device(pile._h, *args, stream),
            "empty_mask": lambda: Lb.slamem_pileup_add_masked_device(pile._h, *args, _ptr(empty), stream),
            "illumina_mask": lambda: Lb.slamem_pileup_add_masked_device(pile._h, *args, _ptr(mask), stream)}
    for fn in ways.values():
        timed(fn)  # warm-up
    ms = {k: [] for k in ways}
    for _ in range(REPS):
        for k, fn in ways.items():
            ms[k].append(timed(fn))
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    ns = min(SAMPLE, M)
    low_host = low[:ns].reshape(-1).cpu().numpy()
    out = {"shape": f"100 Mbp, {M} x {L} reads, -b -l 20", "reps": REPS, "low_letter_share": round(low_share, 5),
           "pack_ms": med(pack_ms), "pack_ms_range": rng(pack_ms), "pack_gb_per_s": round(M * L / 1e6 / max(med(pack_ms), 1e-9), 1),
           "sample_reads": ns}
    for k in ways:
        a, mapped = sample_atomics(m, ns, L, None if k == "unmasked" else (np.zeros_like(low_host) if k == "empty_mask" else low_host))
        out[k] = {"add_ms": med(ms[k]), "add_ms_range": rng(ms[k]), "atomics_per_read": a}
        out["sample_reads_mapped"] = mapped
    out["empty_over_unmasked"] = round(out["empty_mask"]["add_ms"] / max(out["unmasked"]["add_ms"], 1e-9), 3)
    out["illumina_over_unmasked"] = round(out["illumina_mask"]["add_ms"] / max(out["unmasked"]["add_ms"], 1e-9), 3)
    pile.close()
    idx.close()
    line = json.dumps(out)
    print(line)
    with open(os.environ.get("LOWQ_RATE_OUT", os.path.join(ROOT, "profiles", "lowq_rate.json")), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
