#!/usr/bin/env python3
"""-stats against -paf and the pile add, warmed, on the two shapes of tools/pile_rate.py (-b -l 20, every default): the headline
reads and the 5 Mbp genome pair.  The calls alternate in one process; per shape the medians of REPS calls of
  paf        slamem_find_maps_device: the call's wall time and mum_filter_ms (the filter behind K9)
  pile add   slamem_pileup_add_device behind the same call on the same stream: its own device time (HIP events)
  stats add  slamem_stats_add_device behind the same call, without and with quality bytes (a sequencer's four values in runs of
             ten letters): its own device time
The yardsticks of the stats add are the pile add and the -paf filter OF THE SAME RUN (stats_over_pile_add, stats_over_paf_filter).
Prints one JSON line and writes it to profiles/stats_rate.json ($STATS_RATE_OUT).  A file that is there already keeps its other
keys: `unattached` holds the tools/pile_rate.py numbers of this commit and of its parent (the cost to callers that attach no
table), written by whoever ran both.  READS / REPS / SHAPES in the environment as for tools/aln_rate.py."""
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


def run_modes(idx, q_dev, off_dev, nq, qbytes, cap):
    c = cap
    while True:
        try:
            m = map_rate.MapRunner(idx, nq, qbytes, c, c, 2 * c + 4096)
            m.run(q_dev, off_dev, 20)  # warm-up
            break
        except capi.SlamemError as e:
            if e.code != capi.SLAMEM_ERR_CAPACITY:
                raise
            c = max(e.totals[0], e.totals[1], e.totals[2] // 2) + 1024
            del m
    pile, stats = engine.Pileup(idx), engine.MapStats(idx)
    L = capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    values = torch.tensor([2, 12, 25, 37], dtype=torch.uint8, device=dev) + 33
    quals = values[torch.randint(0, 4, ((qbytes + 9) // 10,), device=dev)].repeat_interleave(10)[:qbytes].contiguous()
    quals = torch.cat([quals, torch.zeros(16, dtype=torch.uint8, device=dev)])

    def timed(call):
        e0.record()
        capi.check(call())
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    def pile_add():
        return L.slamem_pileup_add_device(pile._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops), _ptr(m.ooff),
                                          _ptr(m.reads), 0, stream)

    def stats_add(qb):
        return lambda: L.slamem_stats_add_device(stats._h, _ptr(q_dev), _ptr(off_dev), nq, _ptr(m.segs), _ptr(m.roff), _ptr(m.ops),
                                                 _ptr(m.ooff), _ptr(m.reads), _ptr(qb) if qb is not None else None, 33, 0, stream)
    for call in (pile_add, stats_add(None), stats_add(quals)):  # warm-up
        timed(call)
    paf_ms, paf_filter, t_pile, t_plain, t_quals = [], [], [], [], []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segments = int(m.run(q_dev, off_dev, 20))
        paf_ms.append((time.perf_counter() - t0) * 1e3)
        paf_filter.append(engine.timings()["mum_filter_ms"])
        t_pile.append(timed(pile_add))
        t_plain.append(timed(stats_add(None)))
        t_quals.append(timed(stats_add(quals)))
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    rng = lambda v: [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]  # noqa: E731
    tab = stats.table()
    out = {"segments": segments, "operations": int(m.totals[2]), "reads_mapped": int(tab["totals"][1]),
           "letters_aligned": int(tab["totals"][9] + tab["totals"][10]),
           "paf": {"ms_median": med(paf_ms), "filter_ms": med(paf_filter), "filter_ms_range": rng(paf_filter)},
           "pile_add_ms": med(t_pile), "pile_add_ms_range": rng(t_pile),
           "stats_add_ms": med(t_plain), "stats_add_ms_range": rng(t_plain),
           "stats_add_quals_ms": med(t_quals), "stats_add_quals_ms_range": rng(t_quals),
           "stats_over_pile_add": round(med(t_plain) / max(med(t_pile), 1e-9), 3),
           "stats_quals_over_pile_add": round(med(t_quals) / max(med(t_pile), 1e-9), 3),
           "stats_over_paf_filter": round(med(t_plain) / max(med(paf_filter), 1e-9), 3)}
    pile.close()
    stats.close()
    del m
    return out


if __name__ == "__main__":
    pile_rate.run_modes = run_modes  # (the shapes of tools/pile_rate.py, with this file's calls)
    shapes = os.environ.get("SHAPES", "genome_pair,headline").split(",")
    res = {"reps": REPS}
    if "genome_pair" in shapes:
        res["genome_pair"] = pile_rate.genome_pair()
    if "headline" in shapes:
        res["headline"] = pile_rate.headline(int(os.environ.get("READS", 10_000_000)))
    out = os.environ.get("STATS_RATE_OUT", os.path.join(ROOT, "profiles", "stats_rate.json"))
    if os.path.exists(out):
        try:
            with open(out) as f:
                res = {**json.load(f), **res}
        except ValueError:
            pass
    line = json.dumps(res)
    print(line)
    with open(out, "w") as f:
        f.write(line + "\n")
