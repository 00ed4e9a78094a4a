"""bench.py on a small batch: a plain run prints the headline line and nothing it needs extra work for; --dump-outputs writes
what the last timed step computed (the same files on a second run, the oracle's MEMs); --full keeps the other measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, L, SEED = 2_000_000, 50_000, 150, 42
SMALL = ["--gpus", "1", "--ref-len", str(N), "--reads", str(M), "--read-len", str(L), "--seed", str(SEED), "--steps", "3",
         "--warmup", "1"]
DUMPED = ["sample_block_mems.npy", "sample_blocks.npy", "sample_mems.npy", "totals.npy"]


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_step_computed(tmp_path):
    import torch
    from slamem_amd import engine
    from oracle import pyoracle as po
    a = run_bench("--dump-outputs", str(tmp_path / "a"))
    b = run_bench("--dump-outputs", str(tmp_path / "b"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0
    for k in ("roofline", "cpu_baseline", "sample_parity_vs_oracle", "value_host_to_host"):
        assert k not in a, k
    assert sorted(os.listdir(tmp_path / "a")) == DUMPED
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in DUMPED) <= 64_000_000
    got = {}
    for f in DUMPED:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.array_equal(x, y), f
        got[f[:-4]] = x
    # 100 k blocks: the sample is the whole output; it must be the oracle's answer on the same generated reads
    ref = engine.synth_reference(N, SEED, "cuda:0")
    reads = engine.synth_reads(ref, 0, M, L, 0.02, SEED, 50)[: M * L].cpu().numpy()
    torch.cuda.synchronize()
    om, obc = po.OracleIndex(ref.cpu().numpy().tobytes()).match_batch(reads, np.arange(M + 1, dtype=np.uint64) * np.uint64(L),
                                                                       20, True)
    assert np.array_equal(got["sample_blocks"], np.arange(2 * M))
    assert np.array_equal(got["sample_block_mems"], obc.astype(np.float64))
    assert np.array_equal(got["sample_mems"], np.stack([om["ref_pos"], om["query_pos"], om["length"]], 1).astype(np.float64))
    assert np.array_equal(got["totals"], np.array([len(om), om["ref_pos"].sum(dtype=np.uint64), om["query_pos"].sum(dtype=np.uint64),
                                                   om["length"].sum(dtype=np.uint64)], dtype=np.float64))
    assert a["mems_per_step"] == len(om)


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements():
    d = run_bench("--full", "--cpu-sample-reads", "5000", "--long-stream-reads", "0")
    assert d["roofline"]["kernel"] in ("k_seed_mems", "k_find_mems_v3") and d["roofline"]["traffic"] > 0
    assert d["sample_parity_vs_oracle"] is True
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline_all_cores"]["value"] > 0
    assert d["value_host_to_host"] > 0 and d["host_to_host_packed"]["value"] > 0
