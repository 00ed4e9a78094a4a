"""-chain on the MI355X (slamem_find_chains_device, Index.find_chains, Stream(chain=True), slaMEM-hip -chain [-mgap N]): every
result is the chain filter of the complete -mem list of the same engine (tests/chain_spec.py) -- on the golden files the real
reference wrote, on reads with planted indels and a distant repeat copy, on blocks of every tier of the filter (a lane, a
wave, more rows than the wave's LDS tile, a sliced long record), through the stream, at the capacity edge and on the N-GPU
schedule of the command line."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import chain_spec
import hostlib
import mum_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, ecoli_like_pair, opt_value

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
COMP = np.frombuffer(bytes.maketrans(b"ACGTN", b"TGCAN"), dtype=np.uint8)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def triples(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


def assert_is_chain_of(chain, chain_boff, scores, mem, mem_boff, gap=chain_spec.DEFAULT_GAP, windowed=False):
    kept, kept_boff, want = chain_spec.filter_blocks(mem, mem_boff, gap, windowed)
    assert np.array_equal(np.asarray(chain_boff, dtype=np.int64), kept_boff)
    assert np.array_equal(triples(chain), kept)
    if scores is not None:
        assert np.array_equal(np.asarray(scores, dtype=np.int64), want)


def revcomp(s: np.ndarray) -> np.ndarray:
    return COMP[s[::-1]]


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_engine(eng, case, path):
    idx = None
    for gap in (0, 50):
        _, kept, want, ref, qs, opts = chain_spec.golden_chain_file(case, gap or chain_spec.DEFAULT_GAP)
        if idx is None:
            idx = eng.Index.build(np.frombuffer(ref.chars, dtype=np.uint8).copy())
        off = np.array(qs.offsets, dtype=np.uint64)
        with search_path(path):
            mems, boff, scores = idx.find_chains(np.frombuffer(qs.chars, dtype=np.uint8), off, int(opt_value(opts, "-l", 20)),
                                                 "-b" in opts, max_gap=gap)
        assert len(boff) == len(kept) + 1 and len(scores) == len(kept)
        for b, rows in enumerate(kept):
            assert np.array_equal(triples(mems[int(boff[b]):int(boff[b + 1])]), rows.astype(np.int64)), (case, gap, b)
        assert np.array_equal(scores.astype(np.int64), np.array(want, dtype=np.int64)), (case, gap)
        assert eng.timings()["mum_filter_ms"] > 0
    idx.close()


@pytest.mark.parametrize("gap", [0, 50])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_cli(case, gap, tmp_path):
    expected, _, _, _, _, _ = chain_spec.golden_chain_file(case, gap or chain_spec.DEFAULT_GAP)
    ref_fa, q_fa, _, _ = case_paths(case)
    out = tmp_path / "out.txt"
    extra = ["-mgap", str(gap)] if gap else []
    # -chain takes no value, so it may stand anywhere; the value of -mgap is never taken for a file
    r = subprocess.run([EXE] + MANIFEST[case]["opts"] + extra + ["-o", str(out), ref_fa, "-chain", q_fa], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    assert out.read_bytes() == expected
    assert b"minimum chained MEM length" in r.stdout and b"Saving chained MEMs" in r.stdout
    assert (b"; maximum gap = %d\n" % (gap or 5000)) in r.stdout


def indel_reads(seed):
    """A reference with one 60-letter element repeated 3,000 letters further on; reads of 200 letters across the first copy,
    each with a deleted or an inserted letter and a few substitutions: their matches lie on two diagonals one apart, and the
    element matches its distant copy as well -- inside the gap for G >= 3000, outside for a small G."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=40000)
    for a in range(2000, 30000, 4000):
        ref[a + 3000:a + 3060] = ref[a:a + 60]
    reads = []
    for k in range(160):
        a = 2000 + 4000 * (k % 7) - int(rng.integers(20, 120))
        r = ref[a:a + 200].copy()
        at = int(rng.integers(60, 140))
        r = np.delete(r, at) if k % 2 else np.insert(r, at, rng.choice(acgt))
        mut = rng.random(len(r)) < 0.02
        r[mut] = rng.choice(acgt, size=int(mut.sum()))
        reads.append(revcomp(r) if k % 3 == 0 else r)
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return ref, q, off


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
def test_planted_indels_and_distant_copy(eng, path, both):
    ref, q, off = indel_reads(3)
    idx = eng.Index.build(ref)
    sk = int(idx.info.seed_k) or 12
    linked = dropped = differ = 0
    for min_len in (sk + 1, sk + 6):
        with search_path(path):
            mem, mem_boff = idx.find_mems(q, off, min_len, both)
            res = {gap: idx.find_chains(q, off, min_len, both, max_gap=gap) for gap in (0, 100, 3500)}
        for gap, (ch, ch_boff, scores) in res.items():
            assert_is_chain_of(ch, ch_boff, scores, mem, mem_boff, gap or chain_spec.DEFAULT_GAP)
            linked += int((np.diff(ch_boff.astype(np.int64)) > 1).sum())
            dropped += len(mem) - len(ch)
        differ += not np.array_equal(res[100][2], res[3500][2])
    assert linked > 0 and dropped > 0 and differ > 0
    idx.close()


def tier_batch():
    """The sliced strain of the E. coli-like genome pair cut down to its first 400 kbp (a block of thousands of rows: more
    than the wave's LDS tile), a 6,000-letter record (a block of some tens of rows: a wave), short reads (a lane each) and an
    empty-handed read, in one batch."""
    ref, strain = ecoli_like_pair(duplicates=True)
    ref, strain = ref[:400_000].copy(), strain[:400_000].copy()
    rng = np.random.default_rng(12)
    reads = [ref[int(a):int(a) + 150].copy() for a in rng.integers(0, len(ref) - 150, size=40)]
    reads.insert(10, strain)
    reads.insert(25, strain[100_000:106_000].copy())
    reads.append(np.frombuffer(b"N" * 80, dtype=np.uint8).copy())
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return ref, q, off


def test_every_tier_and_a_sliced_record(eng, capsys):
    ref, q, off = tier_batch()
    idx = eng.Index.build(ref)
    checked = 0.0
    for both in (False, True):
        mem, mem_boff = idx.find_mems(q, off, 20, both)
        sizes = np.diff(mem_boff.astype(np.int64))
        assert sizes.max() > 1024 and np.any((sizes > 32) & (sizes <= 1024)) and np.any((sizes > 0) & (sizes <= 32)) and np.any(sizes == 0)
        for gap in (0, 300, 200_000):
            ch, ch_boff, scores = idx.find_chains(q, off, 20, both, max_gap=gap)
            ms = eng.timings()["mum_filter_ms"]
            t0 = time.perf_counter()
            assert_is_chain_of(ch, ch_boff, scores, mem, mem_boff, gap or chain_spec.DEFAULT_GAP, windowed=True)
            checked += time.perf_counter() - t0
            assert 0 < len(ch) < len(mem)
            assert ms > 0
    with capsys.disabled():
        print(f"\n[chain tiers] largest block {int(sizes.max())} rows; the Python checker took {checked:.1f} s for 6 results")
    idx.close()


def test_stream_equals_one_shot(eng):
    from slamem_amd import capi
    ref, q, off = indel_reads(7)
    idx = eng.Index.build(ref)
    for gap in (0, 100):
        one, one_boff, _ = idx.find_chains(q, off, 14, True, max_gap=gap)
        per = 13
        nq = len(off) - 1
        wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
        st = eng.Stream(idx, 3, 1 << 16, per, True, chain=True, max_gap=gap)
        got, got_counts = [], []
        st.submit(q, wins[0], 14)
        st.submit(q, wins[1], 14)
        for b in range(len(wins)):
            m, boff, tm = st.next()
            if b + 2 < len(wins):
                st.submit(q, wins[b + 2], 14)  # every slot in use
            got.append(triples(m))
            got_counts.append(np.diff(boff.astype(np.int64)))
        st.close()
        assert np.array_equal(np.concatenate(got), triples(one))
        assert np.array_equal(np.concatenate(got_counts), np.diff(one_boff.astype(np.int64)))
    for bad in (dict(mam=True, chain=True), dict(mum=True, chain=True), dict(smem=True, chain=True), dict(max_gap=20),
                dict(smem=True, max_gap=20), dict(chain=True, max_occ=2), dict(chain=True, max_gap=2 ** 31),
                dict(chain=True, max_gap=-1)):
        with pytest.raises(ValueError):
            eng.Stream(idx, 3, 1 << 16, 13, True, **bad)
        with pytest.raises(ValueError):
            idx.find_mems(q, off, 14, True, **bad)
    # set_max_gap: refused on a stream of another match type, and after the first submit
    L = capi.lib()
    st = eng.Stream(idx, 3, 1 << 16, 13, True, smem=True)
    assert L.slamem_stream_set_max_gap(st._h, 20) == capi.SLAMEM_ERR_ARG
    assert L.slamem_stream_set_max_gap(st._h, 0) == capi.SLAMEM_OK
    st.close()
    st = eng.Stream(idx, 3, 1 << 16, 13, True, chain=True)
    assert L.slamem_stream_set_max_gap(st._h, 2 ** 31) == capi.SLAMEM_ERR_ARG
    assert L.slamem_stream_set_max_gap(st._h, 20) == capi.SLAMEM_OK
    st.submit(q, off[:14].copy(), 14)
    assert L.slamem_stream_set_max_gap(st._h, 30) == capi.SLAMEM_ERR_ARG
    st.next()
    st.close()
    idx.close()


def test_capacity_between_chain_and_mem_counts(eng):
    import torch
    from slamem_amd import capi
    ref, q, off = indel_reads(11)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    ch, ch_boff, scores = idx.find_chains(q, off, 14, True)
    assert len(ch) < len(mem)
    qd = torch.zeros((len(q) + 15) // 8 * 8, dtype=torch.uint8, device=idx.device)
    qd[: len(q)] = torch.from_numpy(q).to(idx.device)
    od = torch.from_numpy(off.view(np.int64)).to(idx.device)
    m = idx.matcher(len(off) - 1, True, (len(ch) + len(mem)) // 2, int(off[-1]), chain=True)
    with pytest.raises(capi.SlamemError) as e:
        m.run(qd, od, 14)
    assert e.value.code == capi.SLAMEM_ERR_CAPACITY
    assert m.last_total == len(mem)
    m2 = idx.matcher(len(off) - 1, True, m.last_total, int(off[-1]), chain=True)
    total = m2.run(qd, od, 14)
    assert total == len(ch)
    got = m2.mems[:total].cpu().numpy().view(np.uint32).reshape(-1, 3).astype(np.int64)
    assert np.array_equal(got, triples(ch))
    assert np.array_equal(m2.block_offsets.cpu().numpy(), ch_boff.astype(np.int64))
    assert np.array_equal(m2.scores.cpu().numpy().view(np.uint32), scores)
    idx.close()


def test_other_modes_unchanged_by_chain_calls(eng):
    ref, q, off = indel_reads(13)
    idx = eng.Index.build(ref)
    modes = (dict(), dict(mam=True), dict(mum=True), dict(smem=True))
    before = [idx.find_mems(q, off, 14, True, **kw) for kw in modes]
    for gap in (0, 10, 4000):
        idx.find_mems(q, off, 14, True, chain=True, max_gap=gap)
        assert eng.timings()["mum_filter_ms"] > 0
        mid = idx.find_mems(q, off, 14, True)
        assert eng.timings()["mum_filter_ms"] == 0
        assert np.array_equal(triples(mid[0]), triples(before[0][0]))
    after = [idx.find_mems(q, off, 14, True, **kw) for kw in modes]
    for (m0, b0), (m1, b1) in zip(before, after):
        assert np.array_equal(b0, b1)
        assert np.array_equal(triples(m0), triples(m1))
    idx.close()


def test_cli_logical_gpus_byte_identical(tmp_path):
    """The N-GPU schedule of the command line (SLAMEM_LOGICAL_GPUS=2: two streams on the one device, batches alternate)
    passes the mode and the gap to every stream: the file equals the one-GPU file, and the -mem file filtered by the spec."""
    d = str(tmp_path)
    gen = os.path.join(ROOT, "tools", "gen_synth.py")
    g = subprocess.run([sys.executable, gen, "2000000", "20000", "150", "0.02", "7", "50", d], stdout=subprocess.PIPE)
    assert g.returncode == 0
    ref_fa, q_fa = os.path.join(d, "ref.fa"), os.path.join(d, "qry.fa")
    base = dict(os.environ, SLAMEM_BATCH_MB="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for name, args, env in (("mem", [], base), ("one", ["-chain", "-mgap", "40"], base),
                            ("two", ["-chain", "-mgap", "40"], dict(base, SLAMEM_LOGICAL_GPUS="2"))):
        out = os.path.join(d, f"{name}.txt")
        r = subprocess.run([EXE, "-b", "-l", "14"] + args + ["-o", out, ref_fa, q_fa], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, env=env, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        if name == "two":
            assert b"replicated to 2 logical GPUs by RCCL broadcast ... OK" in r.stdout
        outs[name] = open(out, "rb").read()
    assert outs["two"] == outs["one"]
    ref = hostlib.Loaded(ref_fa, 1)
    qs = hostlib.Loaded(q_fa, 0)
    blocks = mum_spec.parse_mems_file(outs["mem"], ref)
    assert len(blocks) == 2 * qs.n
    exp = [hostlib.format_block(qs.names[b // 2], b % 2, rows[chain_spec.block_chain(rows, 40)[0]], ref)
           for b, (_, rows) in enumerate(blocks)]
    assert b"".join(exp) == outs["one"]
    assert len(outs["one"]) < len(outs["mem"])
