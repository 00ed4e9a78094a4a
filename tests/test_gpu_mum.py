"""-mum on the MI355X (slamem_find_mums_device, Stream(mum=True), slaMEM-hip ... -mum): every result is the containment filter
of the complete -mem list (tests/mum_spec.py) -- on the golden files the real reference wrote, on planted repeats against
naive occurrence counting, on blocks large enough for the filter's sort path, through the stream and at the capacity edge."""
import os
import subprocess

import numpy as np
import pytest

import mum_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, opt_value

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


def assert_is_filter_of(mum, mum_boff, mem, mem_boff):
    kept, kept_boff = mum_spec.filter_blocks(mem, mem_boff)
    assert np.array_equal(np.asarray(mum_boff, dtype=np.int64), kept_boff)
    assert np.array_equal(triples(mum), kept)


def revcomp(s: np.ndarray) -> np.ndarray:
    return COMP[s[::-1]]


@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_engine(eng, case):
    _, kept, ref, qs, opts = mum_spec.golden_mum_file(case)
    idx = eng.Index.build(np.frombuffer(ref.chars, dtype=np.uint8).copy())
    off = np.array(qs.offsets, dtype=np.uint64)
    mems, boff = idx.find_mems(np.frombuffer(qs.chars, dtype=np.uint8), off, int(opt_value(opts, "-l", 20)), "-b" in opts,
                               mum=True)
    assert len(boff) == len(kept) + 1
    for b, rows in enumerate(kept):
        assert np.array_equal(triples(mems[int(boff[b]):int(boff[b + 1])]), rows.astype(np.int64)), (case, b)
    assert eng.timings()["mum_filter_ms"] > 0
    idx.close()


@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_cli(case, tmp_path):
    expected, _, _, _, _ = mum_spec.golden_mum_file(case)
    ref_fa, q_fa, _, _ = case_paths(case)
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + MANIFEST[case]["opts"] + ["-o", str(out), ref_fa, q_fa, "-mum"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    assert out.read_bytes() == expected
    assert b"minimum MUM length" in r.stdout and b"Saving MUMs" in r.stdout


def planted_pair(seed):
    """A reference with a segment planted twice and a tandem repeat; reads from it, some carrying a segment twice, some a
    reverse-complement palindrome (its own reverse complement: found on both strands under -b)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=30000)
    seg = ref[1000:1060].copy()
    ref[9000:9060] = seg                                  # a segment twice in the reference
    unit = rng.choice(acgt, size=7)
    ref[15000:15070] = np.tile(unit, 10)                  # a self-overlapping tandem repeat
    half = rng.choice(acgt, size=20)
    ref[20000:20040] = np.concatenate([half, revcomp(half)])  # a reverse-complement palindrome
    reads = []
    for k in range(120):
        a = int(rng.integers(0, len(ref) - 150))
        r = ref[a:a + 150].copy()
        if k % 4 == 1:                                     # a segment twice in one read
            r[100:130] = r[10:40]
        mut = rng.random(150) < 0.02
        r[mut] = rng.choice(acgt, size=int(mut.sum()))
        reads.append(r)
    for a in (990, 8990, 14990, 19990):                   # reads across every planted repeat
        reads.append(ref[a:a + 100].copy())
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return ref, q, off


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
def test_planted_repeats_against_naive_counting(eng, path, both):
    ref, q, off = planted_pair(5)
    idx = eng.Index.build(ref)
    sk = int(idx.info.seed_k) or 12
    text = ref.tobytes()
    dropped = 0
    for min_len in (sk + 1, sk + 2, sk + 6):
        with search_path(path):
            mem, mem_boff = idx.find_mems(q, off, min_len, both)
            mum, mum_boff = idx.find_mems(q, off, min_len, both, mum=True)
        assert_is_filter_of(mum, mum_boff, mem, mem_boff)
        strands = 2 if both else 1
        rows = triples(mem)
        for b in range(len(mem_boff) - 1):
            i = b // strands
            s = q[int(off[i]):int(off[i + 1])]
            if b % strands:
                s = revcomp(s)
            blk = rows[int(mem_boff[b]):int(mem_boff[b + 1])]
            keep = mum_spec.naive_keep(text, s.tobytes(), blk)
            assert np.array_equal(blk[keep], triples(mum[int(mum_boff[b]):int(mum_boff[b + 1])])), (path, both, min_len, b)
            dropped += int((~keep).sum())
    assert dropped > 0
    idx.close()


def genome_pair(n, seed):
    """A reference with planted duplications and a query that is a mutated copy of it (1.5 % substitutions)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=n)
    for _ in range(8):
        a, b = (int(x) for x in rng.integers(0, n - 3000, size=2))
        ref[b:b + 2000] = ref[a:a + 2000]
    q = ref.copy()
    mut = rng.random(n) < 0.015
    q[mut] = rng.choice(acgt, size=int(mut.sum()))
    a = int(rng.integers(0, n - 5000))
    q[a + 2000:a + 3000] = q[a:a + 1000]                  # a duplication inside the query
    return ref, q


def test_large_blocks_sort_path_and_sliced_record(eng):
    """One 300 kbp record (sliced: longer than 4096 letters; thousands of MEMs per block: the sort path), beside short reads
    in the same batch (their blocks take the lane path) -- against the containment filter of the same call's -mem output."""
    ref, qlong = genome_pair(300_000, 9)
    rng = np.random.default_rng(10)
    reads = [ref[int(a):int(a) + 150] for a in rng.integers(0, len(ref) - 150, size=50)]
    reads.insert(20, qlong)
    reads.insert(30, ref[5000:10000].copy())               # a 5,000-letter record: sliced, below the sort path's size
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    idx = eng.Index.build(ref)
    for both in (False, True):
        mem, mem_boff = idx.find_mems(q, off, 20, both)
        mum, mum_boff = idx.find_mems(q, off, 20, both, mum=True)
        assert eng.timings()["mum_filter_ms"] > 0
        assert int(np.diff(mem_boff.astype(np.int64)).max()) > 256  # a block above the lane path's limit
        assert_is_filter_of(mum, mum_boff, mem, mem_boff)
        assert 0 < len(mum) < len(mem)
    idx.close()


def test_stream_equals_one_shot(eng):
    ref, q, off = planted_pair(7)
    idx = eng.Index.build(ref)
    one, one_boff = idx.find_mems(q, off, 14, True, mum=True)
    per = 13
    nq = len(off) - 1
    wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
    st = eng.Stream(idx, 3, 1 << 16, per, True, mum=True)
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
    with pytest.raises(ValueError):
        eng.Stream(idx, 3, 1 << 16, per, True, mam=True, mum=True)
    with pytest.raises(ValueError):
        idx.find_mems(q, off, 14, True, mam=True, mum=True)
    idx.close()


def test_capacity_between_mum_and_mem_counts(eng):
    import torch
    from slamem_amd import capi
    ref, q, off = planted_pair(11)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    mum, mum_boff = idx.find_mems(q, off, 14, True, mum=True)
    assert len(mum) < len(mem)
    qd = torch.zeros((len(q) + 15) // 8 * 8, dtype=torch.uint8, device=idx.device)
    qd[: len(q)] = torch.from_numpy(q).to(idx.device)
    od = torch.from_numpy(off.view(np.int64)).to(idx.device)
    m = idx.matcher(len(off) - 1, True, (len(mum) + len(mem)) // 2, int(off[-1]), mum=True)
    with pytest.raises(capi.SlamemError) as e:
        m.run(qd, od, 14)
    assert e.value.code == capi.SLAMEM_ERR_CAPACITY
    assert m.last_total == len(mem)
    m2 = idx.matcher(len(off) - 1, True, m.last_total, int(off[-1]), mum=True)
    total = m2.run(qd, od, 14)
    assert total == len(mum)
    got = m2.mems[:total].cpu().numpy().view(np.uint32).reshape(-1, 3).astype(np.int64)
    assert np.array_equal(got, triples(mum))
    assert np.array_equal(m2.block_offsets.cpu().numpy(), mum_boff.astype(np.int64))
    idx.close()


def test_other_modes_unchanged_by_mum_calls(eng):
    ref, q, off = planted_pair(13)
    idx = eng.Index.build(ref)
    before = [idx.find_mems(q, off, 14, True, mam=mam) for mam in (False, True)]
    assert eng.timings()["mum_filter_ms"] == 0
    for _ in range(2):
        idx.find_mems(q, off, 14, True, mum=True)
    after = [idx.find_mems(q, off, 14, True, mam=mam) for mam in (False, True)]
    assert eng.timings()["mum_filter_ms"] == 0
    for (m0, b0), (m1, b1) in zip(before, after):
        assert np.array_equal(b0, b1)
        assert np.array_equal(triples(m0), triples(m1))
    idx.close()


def test_cli_nothing_found(tmp_path):
    """Two queries that match nothing of at least 60 letters: no MUMs, and the average line divides by the query count."""
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    (tmp_path / "ref.fa").write_bytes(b">r\n" + rng.choice(acgt, size=5000).tobytes() + b"\n")
    (tmp_path / "q.fa").write_bytes(b">a\n" + rng.choice(acgt, size=300).tobytes() + b"\n>b\n" +
                                    rng.choice(acgt, size=300).tobytes() + b"\n")
    r = subprocess.run([EXE, "-b", "-l", "60", "-o", "out.txt", "ref.fa", "q.fa", "-mum"], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    assert b":: Average 0 MUMs found per query sequence (total = 0, avg size = 0 bp)" in r.stdout
    assert (tmp_path / "out.txt").read_bytes() == b">a\n>a Reverse\n>b\n>b Reverse\n"
