"""-smem on the MI355X (slamem_find_smems_device, Stream(smem=True), slaMEM-hip -smem [-occ N]): every result is the
super-maximal filter of the complete -mem list (tests/smem_spec.py) -- on the golden files the real reference wrote, on
planted and nested repeats against naive substring counting, on blocks large enough for the filter's workgroup path, with the
occurrence cap, through the stream, at the capacity edge and on the N-GPU schedule of the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hostlib
import mum_spec
import smem_spec
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


def assert_is_filter_of(smem, smem_boff, mem, mem_boff, max_occ=0):
    kept, kept_boff = smem_spec.filter_blocks(mem, mem_boff, max_occ)
    assert np.array_equal(np.asarray(smem_boff, dtype=np.int64), kept_boff)
    assert np.array_equal(triples(smem), kept)


def revcomp(s: np.ndarray) -> np.ndarray:
    return COMP[s[::-1]]


@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_engine(eng, case):
    idx = None
    for max_occ in (0, 1):
        _, kept, ref, qs, opts = smem_spec.golden_smem_file(case, max_occ)
        if idx is None:
            idx = eng.Index.build(np.frombuffer(ref.chars, dtype=np.uint8).copy())
        off = np.array(qs.offsets, dtype=np.uint64)
        mems, boff = idx.find_mems(np.frombuffer(qs.chars, dtype=np.uint8), off, int(opt_value(opts, "-l", 20)), "-b" in opts,
                                   smem=True, max_occ=max_occ)
        assert len(boff) == len(kept) + 1
        for b, rows in enumerate(kept):
            assert np.array_equal(triples(mems[int(boff[b]):int(boff[b + 1])]), rows.astype(np.int64)), (case, max_occ, b)
        assert eng.timings()["mum_filter_ms"] > 0
    idx.close()


@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_cli(case, tmp_path):
    expected, _, _, _, _ = smem_spec.golden_smem_file(case)
    ref_fa, q_fa, _, _ = case_paths(case)
    out = tmp_path / "out.txt"
    # -smem first: it takes no value, so it may stand anywhere
    r = subprocess.run([EXE, "-smem"] + MANIFEST[case]["opts"] + ["-o", str(out), ref_fa, q_fa], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    assert out.read_bytes() == expected
    assert b"minimum SMEM length" in r.stdout and b"Saving SMEMs" in r.stdout
    assert b"maximum occurrences" not in r.stdout


@pytest.mark.parametrize("case", ["acgt_l3_both", "ac_l10_both", "long_repeat_l20", "multi_record_ref"])
def test_golden_cases_cli_with_cap(case, tmp_path):
    expected, _, _, _, _ = smem_spec.golden_smem_file(case, 2)
    ref_fa, q_fa, _, _ = case_paths(case)
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + MANIFEST[case]["opts"] + ["-o", str(out), "-occ", "2", ref_fa, "-smem", q_fa],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    assert out.read_bytes() == expected
    assert b"; maximum occurrences = 2\n" in r.stdout


def planted_pair(seed):
    """A reference with nested repeats (a segment, and pieces of it, planted several times), a tandem repeat and a
    reverse-complement palindrome; reads across them, some carrying a segment twice, so that most -mem rows are nested."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=30000)
    seg = ref[1000:1080].copy()
    for at, ln in ((6000, 80), (9000, 70), (12000, 60), (24000, 50)):  # the segment once more, and prefixes of it
        ref[at:at + ln] = seg[:ln]
    for at in (26000, 27000, 28000):
        ref[at:at + 30] = seg[25:55]                      # a piece in the middle, three more times
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
    for a in (990, 5990, 8990, 11990, 14990, 19990, 23990, 25990):  # reads across every planted repeat
        reads.append(ref[a:a + 120].copy())
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return ref, q, off


def strand_of(q, off, b, strands):
    i = b // strands
    s = q[int(off[i]):int(off[i + 1])]
    return revcomp(s) if b % strands else s


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
def test_planted_repeats_against_naive_counting(eng, path, both):
    ref, q, off = planted_pair(5)
    idx = eng.Index.build(ref)
    sk = int(idx.info.seed_k) or 12
    text = ref.tobytes()
    strands = 2 if both else 1
    dropped = kept_multi = 0
    for min_len in (sk + 1, sk + 2, sk + 6):
        with search_path(path):
            mem, mem_boff = idx.find_mems(q, off, min_len, both)
            smem, smem_boff = idx.find_mems(q, off, min_len, both, smem=True)
        assert_is_filter_of(smem, smem_boff, mem, mem_boff)
        rows = triples(mem)
        for b in range(len(mem_boff) - 1):
            s = strand_of(q, off, b, strands).tobytes()
            blk = rows[int(mem_boff[b]):int(mem_boff[b + 1])]
            keep = smem_spec.claim1_keep(text, s, blk)
            got = triples(smem[int(smem_boff[b]):int(smem_boff[b + 1])])
            assert np.array_equal(blk[keep], got), (path, both, min_len, b)
            occ = smem_spec.occurrence_counts(blk)[keep]
            assert np.array_equal(occ, smem_spec.claim2_counts(text, s, got)), (path, both, min_len, b)
            dropped += int((~keep).sum())
            kept_multi += int((occ > 1).sum())
    assert dropped > 0 and kept_multi > 0
    idx.close()


@pytest.mark.parametrize("max_occ", [1, 2, 5])
def test_occurrence_cap_against_naive_counting(eng, max_occ):
    ref, q, off = planted_pair(21)
    idx = eng.Index.build(ref)
    text = ref.tobytes()
    mem, mem_boff = idx.find_mems(q, off, 16, True)
    smem, smem_boff = idx.find_mems(q, off, 16, True, smem=True)
    capped, capped_boff = idx.find_mems(q, off, 16, True, smem=True, max_occ=max_occ)
    assert_is_filter_of(capped, capped_boff, mem, mem_boff, max_occ)
    rows = triples(smem)
    cut = 0
    for b in range(len(smem_boff) - 1):
        s = strand_of(q, off, b, 2).tobytes()
        blk = rows[int(smem_boff[b]):int(smem_boff[b + 1])]
        keep = smem_spec.claim2_counts(text, s, blk) <= max_occ  # the cap by counting in the text
        assert np.array_equal(blk[keep], triples(capped[int(capped_boff[b]):int(capped_boff[b + 1])])), (max_occ, b)
        cut += int((~keep).sum())
    assert cut > 0
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


def test_large_blocks_and_sliced_records(eng):
    """A 2 Mbp record (sliced: longer than 4096 letters; > 10,000 MEMs in its block: the workgroup path) beside short reads
    (the lane path) and a 5,000-letter record, in one batch -- against the filter of the same call's -mem output, with and
    without a cap.  The filter's device time bounds the large block's work: one lane walking its rows would take far longer."""
    ref, qlong = genome_pair(2_000_000, 9)
    rng = np.random.default_rng(10)
    reads = [ref[int(a):int(a) + 150] for a in rng.integers(0, len(ref) - 150, size=50)]
    reads.insert(20, qlong)
    reads.insert(30, ref[5000:10000].copy())
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    idx = eng.Index.build(ref)
    for both in (False, True):
        mem, mem_boff = idx.find_mems(q, off, 20, both)
        assert int(np.diff(mem_boff.astype(np.int64)).max()) >= 10_000
        for max_occ in (0, 2):
            smem, smem_boff = idx.find_mems(q, off, 20, both, smem=True, max_occ=max_occ)
            assert_is_filter_of(smem, smem_boff, mem, mem_boff, max_occ)
            assert 0 < len(smem) < len(mem)
            ms = eng.timings()["mum_filter_ms"]
            assert 0 < ms < 2.0, ms
    idx.close()


def test_stream_equals_one_shot(eng):
    ref, q, off = planted_pair(7)
    idx = eng.Index.build(ref)
    for max_occ in (0, 2):
        one, one_boff = idx.find_mems(q, off, 14, True, smem=True, max_occ=max_occ)
        per = 13
        nq = len(off) - 1
        wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
        st = eng.Stream(idx, 3, 1 << 16, per, True, smem=True, max_occ=max_occ)
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
    for bad in (dict(mam=True, smem=True), dict(mum=True, smem=True), dict(max_occ=2), dict(mum=True, max_occ=1)):
        with pytest.raises(ValueError):
            eng.Stream(idx, 3, 1 << 16, 13, True, **bad)
        with pytest.raises(ValueError):
            idx.find_mems(q, off, 14, True, **bad)
    idx.close()


def test_capacity_between_smem_and_mem_counts(eng):
    import torch
    from slamem_amd import capi
    ref, q, off = planted_pair(11)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    smem, smem_boff = idx.find_mems(q, off, 14, True, smem=True)
    assert len(smem) < len(mem)
    qd = torch.zeros((len(q) + 15) // 8 * 8, dtype=torch.uint8, device=idx.device)
    qd[: len(q)] = torch.from_numpy(q).to(idx.device)
    od = torch.from_numpy(off.view(np.int64)).to(idx.device)
    m = idx.matcher(len(off) - 1, True, (len(smem) + len(mem)) // 2, int(off[-1]), smem=True)
    with pytest.raises(capi.SlamemError) as e:
        m.run(qd, od, 14)
    assert e.value.code == capi.SLAMEM_ERR_CAPACITY
    assert m.last_total == len(mem)
    m2 = idx.matcher(len(off) - 1, True, m.last_total, int(off[-1]), smem=True)
    total = m2.run(qd, od, 14)
    assert total == len(smem)
    got = m2.mems[:total].cpu().numpy().view(np.uint32).reshape(-1, 3).astype(np.int64)
    assert np.array_equal(got, triples(smem))
    assert np.array_equal(m2.block_offsets.cpu().numpy(), smem_boff.astype(np.int64))
    idx.close()


def test_other_modes_unchanged_by_smem_calls(eng):
    ref, q, off = planted_pair(13)
    idx = eng.Index.build(ref)
    modes = (dict(), dict(mam=True), dict(mum=True))
    before = [idx.find_mems(q, off, 14, True, **kw) for kw in modes]
    for max_occ in (0, 1, 3):
        idx.find_mems(q, off, 14, True, smem=True, max_occ=max_occ)
        mid = idx.find_mems(q, off, 14, True)
        assert np.array_equal(triples(mid[0]), triples(before[0][0]))
    after = [idx.find_mems(q, off, 14, True, **kw) for kw in modes]
    assert eng.timings()["mum_filter_ms"] > 0  # (the last call was -mum)
    idx.find_mems(q, off, 14, True)
    assert eng.timings()["mum_filter_ms"] == 0
    for (m0, b0), (m1, b1) in zip(before, after):
        assert np.array_equal(b0, b1)
        assert np.array_equal(triples(m0), triples(m1))
    idx.close()


def test_cli_logical_gpus_byte_identical(tmp_path):
    """The N-GPU schedule of the command line (SLAMEM_LOGICAL_GPUS=2: two streams on the one device, batches alternate)
    passes the mode and the cap to every stream: the file equals the one-GPU file, and the -mem file filtered by the spec."""
    d = str(tmp_path)
    gen = os.path.join(ROOT, "tools", "gen_synth.py")
    g = subprocess.run([sys.executable, gen, "2000000", "20000", "150", "0.02", "7", "50", d], stdout=subprocess.PIPE)
    assert g.returncode == 0
    ref_fa, q_fa = os.path.join(d, "ref.fa"), os.path.join(d, "qry.fa")
    base = dict(os.environ, SLAMEM_BATCH_MB="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for name, args, env in (("mem", [], base), ("one", ["-smem", "-occ", "3"], base),
                            ("two", ["-smem", "-occ", "3"], dict(base, SLAMEM_LOGICAL_GPUS="2"))):
        out = os.path.join(d, f"{name}.txt")
        # (-l 14: chance matches inside the reads' true ones, which -smem drops)
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
    exp = [hostlib.format_block(qs.names[b // 2], b % 2, rows[smem_spec.block_keep(rows, 3)], ref)
           for b, (_, rows) in enumerate(blocks)]
    assert b"".join(exp) == outs["one"]
    assert len(outs["one"]) < len(outs["mem"])


@pytest.mark.parametrize("args", [["-occ", "2"], ["-smem", "-occ", "0"], ["-smem", "-mam", "x"], ["-mum", "x", "-smem"]])
def test_cli_refusals(args, tmp_path):
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_both")
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + args + ["-o", str(out), ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60)
    assert r.returncode == 255
    assert b"> ERROR: Option" in r.stdout
    assert not out.exists()
