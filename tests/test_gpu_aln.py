"""-aln on the MI355X (slamem_find_alns_device, Index.find_alns): every result is tests/aln_spec.py applied to the complete -mem
list of the same engine -- on the golden files the real reference wrote (both search paths, two parameter sets), on every tier
of the gap closure, at every kind of break, at both capacity edges -- and, without the spec, constructed reads must come back
with the CIGAR written down from their construction.  The edit limits here are 31, 3, 2, 1 and 0; limits from 32 to 127, where a
lane of k_aln_wave holds several diagonals and a workgroup closes several gaps, are in tests/test_gpu_aln_edits.py."""
import os
import subprocess

import numpy as np
import pytest

import aln_spec
import ext_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, ecoli_like_pair, opt_value
from test_gpu_chain import indel_reads

pytestmark = pytest.mark.gpu

MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def batch(reads):
    q = np.concatenate(reads) if reads else np.zeros(0, np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return q, off


def seg_rows(segs):
    return np.stack([segs[k] for k in ("ref_pos", "query_pos", "ref_len", "query_len", "edits")], axis=1).astype(np.int64) \
        if len(segs) else np.zeros((0, 5), np.int64)


def assert_equals_blocks(got, blocks):
    segs, boff, ops, ooff = got
    w_segs, w_boff, w_ops, w_ooff = aln_spec.pack(blocks)
    assert np.array_equal(np.asarray(boff, dtype=np.int64), w_boff)
    assert np.array_equal(seg_rows(segs), w_segs)
    assert np.array_equal(np.asarray(ooff, dtype=np.int64), w_ooff)
    assert np.array_equal(np.asarray(ops, dtype=np.uint32), w_ops)


def assert_is_aln_of(got, mem, mem_boff, ref, q, off, both, G=5000, P=4, X=20, E=31, gaps_out=None):
    blocks = aln_spec.filter_blocks(mem, mem_boff, ref, q, off, both, G, P, X, E, gaps_out)
    assert_equals_blocks(got, blocks)
    return blocks


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_engine(eng, case, path):
    idx = None
    for G, P, X, E in ((5000, 4, 20, 31), (200, 1, 5, 3)):
        want, _, ref, qs, opts = aln_spec.golden_aln(case, G, P, X, E)
        text = np.frombuffer(ref.chars, dtype=np.uint8).copy()
        if idx is None:
            idx = eng.Index.build(text)
        q = np.frombuffer(qs.chars, dtype=np.uint8)
        off = np.array(qs.offsets, dtype=np.uint64)
        min_len, both = int(opt_value(opts, "-l", 20)), "-b" in opts
        dflt = (G, P, X, E) == (5000, 4, 20, 31)
        with search_path(path):
            mem, mem_boff = idx.find_mems(q, off, min_len, both)
            got = idx.find_alns(q, off, min_len, both, max_gap=0 if dflt else G, penalty=0 if dflt else P,
                                xdrop=None if dflt else X, max_edits=None if dflt else E)
        assert eng.timings()["mum_filter_ms"] > 0
        assert_is_aln_of(got, mem, mem_boff, text, q, off, both, G, P, X, E)
        assert_equals_blocks(got, want)  # ... which is the spec applied to the file the real reference wrote
    idx.close()


@pytest.mark.parametrize("path", ["seed", "walk"])
def test_constructed_reads_known_answer(eng, path):
    """No spec here: substitutions, one inserted or one deleted letter; the CIGAR comes from the construction."""
    ref, q, off, truth = aln_spec.constructed_reads(11)
    idx = eng.Index.build(ref)
    with search_path(path):
        segs, boff, ops, ooff = idx.find_alns(q, off, 20, True)
    rows = seg_rows(segs)
    for b, seg, rl in truth:
        s, e = int(boff[b]), int(boff[b + 1])
        assert e - s == 1 and tuple(rows[s]) == seg, (b, rows[s:e], seg)
        got = [(aln_spec.CODE_OP[int(w) & 15], int(w) >> 4) for w in ops[int(ooff[s]):int(ooff[s + 1])]]
        assert got == rl, (b, got, rl)
    idx.close()


def test_indel_reads(eng):
    ref, q, off = indel_reads(21)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    for G in (5000, 100):
        gaps = []
        assert_is_aln_of(idx.find_alns(q, off, 14, True, max_gap=G), mem, mem_boff, ref, q, off, True, G=G, gaps_out=gaps)
        assert sum(g is not None and ("I" in g[0] or "D" in g[0]) for _, _, g in gaps) > 50
    idx.close()


def tier_batch():
    """A 400 kbp piece of the E. coli-like genome pair (a block far above the chain's LDS tile, sliced), a 6,000-letter record
    (longer than a slice), short reads with substitutions (inline gaps), reads with several edits close together and with
    indels of up to 30 letters (wave gaps, |a - b| near E), an exact read and a read of N."""
    ref, strain = ecoli_like_pair(duplicates=True)
    ref, strain = ref[:400_000].copy(), strain[:400_000].copy()
    rng = np.random.default_rng(12)
    reads = []
    for a in rng.integers(0, len(ref) - 300, size=40):
        r = ref[int(a):int(a) + 150].copy()
        for x in rng.integers(0, 150, size=3):
            r[int(x)] = rng.choice(ACGT)
        reads.append(r)
    for k, a in enumerate(rng.integers(0, len(ref) - 400, size=40)):
        a = int(a)
        cut = int(rng.integers(1, 34))  # 31 closes at the default, 32 and 33 do not
        if k % 2:
            r = np.concatenate([ref[a:a + 100], ref[a + 100 + cut:a + 220 + cut]])  # letters of the text missing
        else:
            r = np.concatenate([ref[a:a + 100], rng.choice(ACGT, size=cut), ref[a + 100:a + 220]])
        x = 160 + int(rng.integers(0, 10))
        r = r.copy()
        r[x] = rng.choice(ACGT)
        r[x + 2] = rng.choice(ACGT)
        r[x + 5] = rng.choice(ACGT)
        reads.append(r)
    reads.insert(10, strain)
    reads.insert(25, strain[100_000:106_000].copy())
    reads.append(ref[5000:5150].copy())
    reads.append(np.frombuffer(b"N" * 80, dtype=np.uint8).copy())
    q, off = batch(reads)
    return ref, q, off


@pytest.mark.parametrize("path", ["seed", "walk"])
def test_every_tier_in_one_batch(eng, path):
    """The 400 kbp piece is compared in full, every block and every gap."""
    ref, q, off = tier_batch()
    idx = eng.Index.build(ref)
    with search_path(path):
        mem, mem_boff = idx.find_mems(q, off, 14, True)
        got = idx.find_alns(q, off, 14, True)
    gaps = []
    blocks = assert_is_aln_of(got, mem, mem_boff, ref, q, off, True, gaps_out=gaps)
    closed = [(A, B, g) for A, B, g in gaps if g is not None]
    inline = sum(len(A) == len(B) <= 64 and g[1] <= 1 for A, B, g in closed)
    wave = len(closed) - inline
    assert inline > 50 and wave > 20
    assert any(abs(len(A) - len(B)) >= 28 for A, B, g in closed) and any(g is None for _, _, g in gaps)
    assert max(len(s) for s in blocks) >= 1 and max(int(mem_boff[b + 1] - mem_boff[b]) for b in range(len(mem_boff) - 1)) > 1024
    assert blocks[-1] == [] and blocks[-2] == []  # the read of N
    idx.close()


def test_breaks(eng):
    rng = np.random.default_rng(31)
    recs = [rng.choice(ACGT, size=3000) for _ in range(2)]
    ref = np.concatenate([recs[0], [ord("N")], recs[1]]).astype(np.uint8)
    ref[1500] = ord("N")  # an N inside the text where a read has a letter
    r_sub = ref[200:400].copy()
    r_sub[100] = ACGT[(int(np.flatnonzero(ACGT == r_sub[100])[0]) + 1) % 4]
    r_two = ref[600:800].copy()  # distance 2 in one gap: a deleted text letter and a substitution three letters on
    r_two = np.delete(r_two, 100)
    r_two[103] = ACGT[(int(np.flatnonzero(ACGT == r_two[103])[0]) + 1) % 4]
    r_nq = ref[1000:1200].copy()
    r_nq[100] = ord("N")       # an N in the read between two anchors
    r_nt = ref[1400:1600].copy()
    r_nt[100] = ord("A")       # the text has its N here
    r_rec = ref[2900:3100].copy()
    r_rec[100] = ord("C")      # the read has a letter where the text has the N between its records
    q, off = batch([r_sub, r_two, r_nq, r_nt, r_rec])
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 20, True)
    nseg = {}
    for E in (31, 2, 1, 0):
        gaps = []
        blocks = assert_is_aln_of(idx.find_alns(q, off, 20, True, max_edits=E), mem, mem_boff, ref, q, off, True, E=E, gaps_out=gaps)
        nseg[E] = [len(blocks[2 * k]) for k in range(5)]
    assert nseg[31] == [1, 1, 2, 2, 2] and nseg[2] == [1, 1, 2, 2, 2] and nseg[1] == [1, 2, 2, 2, 2] and nseg[0] == [2, 2, 2, 2, 2]
    idx.close()


def test_both_capacity_edges(eng):
    from slamem_amd import capi
    ref, q, off = indel_reads(11)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    segs, boff, ops, ooff = idx.find_alns(q, off, 14, True)
    want = (len(mem), len(segs), len(ops))
    assert len(segs) > 100 and len(ops) > len(segs)
    for caps in ((len(mem) - 1, len(segs), len(ops)), (len(mem), len(segs) - 1, len(ops)), (len(mem), len(segs), len(ops) - 1)):
        with pytest.raises(capi.SlamemError) as e:
            idx.find_alns(q, off, 14, True, capacities=caps)
        assert e.value.code == capi.SLAMEM_ERR_CAPACITY
        if caps[0] == len(mem):
            assert e.value.totals == want
        else:
            assert e.value.totals[0] >= len(mem) and e.value.totals[1:] == (0, 0)
    got = idx.find_alns(q, off, 14, True, capacities=want)  # exactly enough
    for a, b in zip(got, (segs, boff, ops, ooff)):
        assert np.array_equal(a, b)
    idx.close()


def test_compact_index_is_refused_and_still_searches(eng, monkeypatch):
    from slamem_amd import capi
    ref, q, off = indel_reads(13)
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    idx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    assert idx.info.layout == capi.LAYOUT_COMPACT
    with pytest.raises(capi.SlamemError) as e:
        idx.find_alns(q, off, 14, True)
    assert e.value.code == capi.SLAMEM_ERR_ARG
    assert "text planes" in str(e.value) and "compact" in str(e.value)
    mem, _ = idx.find_mems(q, off, 14, True)  # the process and the index go on
    assert len(mem) > 40
    with pytest.raises(capi.SlamemError):
        eng.Index.build(ref).find_alns(q, off, 14, True, max_edits=128)
    idx.close()


def test_other_modes_unchanged_by_aln_calls(eng):
    ref, q, off = indel_reads(13)
    idx = eng.Index.build(ref)
    before = (idx.find_mems(q, off, 14, True), idx.find_chains(q, off, 14, True), idx.find_exts(q, off, 14, True))
    idx.find_alns(q, off, 14, True)
    after = (idx.find_mems(q, off, 14, True), idx.find_chains(q, off, 14, True), idx.find_exts(q, off, 14, True))
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(a, b)
    idx.close()


@pytest.mark.parametrize("params", [(5000, 4, 20, 31), (200, 1, 5, 3)], ids=["defaults", "mgap200-pen1-xdrop5-maxed3"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_cli(case, params, tmp_path):
    """The executable's file, byte for byte: the spec's segments formatted by the front end's writer."""
    G, P, X, E = params
    expected = aln_spec.golden_aln_file(case, G, P, X, E)
    ref_fa, q_fa, _, _ = case_paths(case)
    out = tmp_path / "out.txt"
    opts = MANIFEST[case]["opts"]
    if params == (5000, 4, 20, 31):  # -aln takes no value, so it may stand anywhere
        argv = [EXE] + opts + ["-o", str(out), ref_fa, "-aln", q_fa]
    else:
        argv = [EXE, "-aln", "-maxed", str(E), "-pen", str(P)] + opts + ["-o", str(out), ref_fa, q_fa, "-xdrop", str(X), "-mgap", str(G)]
    r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    assert out.read_bytes() == expected
    assert b"minimum alignment length" in r.stdout and b"Saving alignments" in r.stdout
    assert (b"; maximum gap = %d ; mismatch penalty = %d ; X-drop = %d ; maximum edits = %d\n" % (G, P, X, E)) in r.stdout


@pytest.mark.parametrize("args", [["-aln", "-chain"], ["-aln", "-ext"], ["-aln", "-mam", "x"], ["-aln", "-smem"], ["-aln", "-mum"],
                                  ["-maxed", "3"], ["-aln", "-maxed", "128"], ["-aln", "-maxed", "few"], ["-aln", "-maxed", "-1"]])
def test_cli_refusals(args, tmp_path):
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + args + ["-o", str(out), ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and b"> ERROR: " in r.stdout and not out.exists()


def test_stream_equals_one_shot(eng):
    from slamem_amd import capi
    ref, q, off = indel_reads(7)
    idx = eng.Index.build(ref)
    for kw in (dict(), dict(max_gap=100, penalty=2, xdrop=7, max_edits=2), dict(max_edits=0), dict(max_edits=127)):
        segs, boff, ops, ooff = idx.find_alns(q, off, 14, True, **kw)
        per = 13
        nq = len(off) - 1
        wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
        st = eng.Stream(idx, 3, 1 << 16, per, True, aln=True, **kw)
        g_segs, g_counts, g_ops, g_nops = [], [], [], []
        st.submit(q, wins[0], 14)
        st.submit(q, wins[1], 14)
        for b in range(len(wins)):
            m, bo, tm = st.next()
            o, oo = st.alns()
            assert len(m) == int(bo[-1]) == len(oo) - 1 and int(oo[-1]) == len(o) and int(oo[0]) == 0
            if b + 2 < len(wins):
                st.submit(q, wins[b + 2], 14)  # every slot in use
            g_segs.append(seg_rows(m))
            g_counts.append(np.diff(bo.astype(np.int64)))
            g_ops.append(o)
            g_nops.append(np.diff(oo.astype(np.int64)))
        st.close()
        assert np.array_equal(np.concatenate(g_segs), seg_rows(segs))
        assert np.array_equal(np.concatenate(g_counts), np.diff(boff.astype(np.int64)))
        assert np.array_equal(np.concatenate(g_ops), ops)
        assert np.array_equal(np.concatenate(g_nops), np.diff(ooff.astype(np.int64)))
    for bad in (dict(aln=True, chain=True), dict(aln=True, ext=True), dict(aln=True, mam=True), dict(max_edits=3),
                dict(ext=True, max_edits=3)):
        with pytest.raises((ValueError, capi.SlamemError)):
            eng.Stream(idx, 3, 1 << 16, 13, True, **bad)
    with pytest.raises(capi.SlamemError):
        eng.Stream(idx, 3, 1 << 16, 13, True, aln=True, max_edits=128)
    idx.close()


def test_ecoli_like_genome_pair(eng):
    """The 4.6 Mbp genome pair: one chain of tens of thousands of rows.  The matrix checker is too slow for every gap with
    pieces of thousands of letters, so: the chain's anchors and every segment's ends, lengths and edit count are compared in
    full against the spec evaluated with the wavefront form (aln_spec.wavefront_ops, which tests/test_aln_host.py holds to the
    matrix); the matrix itself checks a sample of 300 gaps; and every CIGAR is replayed over the two sequences.  The 400 kbp
    piece above is compared in full with the matrix."""
    ref, strain = ecoli_like_pair(duplicates=True)
    idx = eng.Index.build(ref)
    q, off = batch([strain])
    mem, mem_boff = idx.find_mems(q, off, 20, False)
    segs, boff, ops, ooff = idx.find_alns(q, off, 20, False)
    idx.close()
    matrix = aln_spec.gap_ops
    gaps = []
    try:
        aln_spec.gap_ops = aln_spec.wavefront_ops
        blocks = aln_spec.filter_blocks(mem, mem_boff, ref, q, off, False, gaps_out=gaps)
    finally:
        aln_spec.gap_ops = matrix
    assert_equals_blocks((segs, boff, ops, ooff), blocks)
    assert len(mem) > 30_000 and len(gaps) > 10_000
    rng = np.random.default_rng(3)
    small = [k for k, (A, B, g) in enumerate(gaps) if len(A) * len(B) <= 4_000_000]
    for k in rng.choice(small, size=300, replace=False):
        A, B, g = gaps[int(k)]
        assert matrix(A, B) == g
    Q, T = strain.tobytes(), ref.tobytes()
    rows = seg_rows(segs)
    for i in range(len(rows)):  # replay
        x, y, cost = int(rows[i][1]), int(rows[i][0]), 0
        for w in ops[int(ooff[i]):int(ooff[i + 1])]:
            c, n = aln_spec.CODE_OP[int(w) & 15], int(w) >> 4
            if c in "=X":
                a = np.frombuffer(Q[x:x + n], dtype=np.uint8) & 0xDF
                b = np.frombuffer(T[y:y + n], dtype=np.uint8) & 0xDF
                assert bool((a == b).all()) if c == "=" else bool((a != b).all())
                x, y = x + n, y + n
            elif c == "I":
                x += n
            else:
                y += n
            cost += n if c != "=" else 0
        assert (x - int(rows[i][1]), y - int(rows[i][0]), cost) == (int(rows[i][3]), int(rows[i][2]), int(rows[i][4]))


def test_cli_logical_gpus_byte_identical(tmp_path):
    """The N-GPU schedule of the command line (SLAMEM_LOGICAL_GPUS=2: two streams on the one device, batches alternate) passes
    the mode and its parameters to every stream, and every batch's operations stay with its segments."""
    import sys
    import hostlib
    import mum_spec
    d = str(tmp_path)
    gen = os.path.join(ROOT, "tools", "gen_synth.py")
    g = subprocess.run([sys.executable, gen, "2000000", "20000", "150", "0.02", "7", "50", d], stdout=subprocess.PIPE)
    assert g.returncode == 0
    ref_fa, q_fa = os.path.join(d, "ref.fa"), os.path.join(d, "qry.fa")
    base = dict(os.environ, SLAMEM_BATCH_MB="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for name, args, env in (("mem", [], base), ("one", ["-aln", "-maxed", "2"], base),
                            ("two", ["-aln", "-maxed", "2"], dict(base, SLAMEM_LOGICAL_GPUS="2"))):
        out = os.path.join(d, f"{name}.txt")
        r = subprocess.run([EXE, "-b", "-l", "20"] + args + ["-o", out, ref_fa, q_fa], stdout=subprocess.PIPE,
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
    chars = np.frombuffer(qs.chars, dtype=np.uint8)
    exp = []
    for b, (_, rows) in enumerate(blocks[:4000]):  # (the checker is slow: the first 2,000 reads)
        rec = chars[qs.offsets[b // 2]:qs.offsets[b // 2 + 1]]
        segl = aln_spec.block_aln(rows, ext_spec.revcomp(rec) if b % 2 else rec, ref.chars, E=2)
        exp.append(aln_spec.format_block(qs.names[b // 2], b % 2, segl, ref))
    exp = b"".join(exp)
    assert outs["one"][:len(exp)] == exp
    assert outs["one"].count(b"\n") < outs["mem"].count(b"\n")


def test_host_convenience_call(eng):
    """slamem_find_alns_host (upload, the retries on all three capacities, four malloc()ed arrays) against Index.find_alns."""
    import ctypes as C
    from slamem_amd import capi
    ref, q, off = indel_reads(17)
    idx = eng.Index.build(ref)
    want = idx.find_alns(q, off, 14, True, max_edits=5)
    L = capi.lib()
    segs, boff, ops, ooff = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    totals = (C.c_uint64 * 3)()
    qb = np.ascontiguousarray(q).tobytes()
    offs = np.ascontiguousarray(off, dtype=np.uint64)
    # min_len 14 on reads of 200 letters: the first guess of the -mem room (two rows per min_len letters) is generous, the
    # guesses for segments and operations are not tuned to this batch -- whichever is short, the call has to come back whole
    rc = L.slamem_find_alns_host(idx._h, qb, offs.ctypes.data, len(offs) - 1, 14, 1, 0, 0, 0xFFFFFFFF, 5, C.byref(segs), C.byref(boff),
                                 C.byref(ops), C.byref(ooff), totals)
    assert rc == capi.SLAMEM_OK, L.slamem_last_error_message()
    nseg, nops, nb = int(totals[1]), int(totals[2]), 2 * (len(offs) - 1)
    assert (nseg, nops) == (len(want[0]), len(want[2]))
    got_segs = np.ctypeslib.as_array((C.c_uint32 * (5 * max(nseg, 1))).from_address(segs.value))[: 5 * nseg].reshape(-1, 5)
    assert np.array_equal(got_segs.astype(np.int64), seg_rows(want[0]))
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint64 * (nb + 1)).from_address(boff.value)), want[1])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint32 * max(nops, 1)).from_address(ops.value))[:nops], want[2])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint64 * (nseg + 1)).from_address(ooff.value)), want[3])
    for p in (segs, boff, ops, ooff):
        L.slamem_host_free(p)
    idx.close()
