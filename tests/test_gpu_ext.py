"""-ext on the MI355X (slamem_find_exts_device, Index.find_exts, Stream(ext=True), slaMEM-hip -ext [-pen N] [-xdrop N]): every
result is the extension filter of the complete -mem list of the same engine by the per-letter definition (tests/ext_spec.py)
-- on the golden files the real reference wrote, on every tier of the filter, at every kind of end an extension can have,
through the stream, at the capacity edge and on the command line -- and, without the spec, reads with planted substitutions
must come back as one row of their whole length with the planted number of mismatches."""
import os
import subprocess

import numpy as np
import pytest

import ext_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, ecoli_like_pair, opt_value

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def triples(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


def batch(reads):
    q = np.concatenate(reads) if reads else np.zeros(0, np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return q, off


def assert_is_ext_of(rows, boff, mms, mem, mem_boff, ref, q, off, both, P=ext_spec.DEFAULT_PENALTY, X=ext_spec.DEFAULT_XDROP,
                     fast=False):
    want, want_boff, want_mm = ext_spec.filter_blocks(mem, mem_boff, ref, q, off, both, P, X, fast)
    assert np.array_equal(np.asarray(boff, dtype=np.int64), want_boff)
    assert np.array_equal(triples(rows), want)
    assert np.array_equal(np.asarray(mms, dtype=np.int64), want_mm)
    return want, want_mm


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_engine(eng, case, path):
    idx = None
    for P, X in ((4, 20), (1, 5)):
        _, kept, mms, ref, qs, opts = ext_spec.golden_ext_file(case, P, X)
        text = np.frombuffer(ref.chars, dtype=np.uint8).copy()
        if idx is None:
            idx = eng.Index.build(text)
        q = np.frombuffer(qs.chars, dtype=np.uint8)
        off = np.array(qs.offsets, dtype=np.uint64)
        min_len, both = int(opt_value(opts, "-l", 20)), "-b" in opts
        with search_path(path):
            mem, mem_boff = idx.find_mems(q, off, min_len, both)
            rows, boff, mm = idx.find_exts(q, off, min_len, both, penalty=0 if P == 4 else P, xdrop=None if X == 20 else X)
        assert eng.timings()["mum_filter_ms"] > 0
        # the spec applied to the -mem list of the same engine ...
        assert_is_ext_of(rows, boff, mm, mem, mem_boff, text, q, off, both, P, X)
        # ... which is the spec applied to the file the real reference wrote
        assert len(boff) == len(kept) + 1
        for b, (k, m) in enumerate(zip(kept, mms)):
            assert np.array_equal(triples(rows[int(boff[b]):int(boff[b + 1])]), k), (case, P, X, b)
            assert np.array_equal(mm[int(boff[b]):int(boff[b + 1])].astype(np.int64), m), (case, P, X, b)
    idx.close()


@pytest.mark.parametrize("params", [(4, 20), (1, 5)], ids=["defaults", "pen1-xdrop5"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_cli(case, params, tmp_path):
    P, X = params
    expected, _, _, _, _, _ = ext_spec.golden_ext_file(case, P, X)
    ref_fa, q_fa, _, _ = case_paths(case)
    out = tmp_path / "out.txt"
    opts = MANIFEST[case]["opts"]
    # -ext takes no value, so it may stand anywhere; the values of -pen and -xdrop are never taken for files
    if (P, X) == (4, 20):
        argv = [EXE] + opts + ["-o", str(out), ref_fa, "-ext", q_fa]
    else:
        argv = [EXE, "-ext", "-pen", str(P)] + opts + ["-o", str(out), ref_fa, q_fa, "-xdrop", str(X)]
    r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    assert out.read_bytes() == expected
    assert b"minimum extended MEM length" in r.stdout and b"Saving extended MEMs" in r.stdout
    assert (b"; mismatch penalty = %d ; X-drop = %d\n" % (P, X)) in r.stdout


@pytest.mark.parametrize("path", ["seed", "walk"])
def test_planted_substitutions_known_answer(eng, path):
    """No spec here: a 200-letter read with 0-4 planted substitutions, each 10 or more letters from the ends and 25 or more
    apart, must give (a, 0, 200) with exactly the planted number of mismatches, once, in its matching strand's block."""
    ref, q, off, truth = ext_spec.planted_reads(5, count=300)
    idx = eng.Index.build(ref)
    with search_path(path):
        rows, boff, mm = idx.find_exts(q, off, 20, True)
    t = triples(rows)
    planted_total = 0
    for k, (a, rev, planted) in enumerate(truth):
        b = 2 * k + (1 if rev else 0)
        s, e = int(boff[b]), int(boff[b + 1])
        hit = [i for i in range(s, e) if tuple(t[i]) == (a, 0, 200)]
        assert len(hit) == 1, (k, a, rev, planted, t[s:e])
        assert int(mm[hit[0]]) == planted
        planted_total += planted
    assert planted_total > 300
    idx.close()


def tier_batch():
    """A 400 kbp piece of the E. coli-like genome pair (sliced; a block of thousands of rows on the large-block list, its
    extensions run over many text units and many seeds collapse into one segment), a 6,000-letter record (longer than a slice,
    some tens of rows), short reads with substitutions (blocks of one to a few rows), an exact read (one row) and a read of N
    (an empty block), in one batch."""
    ref, strain = ecoli_like_pair(duplicates=True)
    ref, strain = ref[:400_000].copy(), strain[:400_000].copy()
    rng = np.random.default_rng(12)
    reads = []
    for a in rng.integers(0, len(ref) - 150, size=40):
        r = ref[int(a):int(a) + 150].copy()
        for x in rng.integers(0, 150, size=3):
            r[int(x)] = rng.choice(ACGT)
        reads.append(r)
    reads.insert(10, strain)
    reads.insert(25, strain[100_000:106_000].copy())
    reads.append(ref[5000:5150].copy())
    reads.append(np.frombuffer(b"N" * 80, dtype=np.uint8).copy())
    q, off = batch(reads)
    return ref, q, off


def test_every_tier_and_a_sliced_record(eng):
    ref, q, off = tier_batch()
    idx = eng.Index.build(ref)
    for both in (False, True):
        mem, mem_boff = idx.find_mems(q, off, 20, both)
        sizes = np.diff(mem_boff.astype(np.int64))
        assert sizes.max() > 1024 and np.any((sizes > 32) & (sizes <= 1024)) and np.any(sizes == 1) and np.any(sizes == 0)
        for P, X in ((4, 20), (1, 100)) if both else ((4, 20),):
            rows, boff, mm = idx.find_exts(q, off, 20, both, penalty=P, xdrop=X)
            assert eng.timings()["mum_filter_ms"] > 0
            want, want_mm = assert_is_ext_of(rows, boff, mm, mem, mem_boff, ref, q, off, both, P, X, fast=True)
            assert len(rows) < len(mem)                        # seeds collapsed into segments
            assert int(want[:, 2].max()) > 2000                # an extension over tens of text units
            assert int(want_mm.max()) > 20
    idx.close()


def test_ecoli_like_genome_pair(eng):
    """The 4.6 Mbp genome pair: one block of tens of thousands of rows whose sides run for hundreds of thousands of letters.  The
    letter-wise checker needs about ten milliseconds per row and million letters -- hours for every row -- so here a sample of
    300 -mem rows is extended by the spec (every sampled row's segment must be in the output with its mismatches) and the
    whole output is held to what needs no extension: rows pairwise different, each covering the seed of a -mem row of its
    diagonal, every -mem row covered by an output row of its diagonal.  The 400 kbp piece above is compared row for row."""
    ref, strain = ecoli_like_pair(duplicates=True)
    idx = eng.Index.build(ref)
    q, off = batch([strain])
    mem, mem_boff = idx.find_mems(q, off, 20, False)
    rows, boff, mm = idx.find_exts(q, off, 20, False)
    idx.close()
    t, m = triples(rows), triples(mem)
    assert len(m) > 30_000 and len(t) < len(m) // 4  # 1.5 % substitutions: most seeds of a diagonal are one segment
    assert list(boff) == [0, len(t)]
    out = {tuple(r): int(x) for r, x in zip(t, mm)}
    assert len(out) == len(t)
    rng = np.random.default_rng(3)
    for i in rng.choice(len(m), size=300, replace=False):
        seg, want = ext_spec.extend_row(strain, ref, m[i], fast=True)
        assert out.get(seg) == want, (m[i], seg, want)
    # every -mem row lies inside an output row of its diagonal, and every output row holds one
    by_diag = {}
    for p, qq, ln in t:
        by_diag.setdefault(int(p - qq), []).append((int(qq), int(qq + ln)))
    covered = set()
    for p, qq, ln in m:
        hits = [k for k, (a, e) in enumerate(by_diag.get(int(p - qq), [])) if a <= qq and qq + ln <= e]
        assert hits
        covered.update((int(p - qq), k) for k in hits)
    assert len(covered) == len(t)
    assert int(t[:, 2].max()) > 100_000 and int(mm.max()) > 1000


def test_ends_of_every_kind(eng):
    """Extensions that stop at the record's first / last letter, at text position 0 and n - 1, at an N in the read, and at the N
    between two reference records: a read spanning two records gives two rows, none crossing."""
    rng = np.random.default_rng(77)
    rec_a, rec_b = rng.choice(ACGT, size=3000), rng.choice(ACGT, size=2500)
    ref = np.concatenate([rec_a, np.frombuffer(b"N", dtype=np.uint8), rec_b])
    n = len(ref)
    def sub(r, *at):
        r = r.copy()
        for x in at:
            r[x] = ACGT[(int(np.flatnonzero(ACGT == r[x])[0]) + 1) % 4]
        return r
    reads = [
        sub(ref[0:120], 30, 75),                  # starts at text position 0
        sub(ref[n - 120:n], 40, 90),              # ends at text position n - 1
        sub(ref[500:700], 50, 120),               # the record's own ends, inside the text
        sub(ref[2900:3100], 40, 150),             # spans the N between the two records
        ref[1000:1200].copy(),                    # an N in the read
        np.concatenate([rng.choice(ACGT, size=7), sub(ref[1500:1640], 60), rng.choice(ACGT, size=9)]),  # ends inside the read
    ]
    reads[3][100] = ord("A")  # (a read carries a letter where the merged text has its separator; N = N would be -mem's match)
    reads[4][100] = ord("N")
    reads[4] = sub(reads[4], 30, 160)
    reads.append(ext_spec.revcomp(reads[3]))
    q, off = batch(reads)
    idx = eng.Index.build(ref)
    for both in (False, True):
        mem, mem_boff = idx.find_mems(q, off, 20, both)
        rows, boff, mm = idx.find_exts(q, off, 20, both)
        assert_is_ext_of(rows, boff, mm, mem, mem_boff, ref, q, off, both)
        t = triples(rows)
        s = 2 if both else 1
        blk = lambda k, strand=0: [tuple(int(v) for v in r) + (int(m),) for r, m in
                                   zip(t[int(boff[s * k + strand]):int(boff[s * k + strand + 1])],
                                       mm[int(boff[s * k + strand]):int(boff[s * k + strand + 1])])]
        assert (0, 0, 120, 2) in blk(0)
        assert (n - 120, 0, 120, 2) in blk(1)
        assert (500, 0, 200, 2) in blk(2)
        # two rows at the record separator (position 3000): [2900, 3000) and [3001, 3100)
        assert (2900, 0, 100, 1) in blk(3) and (3001, 101, 99, 1) in blk(3)
        assert not any(p <= 3000 < p + ln for p, _, ln, _ in blk(3))
        # the N at read letter 100 splits the read
        assert (1000, 0, 100, 1) in blk(4) and (1101, 101, 99, 1) in blk(4)
        # the piece inside random flanks: one row on its diagonal over the whole piece (a flank letter that happens to agree is
        # taken; the disagreeing ones behind it are not)
        assert any(p - qq == 1493 and qq <= 7 and qq + ln >= 147 and m >= 1 for p, qq, ln, m in blk(5))
        if both:
            assert (2900, 0, 100, 1) in blk(6, 1) and (3001, 101, 99, 1) in blk(6, 1)
    idx.close()


def mutated_reads(seed, count=160):
    rng = np.random.default_rng(seed)
    ref = rng.choice(ACGT, size=30000)
    reads = []
    for k in range(count):
        a = int(rng.integers(0, len(ref) - 200))
        r = ref[a:a + 200].copy()
        mut = rng.random(200) < 0.03
        r[mut] = rng.choice(ACGT, size=int(mut.sum()))
        reads.append(ext_spec.revcomp(r) if k % 3 == 0 else r)
    q, off = batch(reads)
    return ref, q, off


def test_xdrop_zero_and_a_large_drop(eng):
    ref, q, off = mutated_reads(21)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    # X = 0: every side ends at its first mismatch -- the rows are the -mem rows, no mismatch, nothing dropped
    rows, boff, mm = idx.find_exts(q, off, 14, True, xdrop=0)
    assert np.array_equal(triples(rows), triples(mem)) and np.array_equal(boff, mem_boff) and not mm.any()
    assert_is_ext_of(rows, boff, mm, mem, mem_boff, ref, q, off, True, 4, 0)
    # P = 1 and a drop nothing reaches: the sides run on through the random letters beside a read's place
    rows, boff, mm = idx.find_exts(q, off, 14, True, penalty=1, xdrop=10_000)
    want, want_mm = assert_is_ext_of(rows, boff, mm, mem, mem_boff, ref, q, off, True, 1, 10_000)
    assert len(rows) < len(mem) and int(want_mm.max()) >= 4
    idx.close()


def test_stream_equals_one_shot(eng):
    from slamem_amd import capi
    ref, q, off = mutated_reads(7)
    idx = eng.Index.build(ref)
    for kw in (dict(), dict(penalty=2, xdrop=7), dict(xdrop=0)):
        one, one_boff, one_mm = idx.find_exts(q, off, 14, True, **kw)
        per = 13
        nq = len(off) - 1
        wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
        for packed in (False, True):
            st = eng.Stream(idx, 3, 1 << 16, per, True, ext=True, **kw)
            keep = []

            def submit(w):
                if not packed:
                    st.submit(q, w, 14)
                    return
                chars = np.ascontiguousarray(q[int(w[0]):int(w[-1])])
                rel = (w - w[0]).astype(np.uint64)
                units = int(((np.diff(rel.astype(np.int64)) + 63) // 64).sum())
                planes = eng.PinnedBuffer(16 * units + 64)  # (16-byte aligned)
                other = np.zeros(units + 1, dtype=np.uint64)
                assert eng.pack_reads(chars, rel, planes.array, other, threads=2) == units
                keep.append((chars, rel, planes, other))
                st.submit_packed(planes.array, other, rel, 14, units)

            got, got_mm, got_counts = [], [], []
            submit(wins[0])
            submit(wins[1])
            for b in range(len(wins)):
                m, boff, tm = st.next()
                x = st.mismatches()
                assert len(x) == len(m) == int(boff[-1])  # the column lines up with the rows of this batch
                if b + 2 < len(wins):
                    submit(wins[b + 2])  # every slot in use
                got.append(triples(m))
                got_mm.append(x)
                got_counts.append(np.diff(boff.astype(np.int64)))
            st.close()
            assert np.array_equal(np.concatenate(got), triples(one))
            assert np.array_equal(np.concatenate(got_mm), one_mm)
            assert np.array_equal(np.concatenate(got_counts), np.diff(one_boff.astype(np.int64)))
    for bad in (dict(mam=True, ext=True), dict(mum=True, ext=True), dict(smem=True, ext=True), dict(chain=True, ext=True),
                dict(penalty=2), dict(xdrop=3), dict(chain=True, xdrop=3), dict(ext=True, max_gap=20), dict(ext=True, max_occ=2),
                dict(ext=True, penalty=-1), dict(ext=True, xdrop=-1), dict(ext=True, penalty=2 ** 32), dict(ext=True, xdrop=2 ** 32 - 1)):
        with pytest.raises(ValueError):
            eng.Stream(idx, 3, 1 << 16, 13, True, **bad)
        with pytest.raises(ValueError):
            idx.find_mems(q, off, 14, True, **bad)
    # set_ext_params: refused on a stream of another match type, and after the first submit; mismatches: only -ext, only after next
    L = capi.lib()
    import ctypes as C
    p = C.POINTER(C.c_uint32)()
    st = eng.Stream(idx, 3, 1 << 16, 13, True, chain=True)
    assert L.slamem_stream_set_ext_params(st._h, 2, 5) == capi.SLAMEM_ERR_ARG
    assert L.slamem_stream_set_ext_params(st._h, 0, 0xFFFFFFFF) == capi.SLAMEM_OK
    assert L.slamem_stream_mismatches(st._h, C.byref(p)) == capi.SLAMEM_ERR_ARG
    st.close()
    st = eng.Stream(idx, 3, 1 << 16, 13, True, ext=True)
    assert L.slamem_stream_set_ext_params(st._h, 2, 5) == capi.SLAMEM_OK
    assert L.slamem_stream_mismatches(st._h, C.byref(p)) == capi.SLAMEM_ERR_ARG  # nothing returned yet
    st.submit(q, off[:14].copy(), 14)
    assert L.slamem_stream_set_ext_params(st._h, 3, 5) == capi.SLAMEM_ERR_ARG
    st.next()
    assert L.slamem_stream_mismatches(st._h, C.byref(p)) == capi.SLAMEM_OK
    st.close()
    idx.close()


def test_capacity_edge_and_no_mismatch_buffer(eng):
    import ctypes as C
    import torch
    from slamem_amd import capi
    from slamem_amd.engine import _ptr, _stream_handle
    ref, q, off = mutated_reads(11)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    rows, boff, mm = idx.find_exts(q, off, 14, True)
    assert len(rows) < len(mem)
    qd = torch.zeros((len(q) + 15) // 8 * 8, dtype=torch.uint8, device=idx.device)
    qd[: len(q)] = torch.from_numpy(q).to(idx.device)
    od = torch.from_numpy(off.view(np.int64)).to(idx.device)
    m = idx.matcher(len(off) - 1, True, (len(rows) + len(mem)) // 2, int(off[-1]), ext=True)
    with pytest.raises(capi.SlamemError) as e:
        m.run(qd, od, 14)
    assert e.value.code == capi.SLAMEM_ERR_CAPACITY
    assert m.last_total == len(mem)
    m2 = idx.matcher(len(off) - 1, True, m.last_total, int(off[-1]), ext=True)
    total = m2.run(qd, od, 14)
    assert total == len(rows)
    got = m2.mems[:total].cpu().numpy().view(np.uint32).reshape(-1, 3).astype(np.int64)
    assert np.array_equal(got, triples(rows))
    assert np.array_equal(m2.block_offsets.cpu().numpy(), boff.astype(np.int64))
    assert np.array_equal(m2.mismatches[:total].cpu().numpy().view(np.uint32), mm)
    # mismatches_dev = NULL: the rows and offsets alone
    m2.mems.zero_()
    tot = C.c_uint64()
    rc = capi.lib().slamem_find_exts_device(idx._h, _ptr(qd), _ptr(od), len(off) - 1, int(off[-1]), 14, 1, 0, 0xFFFFFFFF,
                                           _ptr(m2.mems), m2.capacity, _ptr(m2.block_offsets), None, _ptr(m2.workspace),
                                           m2.workspace.numel(), _stream_handle(idx.device), C.byref(tot))
    assert rc == capi.SLAMEM_OK and tot.value == len(rows)
    assert np.array_equal(m2.mems[:total].cpu().numpy().view(np.uint32).reshape(-1, 3).astype(np.int64), triples(rows))
    idx.close()


def test_compact_index_is_refused_and_still_searches(eng, monkeypatch):
    from slamem_amd import capi
    ref, q, off = mutated_reads(13, count=40)
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    idx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    assert idx.info.layout == capi.LAYOUT_COMPACT
    with pytest.raises(capi.SlamemError) as e:
        idx.find_exts(q, off, 14, True)
    assert e.value.code == capi.SLAMEM_ERR_ARG
    assert "text planes" in str(e.value) and "compact" in str(e.value)
    mem, mem_boff = idx.find_mems(q, off, 14, True)  # the process and the index go on
    full = eng.Index.build(ref)
    mem2, mem_boff2 = full.find_mems(q, off, 14, True)
    assert np.array_equal(triples(mem), triples(mem2)) and np.array_equal(mem_boff, mem_boff2) and len(mem) > 40
    full.close()
    idx.close()


def test_other_modes_unchanged_by_ext_calls(eng):
    ref, q, off = mutated_reads(17)
    idx = eng.Index.build(ref)
    modes = (dict(), dict(mam=True), dict(mum=True), dict(smem=True), dict(chain=True))
    before = [idx.find_mems(q, off, 14, True, **kw) for kw in modes]
    for kw in (dict(), dict(penalty=1, xdrop=3), dict(xdrop=0)):
        idx.find_exts(q, off, 14, True, **kw)
        assert eng.timings()["mum_filter_ms"] > 0
        mid = idx.find_mems(q, off, 14, True)
        assert eng.timings()["mum_filter_ms"] == 0
        assert np.array_equal(triples(mid[0]), triples(before[0][0]))
    after = [idx.find_mems(q, off, 14, True, **kw) for kw in modes]
    for (m0, b0), (m1, b1) in zip(before, after):
        assert np.array_equal(b0, b1)
        assert np.array_equal(triples(m0), triples(m1))
    idx.close()


@pytest.mark.parametrize("args", [["-ext", "-chain"], ["-ext", "-mam", "x"], ["-pen", "3"], ["-ext", "-pen", "0"],
                                  ["-ext", "-pen", "four"], ["-ext", "-xdrop", "wide"]])
def test_cli_refusals(args, tmp_path):
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + args + ["-o", str(out), ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and b"> ERROR: " in r.stdout and not out.exists()


def test_cli_logical_gpus_byte_identical(tmp_path):
    """The N-GPU schedule of the command line (SLAMEM_LOGICAL_GPUS=2: two streams on the one device, batches alternate) passes
    the mode and its parameters to every stream, and every batch's fourth column stays with its rows."""
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
    for name, args, env in (("mem", [], base), ("one", ["-ext", "-pen", "3"], base),
                            ("two", ["-ext", "-pen", "3"], dict(base, SLAMEM_LOGICAL_GPUS="2"))):
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
    for b, (_, rows) in enumerate(blocks[:4000]):  # (the per-letter checker is slow: the first 2,000 reads)
        rec = chars[qs.offsets[b // 2]:qs.offsets[b // 2 + 1]]
        k, m, _ = ext_spec.block_ext(rows, ext_spec.revcomp(rec) if b % 2 else rec, ref.chars, 3, 20)
        exp.append(ext_spec.format_block(qs.names[b // 2], b % 2, k, m, ref))
    exp = b"".join(exp)
    assert outs["one"][:len(exp)] == exp
    assert outs["one"].count(b"\n") < outs["mem"].count(b"\n")
