"""-paf on the MI355X (slamem_find_maps_device, Index.map_reads): every result is tests/map_spec.py applied to the complete -mem
list of the same engine -- segments, read offsets, operations and the read records (strand, mapq, s1, s2) -- on the golden files
the real reference wrote, on -aln's constructed and indel reads, on every tier of the chain and of the gap closure, on a
reference of several records with reads on both strands, on reads without a match, at the capacity edges; the stream, the host
call and the executable's PAF file; and, without the spec, two known answers: unique reads map to their origin with quality
60, reads from a duplicated region get quality 0."""
import os
import subprocess

import numpy as np
import pytest

import aln_spec
import ext_spec
import map_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, opt_value
from test_gpu_aln import batch, seg_rows, tier_batch
from test_gpu_chain import indel_reads
from test_map_host import UNIQUE_SEED

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


def rec_rows(reads):
    return np.stack([reads[k] for k in ("strand", "mapq", "s1", "s2")], axis=1).astype(np.int64) if len(reads) else \
        np.zeros((0, 4), np.int64)


def assert_equals_reads(got, want):
    segs, roff, ops, ooff, reads = got
    w_segs, w_roff, w_ops, w_ooff, w_reads = map_spec.pack(want)
    assert np.array_equal(rec_rows(reads), w_reads)
    assert np.array_equal(np.asarray(roff, dtype=np.int64), w_roff)
    assert np.array_equal(seg_rows(segs), w_segs)
    assert np.array_equal(np.asarray(ooff, dtype=np.int64), w_ooff)
    assert np.array_equal(np.asarray(ops, dtype=np.uint32), w_ops)


def assert_is_map_of(got, mem, mem_boff, ref, q, off, both, G=5000, P=4, X=20, E=31):
    want = map_spec.filter_reads(mem, mem_boff, ref, q, off, both, G, P, X, E)
    assert_equals_reads(got, want)
    return want


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_engine(eng, case, path):
    idx = None
    for G, P, X, E in ((5000, 4, 20, 31), (200, 1, 5, 3)):
        want, _, ref, qs, opts = map_spec.golden_map(case, G, P, X, E)
        text = np.frombuffer(ref.chars, dtype=np.uint8).copy()
        if idx is None:
            idx = eng.Index.build(text)
        q = np.frombuffer(qs.chars, dtype=np.uint8)
        off = np.array(qs.offsets, dtype=np.uint64)
        min_len, both = int(opt_value(opts, "-l", 20)), "-b" in opts
        dflt = (G, P, X, E) == (5000, 4, 20, 31)
        with search_path(path):
            mem, mem_boff = idx.find_mems(q, off, min_len, both)
            got = idx.map_reads(q, off, min_len, both, max_gap=0 if dflt else G, penalty=0 if dflt else P,
                                xdrop=None if dflt else X, max_edits=None if dflt else E)
        assert eng.timings()["mum_filter_ms"] > 0
        assert_is_map_of(got, mem, mem_boff, text, q, off, both, G, P, X, E)
        assert_equals_reads(got, want)  # ... which is the spec applied to the file the real reference wrote
    idx.close()


def test_constructed_and_indel_reads(eng):
    ref, q, off, truth = aln_spec.constructed_reads(11)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 20, True)
    got = idx.map_reads(q, off, 20, True)
    assert_is_map_of(got, mem, mem_boff, ref, q, off, True)
    segs, roff, ops, ooff, reads = got
    rows = seg_rows(segs)
    for k, (b, seg, rl) in enumerate(truth):  # (no spec: the strand and the CIGAR written down from the construction)
        s, e = int(roff[k]), int(roff[k + 1])
        assert e - s == 1 and tuple(rows[s]) == seg and int(reads["strand"][k]) == 1 + b % 2
        assert [(aln_spec.CODE_OP[int(w) & 15], int(w) >> 4) for w in ops[int(ooff[s]):int(ooff[s + 1])]] == rl
    idx.close()
    ref, q, off = indel_reads(21)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    for G in (5000, 100):
        want = assert_is_map_of(idx.map_reads(q, off, 14, True, max_gap=G), mem, mem_boff, ref, q, off, True, G=G)
        assert sum(any(c in "ID" for s in w[4] for c, _ in s[5]) for w in want) > 30
    for both in (False,):  # the forward block alone: the competitor is the rest of the block
        mem, mem_boff = idx.find_mems(q, off, 14, both)
        assert_is_map_of(idx.map_reads(q, off, 14, both), mem, mem_boff, ref, q, off, both)
    idx.close()


@pytest.mark.parametrize("path", ["seed", "walk"])
def test_every_tier_in_one_batch(eng, path):
    """Lane and wave chains (blocks of one row, of a few, and far above the chain's LDS tile) in the first AND the second chain
    pass, inline and wave gaps, breaks, an exact read and a read of N."""
    ref, q, off = tier_batch()
    idx = eng.Index.build(ref)
    with search_path(path):
        mem, mem_boff = idx.find_mems(q, off, 14, True)
        got = idx.map_reads(q, off, 14, True)
    want = assert_is_map_of(got, mem, mem_boff, ref, q, off, True)
    sizes = np.diff(np.asarray(mem_boff, dtype=np.int64))
    assert sizes.max() > 1024 and (sizes == 1).any() and ((sizes > 1) & (sizes <= 32)).any()
    big = int(np.argmax(sizes)) // 2
    assert want[big][3] > 0 and len(want[big][4]) >= 1  # (the large block's read has a competing chain)
    assert want[-1] == (0, 0, 0, 0, []) and any(len(w[4]) > 1 for w in want)
    idx.close()


def multi_record_batch(seed=5):
    """Three records, one of them holding a verbatim copy of a piece of another; reads with substitutions from both strands of
    every record, reads from the copied piece, two reads that match nothing."""
    rng = np.random.default_rng(seed)
    recs = [rng.choice(ACGT, size=n) for n in (3000, 5000, 4000)]
    recs[2][1000:1600] = recs[0][500:1100]
    ref = np.concatenate([recs[0], [ord("N")], recs[1], [ord("N")], recs[2]]).astype(np.uint8)
    reads = []
    for k in range(60):
        a = int(rng.integers(0, len(ref) - 200))
        r = ref[a:a + 180].copy()
        for x in rng.integers(0, 180, size=4):
            r[int(x)] = rng.choice(ACGT)
        reads.append(ext_spec.revcomp(r) if k % 2 else r)
    for k in range(10):
        a = 520 + 40 * k
        r = recs[0][a:a + 150].copy()
        reads.append(ext_spec.revcomp(r) if k % 2 else r)
    reads.append(np.frombuffer(b"N" * 90, dtype=np.uint8).copy())
    reads.append(np.frombuffer(b"ACGT" * 3, dtype=np.uint8).copy())  # shorter than the minimum length
    q, off = batch(reads)
    return ref, q, off


def test_multi_record_reference_both_strands_and_unmapped_reads(eng):
    ref, q, off = multi_record_batch()
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 20, True)
    got = idx.map_reads(q, off, 20, True)
    want = assert_is_map_of(got, mem, mem_boff, ref, q, off, True)
    reads = got[4]
    assert (reads["strand"] == 1).sum() > 20 and (reads["strand"] == 2).sum() > 20
    assert list(reads["strand"][-2:]) == [0, 0] and list(reads["mapq"][-2:]) == [0, 0] and int(got[1][-1]) == int(got[1][-3])
    assert all(w[1] == 0 and w[2] == w[3] for w in want[60:70])  # the copied piece
    # a batch in which no read matches at all
    q2, off2 = batch([np.frombuffer(b"N" * 50, dtype=np.uint8).copy(), np.frombuffer(b"ACGTAC", dtype=np.uint8).copy()])
    segs, roff, ops, ooff, reads = idx.map_reads(q2, off2, 20, True)
    assert len(segs) == 0 and len(ops) == 0 and list(roff) == [0, 0, 0] and list(ooff) == [0]
    assert rec_rows(reads).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]
    idx.close()


def test_both_capacity_edges(eng):
    from slamem_amd import capi
    ref, q, off = indel_reads(11)
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, 14, True)
    segs, roff, ops, ooff, reads = idx.map_reads(q, off, 14, True)
    want = (len(mem), len(segs), len(ops))
    assert len(segs) > 50 and len(ops) > len(segs)
    for caps in ((len(mem) - 1, len(segs), len(ops)), (len(mem), len(segs) - 1, len(ops)), (len(mem), len(segs), len(ops) - 1)):
        with pytest.raises(capi.SlamemError) as e:
            idx.map_reads(q, off, 14, True, capacities=caps)
        assert e.value.code == capi.SLAMEM_ERR_CAPACITY
        if caps[0] == len(mem):
            assert e.value.totals == want
        else:
            assert e.value.totals[0] >= len(mem) and e.value.totals[1:] == (0, 0)
    got = idx.map_reads(q, off, 14, True, capacities=want)  # exactly enough
    for a, b in zip(got, (segs, roff, ops, ooff, reads)):
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
        idx.map_reads(q, off, 14, True)
    assert e.value.code == capi.SLAMEM_ERR_ARG
    assert "text planes" in str(e.value) and "compact" in str(e.value) and "-paf" in str(e.value)
    mem, _ = idx.find_mems(q, off, 14, True)  # the process and the index go on
    assert len(mem) > 40
    idx.close()


def test_other_modes_unchanged_by_paf_calls(eng):
    ref, q, off = indel_reads(13)
    idx = eng.Index.build(ref)

    def others():
        return (idx.find_mems(q, off, 14, True), idx.find_chains(q, off, 14, True), idx.find_exts(q, off, 14, True),
                idx.find_alns(q, off, 14, True))
    before = others()
    first = idx.map_reads(q, off, 14, True)
    after = others()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(a, b)
    for a, b in zip(first, idx.map_reads(q, off, 14, True)):
        assert np.array_equal(a, b)
    idx.close()


def test_stream_equals_one_shot(eng):
    from slamem_amd import capi
    ref, q, off = indel_reads(7)
    idx = eng.Index.build(ref)
    for kw in (dict(), dict(max_gap=100, penalty=2, xdrop=7, max_edits=2)):
        segs, roff, ops, ooff, reads = idx.map_reads(q, off, 14, True, **kw)
        per = 13
        nq = len(off) - 1
        wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
        st = eng.Stream(idx, 3, 1 << 16, per, True, paf=True, **kw)
        g_segs, g_counts, g_ops, g_nops, g_reads = [], [], [], [], []
        st.submit(q, wins[0], 14)
        st.submit(q, wins[1], 14)
        for b in range(len(wins)):
            m, ro, tm = st.next()
            o, oo = st.alns()
            assert len(ro) == len(wins[b]) and len(m) == int(ro[-1]) == len(oo) - 1 and int(oo[-1]) == len(o)
            g_reads.append(rec_rows(st.maps()))
            if b + 2 < len(wins):
                st.submit(q, wins[b + 2], 14)  # every slot in use
            g_segs.append(seg_rows(m))
            g_counts.append(np.diff(ro.astype(np.int64)))
            g_ops.append(o)
            g_nops.append(np.diff(oo.astype(np.int64)))
        st.close()
        assert np.array_equal(np.concatenate(g_reads), rec_rows(reads))
        assert np.array_equal(np.concatenate(g_segs), seg_rows(segs))
        assert np.array_equal(np.concatenate(g_counts), np.diff(roff.astype(np.int64)))
        assert np.array_equal(np.concatenate(g_ops), ops)
        assert np.array_equal(np.concatenate(g_nops), np.diff(ooff.astype(np.int64)))
    for bad in (dict(paf=True, chain=True), dict(paf=True, aln=True), dict(paf=True, mam=True)):
        with pytest.raises((ValueError, capi.SlamemError)):
            eng.Stream(idx, 3, 1 << 16, 13, True, **bad)
    idx.close()


def test_host_convenience_call(eng):
    import ctypes as C
    from slamem_amd import capi
    ref, q, off = indel_reads(17)
    idx = eng.Index.build(ref)
    want = idx.map_reads(q, off, 14, True, max_edits=5)
    L = capi.lib()
    segs, roff, ops, ooff, recs = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    totals = (C.c_uint64 * 3)()
    qb = np.ascontiguousarray(q).tobytes()
    offs = np.ascontiguousarray(off, dtype=np.uint64)
    rc = L.slamem_find_maps_host(idx._h, qb, offs.ctypes.data, len(offs) - 1, 14, 1, 0, 0, 0xFFFFFFFF, 5, C.byref(segs), C.byref(roff),
                                 C.byref(ops), C.byref(ooff), C.byref(recs), totals)
    assert rc == capi.SLAMEM_OK, L.slamem_last_error_message()
    nseg, nops, nq = int(totals[1]), int(totals[2]), len(offs) - 1
    assert (nseg, nops) == (len(want[0]), len(want[2]))
    got_segs = np.ctypeslib.as_array((C.c_uint32 * (5 * max(nseg, 1))).from_address(segs.value))[: 5 * nseg].reshape(-1, 5)
    assert np.array_equal(got_segs.astype(np.int64), seg_rows(want[0]))
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint64 * (nq + 1)).from_address(roff.value)), want[1])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint32 * max(nops, 1)).from_address(ops.value))[:nops], want[2])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint64 * (nseg + 1)).from_address(ooff.value)), want[3])
    raw = np.ctypeslib.as_array((C.c_uint32 * (3 * nq)).from_address(recs.value)).reshape(-1, 3)
    assert np.array_equal(raw[:, 0], want[4]["s1"]) and np.array_equal(raw[:, 1], want[4]["s2"])
    assert np.array_equal(raw[:, 2] & 0xFF, want[4]["strand"]) and np.array_equal((raw[:, 2] >> 8) & 0xFF, want[4]["mapq"])
    assert not (raw[:, 2] >> 16).any()
    for p in (segs, roff, ops, ooff, recs):
        L.slamem_host_free(p)
    idx.close()


# ---- known answers, judged without the spec ------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["seed", "walk"])
def test_unique_reads_map_to_their_origin_with_quality_60(eng, path):
    """200-letter reads with 2 % substitutions from both strands of a 40 kbp uniform random reference, -l 20: the origin, the
    strand, and mapq 60 for at least 95 % (a chance 20-mer elsewhere has probability about 1e-5 per read;
    test_map_host.test_unique_reads_spec_meets_the_cap confirms the cap for this seed on the definition alone)."""
    ref, q, off, truth = map_spec.unique_reads(UNIQUE_SEED)
    idx = eng.Index.build(ref)
    with search_path(path):
        segs, roff, ops, ooff, reads = idx.map_reads(q, off, 20, True)
    idx.close()
    rows = seg_rows(segs)
    for k, (a, strand) in enumerate(truth):
        assert int(reads["strand"][k]) == strand and int(roff[k + 1]) > int(roff[k])
        for p, _, rlen, _, _ in rows[int(roff[k]):int(roff[k + 1])]:
            assert a - 200 <= p and p + rlen <= a + 200 + 200  # [ts, te) within the sampled interval widened by the read's length
    assert len(truth) == 200 and int((reads["mapq"] == 60).sum()) >= 0.95 * len(truth)
    assert bool((reads["s2"] <= reads["s1"]).all()) and bool(((reads["mapq"] == 60) == (reads["s2"] == 0)).all())


def test_duplicated_reads_get_quality_0(eng):
    """Exact reads from a region that is copied verbatim elsewhere on the same strand, lying wholly inside the copy."""
    ref, q, off = map_spec.duplicated_reads(7)
    idx = eng.Index.build(ref)
    segs, roff, ops, ooff, reads = idx.map_reads(q, off, 20, True)
    idx.close()
    assert len(reads) == 60 and bool((reads["s2"] == reads["s1"]).all()) and bool((reads["mapq"] == 0).all())
    assert bool((reads["s1"] == 150).all()) and bool((reads["strand"] == 1).all()) and list(np.diff(roff.astype(np.int64))) == [1] * 60


# ---- the executable ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [(5000, 4, 20, 31), (200, 1, 5, 3)], ids=["defaults", "mgap200-pen1-xdrop5-maxed3"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_cli(case, params, tmp_path):
    """The executable's file, byte for byte: the spec's results formatted by the spec's PAF writer."""
    G, P, X, E = params
    expected = map_spec.golden_paf_file(case, G, P, X, E)
    ref_fa, q_fa, _, _ = case_paths(case)
    out = tmp_path / "out.paf"
    opts = MANIFEST[case]["opts"]
    if params == (5000, 4, 20, 31):  # -paf takes no value, so it may stand anywhere
        argv = [EXE] + opts + ["-o", str(out), ref_fa, "-paf", q_fa]
    else:
        argv = [EXE, "-paf", "-maxed", str(E), "-pen", str(P)] + opts + ["-o", str(out), ref_fa, q_fa, "-xdrop", str(X), "-mgap", str(G)]
    r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    assert out.read_bytes() == expected
    assert b"Saving mappings" in r.stdout and b">" not in out.read_bytes()
    assert (b"; maximum gap = %d ; mismatch penalty = %d ; X-drop = %d ; maximum edits = %d\n" % (G, P, X, E)) in r.stdout


def test_cli_logical_gpus_byte_identical(tmp_path):
    """The N-GPU schedule of the command line (SLAMEM_LOGICAL_GPUS=2: two streams on the one device, batches alternate) passes
    the mode and its parameters to every stream, and every batch's read records stay with its segments."""
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
    for name, args, env in (("mem", [], base), ("one", ["-paf", "-maxed", "2"], base),
                            ("two", ["-paf", "-maxed", "2"], dict(base, SLAMEM_LOGICAL_GPUS="2"))):
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
    T = ext_spec._letters(ref.chars)
    exp = []
    for i in range(2000):  # (the checker is slow: the first 2,000 reads)
        read = qs.chars[qs.offsets[i]:qs.offsets[i + 1]]
        res = map_spec.read_map([blocks[2 * i][1].astype(np.int64), blocks[2 * i + 1][1].astype(np.int64)], read, T, E=2)
        exp.append(map_spec.paf_lines(qs.names[i], qs.sizes[i], res, ref))
    exp = b"".join(exp)
    assert outs["one"][:len(exp)] == exp and exp.count(b"\t-\t") > 500 and exp.count(b"\t+\t") > 500
