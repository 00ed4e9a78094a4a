"""-pile on the MI355X (slamem_pileup_*, engine.Pileup, a stream of match type 8): every table is tests/pile_spec.py applied to
map_spec.filter_reads of the complete -mem list of the same engine, compared for exact equality -- on the golden files the real
reference wrote, on -aln's constructed and indel reads, on every tier of the chain, the gap closure and the add kernels, on a
reference of several records with reads on both strands; accumulation across batches, read-out of ranges, reset; the stream and
its refusals; a compact index; the executable's file; and, without the spec, two known answers: the depth and the planted
substitutions of unique reads, and the empty table of duplicated reads above quality 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aln_spec
import ext_spec
import map_spec
import pile_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, opt_value
from test_gpu_aln import batch, tier_batch
from test_gpu_chain import indel_reads
from test_gpu_map import multi_record_batch, rec_rows
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


def spec_results(idx, ref, q, off, min_len, both, G=5000, P=4, X=20, E=31):
    mem, mem_boff = idx.find_mems(q, off, min_len, both)
    return map_spec.filter_reads(mem, mem_boff, ref, q, off, both, G, P, X, E)


def same(got, want):
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.nonzero((got.astype(np.int64) != want).any(axis=1))[0]
    assert len(bad) == 0, "rows %s: got %s, want %s" % (bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())


def piled(eng, idx, q, off, min_len, both, min_mapq=0, **kw):
    p = eng.Pileup(idx)
    recs = p.add(q, off, min_len, both, min_mapq=min_mapq, **kw)
    table = p.counts()
    p.close()
    return table, recs


def halves(q, off):
    h = (len(off) - 1) // 2
    cut = int(off[h])
    return (q[:cut], off[:h + 1].copy()), (q[cut:], (off[h:] - off[h]).astype(np.uint64))


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
        kw = {} if dflt else dict(max_gap=G, penalty=P, xdrop=X, max_edits=E)
        with search_path(path):
            mine = spec_results(idx, text, q, off, min_len, both, G, P, X, E)
            got, recs = piled(eng, idx, q, off, min_len, both, **kw)
        same(got, pile_spec.pile(mine, q, off, len(text)))
        same(got, pile_spec.pile(want, q, off, len(text)))  # ... which is the spec applied to the file the real reference wrote
        assert np.array_equal(rec_rows(recs), map_spec.pack(want)[4])
    idx.close()


def test_constructed_and_indel_reads(eng):
    ref, q, off, _ = aln_spec.constructed_reads(11)
    idx = eng.Index.build(ref)
    want = pile_spec.pile(spec_results(idx, ref, q, off, 20, True), q, off, len(ref))
    assert want[:, 4].sum() > 0 and want[:, 5].sum() > 0 and want[:, :4].sum() > 0
    same(piled(eng, idx, q, off, 20, True)[0], want)
    idx.close()
    ref, q, off = indel_reads(21)
    idx = eng.Index.build(ref)
    res = spec_results(idx, ref, q, off, 14, True)
    want = pile_spec.pile(res, q, off, len(ref))
    assert want[:, 4].sum() > 0 and want[:, 5].sum() > 0
    same(piled(eng, idx, q, off, 14, True)[0], want)
    for min_mapq in (1, 30, 60):
        w = pile_spec.pile(res, q, off, len(ref), min_mapq)
        same(piled(eng, idx, q, off, 14, True, min_mapq=min_mapq)[0], w)
    # (the threshold decides something here: every read meets the repeated element, so none reaches 60)
    assert pile_spec.contributing(res, 60) < pile_spec.contributing(res, 30) <= pile_spec.contributing(res, 0) and pile_spec.contributing(res, 30) > 0
    idx.close()


@pytest.mark.parametrize("path", ["seed", "walk"])
def test_every_tier_in_one_batch(eng, path):
    """Blocks of one row and far above the chain's tile, and segments of one operation and of many: the lane kernel and the wave
    kernel both have work."""
    ref, q, off = tier_batch()
    idx = eng.Index.build(ref)
    with search_path(path):
        res = spec_results(idx, ref, q, off, 14, True)
        got, _ = piled(eng, idx, q, off, 14, True)
    nops = [len(s[5]) for r in res for s in r[4]]
    assert max(nops) > eng.PILE_LANE_OPS and min(nops) == 1 and any(1 < k <= eng.PILE_LANE_OPS for k in nops)
    same(got, pile_spec.pile(res, q, off, len(ref)))
    idx.close()


def test_multi_record_reference_both_strands_and_a_read_with_n(eng):
    ref, q, off = multi_record_batch()
    reads = [q[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]
    rng = np.random.default_rng(3)
    for k, a in enumerate((400, 3500, 9000, 2900)):  # (the last one lies across the separator between two records)
        r = ref[a:a + 180].copy()
        r[60 + 10 * k] = ord("N")
        r[120] = rng.choice(ACGT)
        reads.append(ext_spec.revcomp(r) if k % 2 else r)
    q, off = batch(reads)
    idx = eng.Index.build(ref)
    res = spec_results(idx, ref, q, off, 20, True)
    assert sum(r[0] == 1 for r in res) > 20 and sum(r[0] == 2 for r in res) > 20 and all(r[0] for r in res[-4:-1])
    same(piled(eng, idx, q, off, 20, True)[0], pile_spec.pile(res, q, off, len(ref)))
    idx.close()


# ---- known answers, judged without the spec ------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["seed", "walk"])
def test_unique_reads_depth_and_planted_substitutions(eng, path):
    """200-letter reads with 2 % substitutions from both strands of a 40 kbp random reference.  Where every read that touches a
    position maps whole (one segment, 200 = 200 letters, no indel), the row is known from the construction alone: each read adds
    its own letter -- for a reverse read the complement of the letter as given -- at its place of origin."""
    ref, q, off, truth = map_spec.unique_reads(UNIQUE_SEED)
    idx = eng.Index.build(ref)
    with search_path(path):
        segs, roff, ops, ooff, reads = idx.map_reads(q, off, 20, True)
        got, _ = piled(eng, idx, q, off, 20, True)
    idx.close()
    n = len(ref)
    comp = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
    col = {ord(c): k for k, c in enumerate("ACGT")}
    want = np.zeros((n, 6), dtype=np.int64)
    unsure = np.zeros(n, dtype=bool)
    whole = planted = 0
    for k, (a, strand) in enumerate(truth):
        given = q[int(off[k]):int(off[k + 1])]
        s0, s1 = int(roff[k]), int(roff[k + 1])
        ok = s1 - s0 == 1 and int(segs["ref_pos"][s0]) == a and int(segs["ref_len"][s0]) == 200 and \
            int(segs["query_len"][s0]) == 200 and int(reads["strand"][k]) == strand and \
            all((int(w) & 15) in (7, 8) for w in ops[int(ooff[s0]):int(ooff[s1])])
        if not ok:
            unsure[max(0, a - 200):a + 400] = True
            continue
        whole += 1
        for x in range(200):
            letter = int(given[x]) if strand == 1 else comp[int(given[199 - x])]
            want[a + x, col[letter]] += 1
            planted += letter != int(ref[a + x])
    assert whole >= 120 and planted > 300
    sure = ~unsure
    assert np.array_equal(got[sure].astype(np.int64), want[sure])
    cover = np.zeros(n, dtype=np.int64)
    for a, _ in truth:
        cover[a:a + 200] += 1
    assert np.array_equal(pile_spec.depth(got.astype(np.int64))[sure], cover[sure]) and int(cover[sure].max()) >= 2


def test_duplicated_reads_count_only_at_quality_0(eng):
    ref, q, off = map_spec.duplicated_reads(7)
    idx = eng.Index.build(ref)
    t1, recs = piled(eng, idx, q, off, 20, True, min_mapq=1)
    t0, _ = piled(eng, idx, q, off, 20, True, min_mapq=0)
    idx.close()
    assert bool((recs["mapq"] == 0).all()) and not t1.any()
    assert int(t0.sum()) == 60 * 150 and not t0[:, 4:].any()


# ---- accumulation, read-out, reset ---------------------------------------------------------------------------------------------

def test_accumulation_read_out_and_reset(eng):
    from slamem_amd import capi
    ref, q, off = indel_reads(21)
    n = len(ref)
    idx = eng.Index.build(ref)
    (qa, oa), (qb, ob) = halves(q, off)
    whole, _ = piled(eng, idx, q, off, 14, True)
    assert whole.any()
    p = eng.Pileup(idx)
    assert not p.counts().any()
    p.add(qa, oa, 14, True)
    first = p.counts()  # a read-out between two adds ...
    same(first, pile_spec.pile(spec_results(idx, ref, qa, oa, 14, True), qa, oa, n))
    p.add(qb, ob, 14, True)
    assert np.array_equal(p.counts(), whole)  # ... does not disturb the final table
    assert np.array_equal(p.counts(), whole)
    # ranges that start and end inside 64-letter units, inside one read-out tile and across several
    for a, k in ((2000 + 37, 4000 + 101), (5, 50), (2047, 2), (2048, 2048), (4100, 1), (n - 70, 70), (n, 0), (0, 0)):
        assert np.array_equal(p.counts(a, k), whole[a:a + k]), (a, k)
    for a, k in ((n + 1, 0), (n - 3, 4), (0, n + 1)):
        with pytest.raises(capi.SlamemError) as e:
            p.counts(a, k)
        assert e.value.code == capi.SLAMEM_ERR_ARG
    p.reset()
    assert not p.counts().any()
    p.add(qb, ob, 14, True)  # the halves in the other order
    p.add(qa, oa, 14, True)
    assert np.array_equal(p.counts(), whole)
    # the C calls: the host read-out, and a quality above 60
    out = np.zeros((300, 6), dtype=np.uint32)
    L = capi.lib()
    assert L.slamem_pileup_counts_host(p._h, 1990, 300, out.ctypes.data) == capi.SLAMEM_OK
    assert np.array_equal(out, whole[1990:2290])
    assert L.slamem_pileup_counts_host(p._h, n - 1, 2, out.ctypes.data) == capi.SLAMEM_ERR_ARG
    dummy = out.ctypes.data
    assert L.slamem_pileup_add_device(p._h, dummy, dummy, 0, dummy, dummy, dummy, dummy, dummy, 61, None) == capi.SLAMEM_ERR_ARG
    with pytest.raises(ValueError):
        p.add(qa, oa, 14, True, min_mapq=61)
    assert np.array_equal(p.counts(), whole)
    p.close()
    idx.close()


# ---- the stream ----------------------------------------------------------------------------------------------------------------

def windows(off, per):
    nq = len(off) - 1
    return [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]


def run_stream(eng, idx, pile, q, wins, slots, min_mapq=0, **kw):
    st = eng.Stream(idx, slots, 1 << 16, len(wins[0]) - 1, True, pile=pile, min_mapq=min_mapq, **kw)
    totals, recs = [], []
    for b in range(min(slots - 1, len(wins))):
        st.submit(q, wins[b], 14)
    for b in range(len(wins)):
        total, nothing, tm = st.next()
        assert nothing is None
        totals.append(total)
        recs.append(rec_rows(st.maps()))
        if b + slots - 1 < len(wins):
            st.submit(q, wins[b + slots - 1], 14)
    st.close()
    return totals, np.concatenate(recs)


def test_stream_equals_direct_calls(eng):
    ref, q, off = indel_reads(7)
    idx = eng.Index.build(ref)
    per = (len(off) - 1 + 2) // 3
    wins = windows(off, per)
    assert len(wins) == 3
    for min_mapq, kw in ((0, dict()), (20, dict(max_gap=100, penalty=2, xdrop=7, max_edits=2))):
        direct, recs = piled(eng, idx, q, off, 14, True, min_mapq=min_mapq, **kw)
        segs, roff = idx.map_reads(q, off, 14, True, **kw)[:2]
        p = eng.Pileup(idx)
        totals, got_recs = run_stream(eng, idx, p, q, wins, 2, min_mapq, **kw)
        assert np.array_equal(p.counts(), direct) and direct.any()
        assert np.array_equal(got_recs, rec_rows(recs))
        assert totals == [int(roff[min(len(off) - 1, (b + 1) * per)]) - int(roff[b * per]) for b in range(3)] and sum(totals) == len(segs)
        # a second stream into the same accumulator: the sum
        run_stream(eng, idx, p, q, wins, 3, min_mapq, **kw)
        assert np.array_equal(p.counts().astype(np.int64), 2 * direct.astype(np.int64))
        p.close()
    idx.close()


def test_two_streams_share_one_pileup_at_the_same_time(eng):
    ref, q, off = indel_reads(7)
    idx = eng.Index.build(ref)
    direct, _ = piled(eng, idx, q, off, 14, True)
    wins = windows(off, 40)
    p = eng.Pileup(idx)
    a = eng.Stream(idx, 3, 1 << 16, 40, True, pile=p)
    b = eng.Stream(idx, 3, 1 << 16, 40, True, pile=p)
    for w in wins:  # (batch after batch, both streams busy on each)
        a.submit(q, w, 14)
        b.submit(q, w, 14)
        a.next()
        b.next()
    a.close()
    b.close()
    assert np.array_equal(p.counts().astype(np.int64), 2 * direct.astype(np.int64))
    p.close()
    idx.close()


def test_stream_refusals(eng):
    import torch
    from slamem_amd import capi
    ref, q, off = indel_reads(7)
    idx = eng.Index.build(ref)
    L = capi.lib()
    p = eng.Pileup(idx)
    ARG = capi.SLAMEM_ERR_ARG

    def raw(match_type):
        h = C.c_void_p()
        assert L.slamem_stream_create(idx._h, 2, 1 << 16, 64, 1, match_type, C.byref(h)) == capi.SLAMEM_OK
        return h
    offs = np.ascontiguousarray(off[:9])
    # without an accumulator: no submit
    h = raw(8)
    assert L.slamem_stream_submit(h, q.ctypes.data, offs.ctypes.data, 8, 14) == ARG
    assert b"slamem_stream_set_pileup" in L.slamem_last_error_message()
    assert L.slamem_stream_set_pileup(h, p._h, 61) == ARG and L.slamem_stream_set_pileup(h, None, 0) == ARG
    assert L.slamem_stream_set_pileup(h, p._h, 60) == capi.SLAMEM_OK
    for setter, args in ((L.slamem_stream_set_max_gap, (100,)), (L.slamem_stream_set_ext_params, (2, 7)), (L.slamem_stream_set_max_edits, (2,))):
        assert setter(h, *args) == capi.SLAMEM_OK  # every setter of -paf
    assert L.slamem_stream_submit(h, q.ctypes.data, offs.ctypes.data, 8, 14) == capi.SLAMEM_OK
    assert L.slamem_stream_set_pileup(h, p._h, 0) == ARG  # after the first submit
    mems, boff, total, nq = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
    assert L.slamem_stream_next(h, C.byref(mems), C.byref(boff), C.byref(total), C.byref(nq), None) == capi.SLAMEM_OK and nq.value == 8
    a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert L.slamem_stream_alns(h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == ARG
    assert L.slamem_stream_maps(h, C.byref(a)) == capi.SLAMEM_OK and a.value
    assert L.slamem_stream_destroy(h) == capi.SLAMEM_OK
    # on another match type
    for mt in (0, 6, 7):
        h = raw(mt)
        assert L.slamem_stream_set_pileup(h, p._h, 0) == ARG
        assert L.slamem_stream_destroy(h) == capi.SLAMEM_OK
    h = C.c_void_p()
    assert L.slamem_stream_create(idx._h, 2, 1 << 16, 64, 1, 9, C.byref(h)) == ARG
    for bad in (dict(paf=True), dict(aln=True), dict(chain=True), dict(mam=True)):
        with pytest.raises((ValueError, capi.SlamemError)):
            eng.Stream(idx, 3, 1 << 16, 13, True, pile=p, **bad)
    with pytest.raises(ValueError):
        eng.Stream(idx, 3, 1 << 16, 13, True, paf=True, min_mapq=3)
    if torch.cuda.device_count() > 1:  # an accumulator of another device
        other = eng.Index.build(ref, "cuda:1")
        p1 = eng.Pileup(other)
        h = raw(8)
        assert L.slamem_stream_set_pileup(h, p1._h, 0) == ARG
        assert L.slamem_stream_destroy(h) == capi.SLAMEM_OK
        p1.close()
        other.close()
    p.close()
    idx.close()


def test_compact_index_is_refused(eng, monkeypatch):
    from slamem_amd import capi
    ref, q, off = indel_reads(13)
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    idx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    assert idx.info.layout == capi.LAYOUT_COMPACT
    with pytest.raises(capi.SlamemError) as e:
        eng.Pileup(idx)
    assert e.value.code == capi.SLAMEM_ERR_ARG
    assert "text planes" in str(e.value) and "compact" in str(e.value) and "-pile" in str(e.value)
    mem, _ = idx.find_mems(q, off, 14, True)  # the process and the index go on
    assert len(mem) > 40
    idx.close()


# ---- the executable ------------------------------------------------------------------------------------------------------------

def write_fasta(path, records):
    with open(path, "wb") as f:
        for name, letters in records:
            f.write(b">" + name + b"\n")
            for a in range(0, len(letters), 70):
                f.write(bytes(letters[a:a + 70]) + b"\n")


def test_cli_file_is_the_engines_table(eng, tmp_path):
    """slaMEM-hip -b -l 20 -pile -minq 1 ref.fa reads.fa: byte for byte the file pile_spec formats from the engine's table, on a
    reference of three records (names with blanks, the separators skipped), reads on both strands; with two logical GPUs (an
    accumulator each, added up when the file is written) the same bytes."""
    import hostlib
    ref, q, off = multi_record_batch()
    recs = [ref[:3000], ref[3001:8001], ref[8002:]]
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"one first", recs[0]), (b"two\tsecond", recs[1]), (b"three", recs[2])])
    write_fasta(q_fa, [(b"read%d x" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(ref)
    idx = eng.Index.build(ref)
    table, recs_ = piled(eng, idx, q, off, 20, True, min_mapq=1)
    zero, _ = piled(eng, idx, q, off, 20, True, min_mapq=0)
    idx.close()
    want = pile_spec.pile_file(table.astype(np.int64), loaded)
    assert want.count(b"\n") > 5000 and want != pile_spec.pile_file(zero.astype(np.int64), loaded)
    assert {l.split(b"\t")[0] for l in want.split(b"\n")[:-1]} == {b"one", b"two", b"three"}
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for name, env in (("one", base), ("two", dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1"))):
        out = str(tmp_path / (name + ".txt"))
        r = subprocess.run([EXE, "-b", "-l", "20", "-pile", "-minq", "1", "-o", out, ref_fa, q_fa], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, env=env, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        got = open(out, "rb").read()
        assert got == want and b">" not in got
        assert b"Saving pileups" in r.stdout and b"minimum pileup length = 20" in r.stdout
        assert b"; maximum edits = 31 ; minimum mapping quality = 1\n" in r.stdout
    # the default name, as -paf names it
    r = subprocess.run([EXE, "-pile", "-b", ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=base, timeout=300)
    assert r.returncode == 0
    assert open(str(tmp_path / "ref-mems.txt"), "rb").read() == pile_spec.pile_file(zero.astype(np.int64), loaded)


@pytest.mark.parametrize("args,message", [
    (["-pile", "-paf"], b"Option -pile excludes -mam, -mum, -smem, -chain, -ext, -aln and -paf"),
    (["-chain", "-pile"], b"Option -pile excludes -mam, -mum, -smem, -chain, -ext, -aln and -paf"),
    (["-minq", "5"], b"Option -minq needs -pile"),
    (["-paf", "-minq", "5"], b"Option -minq needs -pile"),
    (["-pile", "-minq", "61"], b"Option -minq needs a whole number from 0 to 60"),
    (["-pile", "-minq", "x"], b"Option -minq needs a whole number from 0 to 60"),
])
def test_cli_clashes_exit_before_any_gpu_work(args, message, tmp_path):
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"r", b"ACGT" * 30)])
    write_fasta(q_fa, [(b"q", b"ACGT" * 10)])
    r = subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))  # (no device: it never asks for one)
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout
    assert not os.path.exists(str(tmp_path / "ref-mems.txt"))
