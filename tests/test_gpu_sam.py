"""-sam on the MI355X (slamem_maps_md_device, Index.map_reads(md=True), the stream's MD pass, the executable's SAM file): the MD
entries, their offsets, the letters under = and the primary segments are tests/sam_spec.py applied to the spec's mapping of the
engine's own -mem list, exactly; segments designed for the edges of the lane and the wave kernel; the capacity edge; the compact
layout; and every file through the replay checker, which knows nothing of the implementation."""
import os
import subprocess
import sys

import numpy as np
import pytest

import aln_spec
import ext_spec
import hostlib
import map_spec
import sam_spec
from conftest import search_path
from golden_cases import CASES, MANIFEST, case_paths, opt_value
from test_gpu_aln import batch, seg_rows
from test_gpu_chain import indel_reads
from test_gpu_map import assert_equals_reads, multi_record_batch, rec_rows

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


def assert_md_equals(got, want, T):
    """got: map_reads(md=True); want: read_map tuples."""
    assert_equals_reads(got[:5], want)
    md, moff, eq, prim = sam_spec.pack_md(want, T)
    assert np.array_equal(np.asarray(got[6], dtype=np.int64), moff)
    assert np.array_equal(np.asarray(got[5], dtype=np.uint32), md)
    assert np.array_equal(np.asarray(got[7], dtype=np.uint32), eq)
    assert np.array_equal(np.asarray(got[8], dtype=np.uint32), prim)


def check(eng, idx, ref, q, off, min_len, both, **kw):
    mem, mem_boff = idx.find_mems(q, off, min_len, both)
    got = idx.map_reads(q, off, min_len, both, md=True, **kw)
    want = map_spec.filter_reads(mem, mem_boff, ref, q, off, both, kw.get("max_gap") or 5000, 4, 20, 31)
    assert_md_equals(got, want, ext_spec._letters(ref))
    return got, want


def seg_ops(got):
    """[(code letter, length)] per segment of an engine result"""
    ops, ooff = got[2], got[3]
    return [[(aln_spec.CODE_OP[int(w) & 15], int(w) >> 4) for w in ops[int(ooff[s]):int(ooff[s + 1])]] for s in range(len(ooff) - 1)]


def results_of(got):
    """read_map-like tuples (strand, mapq, s1, s2, segments) of an engine result, for the replay checker"""
    segs, roff, reads, per = seg_rows(got[0]), got[1], got[4], seg_ops(got)
    return [(int(reads["strand"][r]), int(reads["mapq"][r]), int(reads["s1"][r]), int(reads["s2"][r]),
             [tuple(int(v) for v in segs[s]) + (per[s],) for s in range(int(roff[r]), int(roff[r + 1]))]) for r in range(len(reads))]


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_engine(eng, case, path):
    want, _, ref, qs, opts = map_spec.golden_map(case)
    text = np.frombuffer(ref.chars, dtype=np.uint8).copy()
    idx = eng.Index.build(text)
    q = np.frombuffer(qs.chars, dtype=np.uint8)
    off = np.array(qs.offsets, dtype=np.uint64)
    with search_path(path):
        got = idx.map_reads(q, off, int(opt_value(opts, "-l", 20)), "-b" in opts, md=True)
    assert_md_equals(got, want, ref.chars)  # (the spec applied to the file the real reference wrote)
    for s in range(len(got[0])):  # the engine's md_text is the spec's
        e = got[5][int(got[6][s]):int(got[6][s + 1])]
        assert eng.md_text(e) == sam_spec.md_text(e) and sam_spec.MD_RE.match(eng.md_text(e))
    idx.close()


def test_constructed_indel_unique_and_duplicated_reads(eng):
    ref, q, off, _ = aln_spec.constructed_reads(11)
    idx = eng.Index.build(ref)
    got, _ = check(eng, idx, ref, q, off, 20, True)
    assert len(got[5]) > len(got[0])
    idx.close()
    ref, q, off = indel_reads(21)
    idx = eng.Index.build(ref)
    for both, G in ((True, 0), (True, 100), (False, 0)):
        got, want = check(eng, idx, ref, q, off, 14, both, max_gap=G)
    assert sum(1 for e in got[5] if e & 4) > 20  # (entries under D)
    idx.close()
    ref, q, off, _ = map_spec.unique_reads(5, count=80)
    idx = eng.Index.build(ref)
    check(eng, idx, ref, q, off, 20, True)
    idx.close()
    ref, q, off = map_spec.duplicated_reads(7, count=20)
    idx = eng.Index.build(ref)
    got, _ = check(eng, idx, ref, q, off, 20, True)
    assert list(got[8]) == [0] * 20 and list(got[5]) == [150 << 4 | 8] * 20
    idx.close()


def designed_batch(seed=3):
    """Reads cut from a random reference with substitutions 20 letters apart (an operation pair `X =` each) and, where asked,
    one event in front of the read's last stretch: `dx` a deleted reference letter directly followed by a substituted one, `ins`
    two inserted letters, `del` two deleted reference letters, `x3` three substituted letters in a row; two more substitutions follow an event.  k
    substitutions alone give 2k + 1 operations, with `dx` 2k + 8."""
    rng = np.random.default_rng(seed)
    ref = rng.choice(ACGT, size=60000)
    other = {int(a): int(b) for a, b in zip(b"ACGT", b"CGTA")}
    plans = [(0, None), (1, None), (14, None), (15, None), (16, None), (12, "dx"), (11, "dx"), (13, "dx"), (31, None), (32, None),
             (28, "dx"), (27, "dx"), (29, "dx"), (64, None), (60, "dx"), (59, "dx"), (61, "dx"), (31, "ins"), (31, "del"),
             (30, "ins"), (30, "del"), (3, "x3"), (40, "x3"), (70, "dx")]
    reads = []
    for n, (k, ev) in enumerate(plans):
        a = 500 + 2400 * n
        p = a + 30  # the next reference letter to copy
        r = [ref[a:p]]
        for _ in range(k):
            r.append(np.array([other[int(ref[p])]], dtype=np.uint8))
            r.append(ref[p + 1:p + 20])
            p += 20
        if ev == "dx":
            r.append(np.array([[c for c in ACGT if c != ref[p] and c != ref[p + 1]][0]], dtype=np.uint8))  # (so that two edits are needed)
            p += 2
        elif ev == "ins":
            r.append(np.array([other[int(ref[p])], other[int(ref[p - 1])]], dtype=np.uint8))
        elif ev == "del":
            p += 2
        elif ev == "x3":
            r.append(np.array([other[int(ref[p + j])] for j in range(3)], dtype=np.uint8))
            p += 3
        if ev:
            for _ in range(2):
                r.append(ref[p:p + 19])
                r.append(np.array([other[int(ref[p + 19])]], dtype=np.uint8))
                p += 20
        r.append(ref[p:p + 30])
        read = np.concatenate(r)
        reads.append(ext_spec.revcomp(read) if n % 3 == 1 else read)
    q, off = batch(reads)
    return ref, q, off


def test_designed_segments_at_the_kernels_edges(eng):
    T = eng.SAM_LANE_OPS
    ref, q, off = designed_batch()
    idx = eng.Index.build(ref)
    got, want = check(eng, idx, ref, q, off, 14, True)
    idx.close()
    per = seg_ops(got)
    counts = {len(o) for o in per}
    assert {1, T - 1, T, T + 1, 63, 64, 65, 128, 129} <= counts, sorted(counts)
    assert any(len(o) > 64 and o[63][0] == "I" and o[62][0] == "=" and o[64][0] == "=" for o in per)  # m carried over a trip's end across I
    assert any(len(o) > 64 and o[63][0] == "D" for o in per)  # a D that is the last operation of a trip
    assert any(c == "X" and k >= 3 for o in per for c, k in o)
    assert any(o[i][0] == "D" and o[i + 1][0] == "X" for o in per for i in range(len(o) - 1))
    one = [s for s, o in enumerate(per) if len(o) == 1][0]
    assert int(got[6][one + 1]) - int(got[6][one]) == 1 and int(got[5][int(got[6][one])]) & 8
    assert (got[4]["strand"] == 2).sum() >= 5 and (got[4]["strand"] == 1).sum() >= 5
    # the same through the replay checker, which rebuilds the reads from the reference, the CIGAR and the MD alone
    ref_l = FakeLoaded([bytes(ref)], [b"ref"])
    letters = [bytes(q[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    names = [b"r%d" % i for i in range(len(letters))]
    sam = sam_spec.sam_file(want, names, letters, None, ref_l)
    assert sam_spec.replay_check(sam, ref_l, names, letters, results_of(got)) == len(got[0])


class FakeLoaded:
    """What sam_spec reads of a hostlib.Loaded, for a text built in the test: records joined by one N."""

    class _S:
        pass

    def __init__(self, recs, names):
        self.names, self.sizes = list(names), [len(r) for r in recs]
        self.merged_start = [int(x) for x in np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])[:-1]])]
        self.s = self._S()
        self.s.num = len(recs)
        self.chars = b"N".join(bytes(r) for r in recs)


def test_multi_record_reference_and_a_batch_without_a_mapping(eng):
    ref, q, off = multi_record_batch()
    idx = eng.Index.build(ref)
    got, want = check(eng, idx, ref, q, off, 20, True)
    assert (got[4]["strand"] == 1).sum() > 20 and (got[4]["strand"] == 2).sum() > 20
    assert list(got[8][-2:]) == [0xFFFFFFFF, 0xFFFFFFFF]
    q2, off2 = batch([np.frombuffer(b"N" * 50, dtype=np.uint8).copy(), np.frombuffer(b"ACGTAC", dtype=np.uint8).copy()])
    got = idx.map_reads(q2, off2, 20, True, md=True)
    assert len(got[0]) == 0 and len(got[5]) == 0 and list(got[6]) == [0] and len(got[7]) == 0
    assert list(got[8]) == [0xFFFFFFFF, 0xFFFFFFFF]
    idx.close()


SENTINEL = 0x5A5A5A5A


def maps_md_device(idx, segs, roff, ops, ooff, cap):
    """slamem_maps_md_device over a mapped batch given as map_reads returns it, with room for exactly `cap` entries in a buffer
    of cap + 1 words filled with SENTINEL: (return code, md_total, the whole buffer, md_offsets, seg_eq, primary, message)."""
    import ctypes as C
    import torch
    from slamem_amd import capi
    dev = idx.device

    def up(a, pad):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t = torch.zeros(a.shape[0] + pad, dtype=torch.uint8, device=dev)
        if a.shape[0]:
            t[: a.shape[0]] = torch.from_numpy(a.copy()).to(dev)
        return t
    nseg, num = len(segs), len(roff) - 1
    seg_t = up(segs, 32)
    roff_t = up(np.asarray(roff, dtype=np.uint64), 8)
    ops_t = up(np.asarray(ops, dtype=np.uint32), 8)
    ooff_t = up(np.asarray(ooff, dtype=np.uint64), 8)
    L = capi.lib()
    need, total = C.c_uint64(), C.c_uint64()
    capi.check(L.slamem_maps_md_workspace_bytes(nseg, num, C.byref(need)))
    ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
    md = torch.full((cap + 1,), SENTINEL, dtype=torch.int32, device=dev)
    moff = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    eq = torch.zeros(nseg + 1, dtype=torch.int32, device=dev)
    prim = torch.zeros(num + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = L.slamem_maps_md_device(idx._h, seg_t.data_ptr(), nseg, roff_t.data_ptr(), num, ops_t.data_ptr(), ooff_t.data_ptr(),
                                 md.data_ptr(), cap, moff.data_ptr(), eq.data_ptr(), prim.data_ptr(), ws.data_ptr(), need.value, None,
                                 C.byref(total))
    msg = L.slamem_last_error_message().decode(errors="replace") if rc else ""
    torch.cuda.synchronize(dev)
    return (rc, int(total.value), md.cpu().numpy().view(np.uint32), moff.cpu().numpy().view(np.uint64),
            eq[:nseg].cpu().numpy().view(np.uint32), prim[:num].cpu().numpy().view(np.uint32), msg)


def test_the_capacity_edge(eng):
    from slamem_amd import capi
    ref, q, off = designed_batch()
    idx = eng.Index.build(ref)
    segs, roff, ops, ooff, reads, md, moff, eq, prim = idx.map_reads(q, off, 14, True, md=True)
    need = len(md)
    assert need == int(moff[-1]) and need > 300 and need <= int(segs["edits"].sum()) + len(segs)
    rc, total, buf, g_moff, g_eq, g_prim, _ = maps_md_device(idx, segs, roff, ops, ooff, need)
    assert rc == capi.SLAMEM_OK and total == need and len(buf) == need + 1 and int(buf[need]) == SENTINEL
    for a, b in zip((buf[:need], g_moff, g_eq, g_prim), (md, moff, eq, prim)):
        assert np.array_equal(a, b)
    rc, total, left, _, _, _, msg = maps_md_device(idx, segs, roff, ops, ooff, need - 1)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total == need and str(need) in msg
    assert len(left) == need and int(left[need - 1]) == SENTINEL  # the word behind the capacity is as the caller left it
    assert np.array_equal(left[:need - 1], md[:need - 1])
    idx.close()


def test_compact_index_is_refused_and_still_searches(eng, monkeypatch):
    from slamem_amd import capi
    ref, q, off = indel_reads(13)
    full = eng.Index.build(ref)
    segs, roff, ops, ooff, _ = full.map_reads(q, off, 14, True)
    full.close()
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    idx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    assert idx.info.layout == capi.LAYOUT_COMPACT
    rc, total, buf, _, _, _, msg = maps_md_device(idx, segs, roff, ops, ooff, int(segs["edits"].sum()) + len(segs))
    assert rc == capi.SLAMEM_ERR_ARG and "text planes" in msg and "compact" in msg
    assert total == 0 and bool((buf == SENTINEL).all())  # nothing was run
    with pytest.raises(capi.SlamemError) as e:
        eng.Stream(idx, 3, 1 << 16, 13, True, paf=True, md=True)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "text planes" in str(e.value)
    mem, _ = idx.find_mems(q, off, 14, True)  # the process and the index go on
    assert len(mem) > 40
    idx.close()
    # the refused stream went at once, while its index was alive: collecting the exception after the index is closed runs no
    # destructor of it, and the next build finds no error left behind
    import gc
    gc.collect()
    again = eng.Index.build(ref)
    again.close()


def test_stream_equals_one_shot_and_other_streams_are_unchanged(eng):
    from slamem_amd import capi
    ref, q, off = indel_reads(7)
    idx = eng.Index.build(ref)
    per, nq = 60, len(off) - 1
    wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
    assert len(wins) == 3

    def run(**kw):
        st = eng.Stream(idx, 3, 1 << 16, per, True, **kw)
        out = []
        st.submit(q, wins[0], 14)
        st.submit(q, wins[1], 14)
        for b in range(len(wins)):
            m, ro, _ = st.next()
            item = [m.copy(), ro.copy()]
            if kw.get("paf") or kw.get("aln"):
                item += list(st.alns())
            if kw.get("paf"):
                item.append(rec_rows(st.maps()))
            if kw.get("md"):
                item += list(st.mds())
            out.append(item)
            if b + 2 < len(wins):
                st.submit(q, wins[b + 2], 14)
        st.close()
        return out

    def run_pile():
        """match type 8: the segments piled per batch, the read records, and the table the three batches leave"""
        pile = eng.Pileup(idx)
        st = eng.Stream(idx, 3, 1 << 16, per, True, pile=pile)
        out = []
        st.submit(q, wins[0], 14)
        st.submit(q, wins[1], 14)
        for b in range(len(wins)):
            piled, none, _ = st.next()
            assert none is None
            out.append([np.array([piled]), rec_rows(st.maps())])
            if b + 2 < len(wins):
                st.submit(q, wins[b + 2], 14)
        st.close()
        out.append([pile.counts()])
        pile.close()
        return out

    others = [dict(paf=True), dict(chain=True), dict(aln=True)]
    before = [run(**kw) for kw in others]
    pile_before = run_pile()
    assert int(pile_before[-1][0].sum()) > 0 and sum(int(x[0][0]) for x in pile_before[:-1]) > 100
    got = run(paf=True, md=True)
    segs, roff, ops, ooff, reads, md, moff, eq, prim = idx.map_reads(q, off, 14, True, md=True)
    assert np.array_equal(np.concatenate([g[5] for g in got]), md)
    assert np.array_equal(np.concatenate([np.diff(g[6].astype(np.int64)) for g in got]), np.diff(moff.astype(np.int64)))
    assert np.array_equal(np.concatenate([g[7] for g in got]), eq) and np.array_equal(np.concatenate([g[8] for g in got]), prim)
    assert np.array_equal(np.concatenate([seg_rows(g[0]) for g in got]), seg_rows(segs))
    assert np.array_equal(np.concatenate([g[4] for g in got]), rec_rows(reads))
    for kw, was in zip(others, before):  # what they returned before an MD call in the same process
        for x, y in zip(was, run(**kw)):
            for a, b in zip(x, y):
                assert np.array_equal(a, b)
    for x, y in zip(pile_before, run_pile()):  # match type 8: the piled counts, the read records and the table, exactly
        assert len(x) == len(y)
        for a, b in zip(x, y):
            assert np.array_equal(a, b)
    # the setter's rules
    with pytest.raises(ValueError):
        eng.Stream(idx, 3, 1 << 16, per, True, aln=True, md=True)
    L = capi.lib()
    st = eng.Stream(idx, 3, 1 << 16, per, True, aln=True)
    assert L.slamem_stream_set_md(st._h, 1) == capi.SLAMEM_ERR_ARG
    st.close()
    st = eng.Stream(idx, 3, 1 << 16, per, True, paf=True)
    st.submit(q, wins[0], 14)
    assert L.slamem_stream_set_md(st._h, 1) == capi.SLAMEM_ERR_ARG  # after the first submit
    st.next()
    st.close()
    idx.close()


def test_host_convenience_call(eng):
    import ctypes as C
    from slamem_amd import capi
    ref, q, off = indel_reads(17)
    idx = eng.Index.build(ref)
    want = idx.map_reads(q, off, 14, True, md=True)
    L = capi.lib()
    p = [C.c_void_p() for _ in range(9)]
    totals, nmd = (C.c_uint64 * 3)(), C.c_uint64()
    offs = np.ascontiguousarray(off, dtype=np.uint64)
    rc = L.slamem_find_maps_md_host(idx._h, np.ascontiguousarray(q).tobytes(), offs.ctypes.data, len(offs) - 1, 14, 1, 0, 0, 0xFFFFFFFF,
                                    0xFFFFFFFF, *[C.byref(x) for x in p[:5]], totals, *[C.byref(x) for x in p[5:]], C.byref(nmd))
    assert rc == capi.SLAMEM_OK, L.slamem_last_error_message()
    nseg, nq = int(totals[1]), len(offs) - 1
    assert nseg == len(want[0]) and nmd.value == len(want[5])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint32 * max(1, nmd.value)).from_address(p[5].value))[:nmd.value], want[5])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint64 * (nseg + 1)).from_address(p[6].value)), want[6])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint32 * max(1, nseg)).from_address(p[7].value))[:nseg], want[7])
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint32 * nq).from_address(p[8].value)), want[8])
    for x in p:
        L.slamem_host_free(x)
    idx.close()


# ---- the executable ---------------------------------------------------------------------------------------------------------

def fastq_twin(qs, path):
    """The queries as FASTQ with ascending quality bytes; returns the quality bytes per read."""
    quals = []
    with open(path, "wb") as f:
        for i in range(qs.n):
            letters = qs.chars[qs.offsets[i]:qs.offsets[i + 1]]
            quals.append(bytes(33 + (k % 60) for k in range(len(letters))))
            f.write(b"@" + qs.names[i] + b"\n" + letters + b"\n+\n" + quals[-1] + b"\n")
    return quals


@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_cli(case, tmp_path):
    """The executable's file, byte for byte: the spec's results formatted by the spec's SAM writer, from FASTA queries (QUAL *) and
    from a FASTQ twin of them; both through the replay checker."""
    results, _, ref, qs, opts = map_spec.golden_map(case)
    letters = [qs.chars[qs.offsets[i]:qs.offsets[i + 1]] for i in range(qs.n)]
    ref_fa, q_fa, _, _ = case_paths(case)
    q_fq = str(tmp_path / "q.fq")
    quals = fastq_twin(qs, q_fq)
    for queries, ql, argv_tail in ((q_fa, None, [ref_fa, "-sam", q_fa]), (q_fq, quals, ["-sam", ref_fa, q_fq])):
        out = tmp_path / "out.sam"
        r = subprocess.run([EXE] + opts + ["-o", str(out)] + argv_tail, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
        sam = out.read_bytes()
        assert sam == sam_spec.sam_file(results, qs.names, letters, ql, ref)
        assert sam_spec.replay_check(sam, ref, qs.names, letters, results, ql) == sum(len(x[4]) for x in results if x[0])
        assert b"Saving mappings" in r.stdout


def results_of_paf(paf: bytes, names, n_reads):
    """read_map-like tuples from the -paf file of the same reads (one reference record: ts is the merged position): what the
    replay checker takes as the reads' records.  A read without a line is unmapped."""
    by_name = {}
    for l in paf.split(b"\n")[:-1]:
        f = l.split(b"\t")
        n, qs_, qe, ts = int(f[1]), int(f[2]), int(f[3]), int(f[7])
        strand = 2 if f[4] == b"-" else 1
        rl = [(b.decode(), int(a)) for a, b in sam_spec._CIG.findall(f[15][5:])]
        qlen = qe - qs_
        q = qs_ if strand == 1 else n - qs_ - qlen
        seg = (ts, q, int(f[8]) - ts, qlen, int(f[12][5:]), rl)
        by_name.setdefault(f[0], [strand, int(f[11]), int(f[13][5:]), int(f[14][5:]), []])[4].append(seg)
    return [tuple(by_name.get(map_spec.cut_name(nm), [0, 0, 0, 0, []])) for nm in names[:n_reads]]


def test_cli_logical_gpus_byte_identical_and_the_paf_of_the_same_run(tmp_path):
    """Several batches over two streams (SLAMEM_LOGICAL_GPUS=2) give the file of one; the file replays against the read records
    of the -paf file of the same reads; and its mapped lines agree with that file field by field."""
    d = str(tmp_path)
    gen = os.path.join(ROOT, "tools", "gen_synth.py")
    g = subprocess.run([sys.executable, gen, "200000", "4000", "150", "0.02", "7", "50", d], stdout=subprocess.PIPE)
    assert g.returncode == 0
    ref_fa, q_fa = os.path.join(d, "ref.fa"), os.path.join(d, "qry.fa")
    ref, qs = hostlib.Loaded(ref_fa, 1), hostlib.Loaded(q_fa, 0)
    assert ref.s.num == 1 and len(set(qs.names)) == qs.n
    q_fq = os.path.join(d, "qry.fq")
    quals = fastq_twin(qs, q_fq)
    base = dict(os.environ, SLAMEM_BATCH_MB="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for name, args, env in (("paf", ["-paf"], base), ("one", ["-sam"], base), ("two", ["-sam"], dict(base, SLAMEM_LOGICAL_GPUS="2"))):
        out = os.path.join(d, f"{name}.txt")
        r = subprocess.run([EXE, "-b", "-l", "20"] + args + ["-o", out, ref_fa, q_fq], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, env=env, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        if name == "two":
            assert b"replicated to 2 logical GPUs by RCCL broadcast ... OK" in r.stdout
        outs[name] = open(out, "rb").read()
    assert outs["two"] == outs["one"]
    letters = [qs.chars[qs.offsets[i]:qs.offsets[i + 1]] for i in range(qs.n)]
    results = results_of_paf(outs["paf"], qs.names, qs.n)
    mapped = sam_spec.replay_check(outs["one"], ref, qs.names, letters, results, quals)
    assert mapped == outs["paf"].count(b"\n") > 3000
    sam = [l.split(b"\t") for l in outs["one"].split(b"\n")[:-1] if not l.startswith(b"@") and l.split(b"\t")[1] != b"4"]
    paf = [l.split(b"\t") for l in outs["paf"].split(b"\n")[:-1]]
    assert len(sam) == len(paf) == mapped
    for s, p in zip(sam, paf):
        n, qs_, qe = int(p[1]), int(p[2]), int(p[3])
        cg = sam_spec._CIG.findall(s[5])
        lead = int(cg[0][0]) if cg[0][1] == b"S" else 0
        tail = int(cg[-1][0]) if cg[-1][1] == b"S" else 0
        rev = bool(int(s[1]) & 16)
        assert s[0] == p[0] and len(s[9]) == n and (b"-" if rev else b"+") == p[4] and s[2] == p[5]
        assert (qs_, qe) == ((tail, n - lead) if rev else (lead, n - tail))
        assert int(s[3]) == int(p[7]) + 1 and s[4] == p[11]
        body = b"".join(a + b for a, b in cg if b != b"S")
        assert b"cg:Z:" + body == p[15] and s[11] == p[12] and s[13:15] == p[13:15]
        assert sum(int(a) for a, b in cg if b in b"=XD") == int(p[8]) - int(p[7])
