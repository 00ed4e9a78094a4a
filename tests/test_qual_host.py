"""-wq without a GPU: tests/qual_spec.py against its own known answers, against pile_spec (constant quality gives
q times the pileup) and against gt_spec (the two identities that tie the weighted genotype to the plain one)."""
import numpy as np
import pytest

import ext_spec
import gt_spec as gs
import lowq_spec
import pile_spec
import qual_spec as qs


def test_qv_at_the_edges():
    assert [qs.qv(b) for b in (0, 32, 33, 126, 255)] == [0, 0, 0, 93, 93]
    assert qs.qv(34) == 1 and qs.qv(125) == 92 and qs.qv(127) == 93
    assert [qs.qv(b, 64) for b in (0, 63, 64, 104, 157, 158, 255)] == [0, 0, 0, 40, 93, 93, 93]
    assert qs.qv(0, 0) == 0 and qs.qv(93, 0) == 93 and qs.qv(94, 0) == 93


def test_the_costs_are_the_rounded_logarithms():
    import math
    assert qs.WQ_COSTS == (0, int(math.floor(10000 * math.log10(2) + 0.5)), int(math.floor(10000 * math.log10(3) + 0.5)))
    for q in range(1, 94):  # a miscalled letter of quality q costs what gt_costs' E says, exactly
        assert 1000 * q + qs.WQ_COSTS[2] == gs.gt_costs(q)[2], q


def one_read(strand, p, ops):
    rlen = sum(k for c, k in ops if c in "=XD")
    qlen = sum(k for c, k in ops if c in "=XI")
    return (strand, 60, 0, 0, [(p, 0, rlen, qlen, 0, ops)])


def test_known_answers_forward_and_reverse():
    n = 12
    read = b"ACGTNACG"
    quals = bytes([33 + v for v in (10, 10, 20, 0, 30, 40, 93, 94)])
    # forward at row 2: = 3, X 2 (T, N), I 1 (A), D 2, = 2 (C, G)
    t = pile_spec.empty(n)
    assert qs.add_read(t, one_read(1, 2, [("=", 3), ("X", 2), ("I", 1), ("D", 2), ("=", 2)]), read, quals)
    want = pile_spec.empty(n)
    want[2, 0], want[3, 1], want[4, 2] = 10, 10, 20
    want[5, 3] = 0      # T of quality 0
    #    row 6: N counts nowhere; the inserted A and the deleted rows 7, 8 add nothing
    want[9, 1], want[10, 2] = 93, 93
    assert np.array_equal(t, want)
    # reverse: the scanned strand is CGTNACGT, letter x has the byte at 7 - x
    t = pile_spec.empty(n)
    assert qs.add_read(t, one_read(2, 0, [("=", 8)]), read, quals)
    want = pile_spec.empty(n)
    for x, (col, v) in enumerate(((1, 93), (2, 93), (3, 40), (None, 30), (0, 0), (1, 20), (2, 10), (3, 10))):
        if col is not None:
            want[x, col] = v
    assert np.array_equal(t, want)
    # a low letter counts nowhere; rows at or behind n are dropped; an unmapped read and one below min_mapq give nothing
    t = pile_spec.empty(n)
    qs.add_read(t, one_read(1, 8, [("=", 8)]), read, quals, low=[0, 1, 0, 0, 0, 0, 0, 0])
    assert t.sum() == 10 + 20 and t[8, 0] == 10 and t[10, 2] == 20
    assert not qs.add_read(t, one_read(0, 0, [("=", 8)]), read, quals) and not qs.add_read(t, one_read(1, 0, [("=", 8)]), read, quals, min_mapq=61)
    assert t.sum() == 30


def random_batch(rng, n, reads):
    res, letters, quals, off = [], [], [], [0]
    for _ in range(reads):
        L = int(rng.integers(5, 40))
        strand = int(rng.integers(0, 3))
        ops, left = [], L
        while left:
            c = "=XI"[int(rng.integers(0, 3))]
            k = int(rng.integers(1, left + 1))
            ops.append((c, k))
            left -= k
            if rng.random() < 0.3:
                ops.append(("D", int(rng.integers(1, 4))))
        p = int(rng.integers(0, n - 5))
        # (rows behind n: cut the read's reference span by starting early enough)
        span = sum(k for c, k in ops if c in "=XD")
        p = min(p, max(0, n - span))
        if span > n:
            continue
        res.append((strand, int(rng.integers(0, 61)), 0, 0, [(p, 0, span, L, 0, ops)]))
        letters.append(rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), size=L))
        quals.append(rng.integers(0, 256, size=L).astype(np.uint8))
        off.append(off[-1] + L)
    return res, np.concatenate(letters), np.concatenate(quals), np.array(off, dtype=np.uint64)


@pytest.mark.parametrize("seed", range(3))
def test_constant_quality_is_q_times_the_pileup(seed):
    rng = np.random.default_rng(seed)
    n = 90
    res, q, _, off = random_batch(rng, n, 40)
    bits = (rng.random(len(q)) < 0.2).astype(np.uint8)
    mask = lowq_spec.from_bits(bits.tolist())
    for v, min_mapq, m in ((0, 0, None), (7, 0, None), (40, 20, None), (93, 0, mask), (200, 30, mask)):
        quals = np.full(len(q), min(33 + v, 255), dtype=np.uint8)
        got = qs.pile(res, q, off, quals, n, m, min_mapq)
        want = lowq_spec.pile(res, q, off, n, m, min_mapq)
        assert not got[:, 4:].any()
        assert np.array_equal(got[:, :4], min(v, 93) * want[:, :4]), (v, min_mapq)
    # any qualities: Q <= 93 * P, column by column
    _, _, quals, _ = random_batch(np.random.default_rng(seed), n, 40)
    got, want = qs.pile(res, q, off, quals, n), pile_spec.pile(res, q, off, n)
    assert bool((got[:, :4] <= 93 * want[:, :4]).all()) and got.sum() > 0


def random_tables(rng, n):
    text = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=n, p=[0.24, 0.24, 0.24, 0.24, 0.04])
    table = np.zeros((n, 6), dtype=np.int64)
    for x in range(n):
        kind = x % 4
        depth = int(rng.integers(0, 60))
        r = {65: 0, 67: 1, 71: 2, 84: 3}.get(int(text[x]), 0)
        if kind == 0:
            table[x, r] = depth
        elif kind == 1:
            table[x, r], table[x, (r + 1) % 4] = depth // 2, depth - depth // 2
        elif kind == 2:
            table[x, (r + 2) % 4] = depth
        else:
            table[x, :4] = rng.integers(0, 20, size=4)
        table[x, 4] = int(rng.integers(0, 3))
    return text, table


@pytest.mark.parametrize("ploidy", [1, 2])
def test_the_two_identities_against_gt_spec(ploidy):
    rng = np.random.default_rng(11 + ploidy)
    text, table = random_tables(rng, 300)
    zero = np.zeros_like(table)
    for costs in (qs.WQ_COSTS, gs.gt_costs(20)):
        p = qs.params(ploidy=ploidy, min_depth=2, min_qual=3, costs=costs)
        # Q all zero: the plain read-out, byte for byte
        pos, counts, gts, qsums = qs.genotypes(table, zero, text, p)
        wpos, wcounts, wgts = gs.genotypes(table, text, p)
        assert len(pos) > 20 and np.array_equal(pos, wpos) and np.array_equal(counts, wcounts) and gts.tobytes() == wgts.tobytes()
        assert not qsums.any()
        # every letter at quality q: the plain read-out with err_cost + 1000 q
        for q in (1, 20, 93):
            qt = q * table
            qt[:, 4:] = 0
            pos, counts, gts, qsums = qs.genotypes(table, qt, text, p)
            pq = gs.check_params((p[0], p[1], p[2], p[3] + 1000 * q) + p[4:])
            wpos, wcounts, wgts = gs.genotypes(table, text, pq)
            assert np.array_equal(pos, wpos) and np.array_equal(counts, wcounts) and gts.tobytes() == wgts.tobytes(), q
            assert np.array_equal(qsums, q * counts[:, :4])


def test_a_low_quality_mismatch_weighs_less():
    """Ten reads show the text's A at Q40, four show C: at Q40 the row is called A/C, at Q2 it is not called at all."""
    text = b"A"
    table = np.array([[10, 4, 0, 0, 0, 0]], dtype=np.int64)
    p = qs.params(min_depth=2, min_qual=0)
    high = np.array([[400, 160, 0, 0, 0, 0]], dtype=np.int64)
    low = np.array([[400, 8, 0, 0, 0, 0]], dtype=np.int64)
    pos, _, gts, qsums = qs.genotypes(table, high, text, p)
    assert list(pos) == [0] and (int(gts[0]["a"]), int(gts[0]["b"])) == (0, 1) and list(qsums[0]) == [400, 160, 0, 0]
    pos, _, _, _ = qs.genotypes(table, low, text, p)
    assert len(pos) == 0
    # the scores themselves, by hand: AA costs the four C, 4 * 4771 + 1000 * 8; A/C costs 14 * 3010 + the prior
    g, variant = qs.snv(table[0], low[0], 0, p)
    assert not variant and g[6][0] == 0 and g[6][1] == 14 * 3010 - (4 * 4771 + 8000)


# ---- the formatter and the command line ------------------------------------------------------------------------------------------

import ctypes as C  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

import events_spec as es  # noqa: E402
import hostlib  # noqa: E402
from test_sb_host import sb_case, write_fasta  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")


def wq_case():
    """test_sb_host's case with quality sums: high on most rows, low on the T of row 1 (the 1/1 there weakens) and on the A of row 3."""
    ref, t, f, ev = sb_case()
    q = 30 * t
    q[:, 4:] = 0
    q[1, 3] = 2 * t[1, 3]
    q[3, 0] = 3 * t[3, 0]
    q[2] = (9 * 40, 0, 1 * 5, 9 * 20, 0, 0)
    return ref, t, f, q, ev


def host_wq_vcf(ref, t, f, q, ev, p, sb=False, fs=None, err_q=20) -> bytes:
    """The file as the executable's writer makes it from the read-outs: slh_format_vcf_wq_header, then per record
    slh_format_vcf_wq_rows over the rows the weighted read-out selects (here the spec's) and the events genotyped with -err's costs."""
    L = hostlib.lib()
    vp = C.c_void_p
    L.slh_format_vcf_wq_header.argtypes = [C.POINTER(hostlib.Buffer), C.POINTER(hostlib.Record), C.c_int, C.c_int, C.c_int]
    L.slh_format_vcf_wq_rows.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, vp, vp, vp, vp, vp,
                                         C.c_uint64, vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int]
    pe = gs.check_params((p[0],) + gs.gt_costs(err_q) + p[4:])
    pos, counts, gts, qsums = qs.genotypes(t, q, ref.chars, p)
    recs = (hostlib.Record * len(ref.names))(*[hostlib.Record(nm, sz) for nm, sz in zip(ref.names, ref.sizes)])
    b = hostlib.Buffer()
    filt = -1 if fs is None else fs
    assert L.slh_format_vcf_wq_header(C.byref(b), recs, len(ref.names), int(sb), filt) == 0
    for r, name in enumerate(ref.names):
        a, size = int(ref.merged_start[r]), int(ref.sizes[r])
        mine = (pos >= a) & (pos < a + size)
        evs = [e for e in ev if a <= e[0] < a + size]
        anchors = [e[0] - 1 if e[0] > a else e[0] for e in evs]
        rows = np.ascontiguousarray(t[anchors].astype(np.uint32).reshape(len(anchors), 6))
        frows = np.ascontiguousarray(f[anchors].astype(np.uint32).reshape(len(anchors), 6))
        eg, called = gs.genotype_events(evs, rows, pe)
        p_, c_, g_, q_ = (np.ascontiguousarray(x[mine]) for x in (pos, counts, gts, qsums))
        sf = np.ascontiguousarray(f[p_.astype(np.int64)].astype(np.uint32).reshape(len(p_), 6))
        er = es.to_records(evs)
        assert L.slh_format_vcf_wq_rows(C.byref(b), name, a, size, ref.chars, p_.ctypes.data, c_.ctypes.data, sf.ctypes.data if sb else None,
                                        q_.ctypes.data, g_.ctypes.data, len(p_), er.ctypes.data, rows.ctypes.data,
                                        frows.ctypes.data if sb else None, eg.ctypes.data, called.ctypes.data, len(evs), int(sb), filt) == 0
    out = C.string_at(b.data, b.len) if b.len else b""
    L.slh_buffer_free(C.byref(b))
    return out


def test_spec_file_by_hand():
    ref, t, f, q, ev = wq_case()
    p = qs.params(min_depth=2, min_qual=3)
    vcf = qs.vcf_file(t, q, ev, ref, p)
    head = gs.vcf_header(ref)
    assert vcf.startswith(head[:head.index(b"#CHROM")] + qs.HEADER_ADQ + b"#CHROM")
    lines = vcf[len(qs.vcf_header(ref)):].split(b"\n")[:-1]
    cols = [line.split(b"\t") for line in lines]
    assert all(c[8] == b"GT:DP:AD:GQ:PL:ADQ" for c in cols)
    first = cols[0]  # row 0: A, ten A at Q30 and ten C at Q30: 0/1, AD 10,10, ADQ 300,300
    assert first[1] == b"1" and first[3:5] == [b"A", b"C"] and first[9].startswith(b"0/1:20:10,10:") and first[9].endswith(b":300,300")
    third = next(c for c in cols if c[1] == b"3" and len(c[3]) == 1 and len(c[4].split(b",")) == 2)  # G: 1/2 with A and T
    assert third[9].endswith(b":5,360,180")
    indels = [c for c in cols if len(c[3]) != len(c[4].split(b",")[0])]
    assert indels and all(c[9].endswith(b":.") for c in indels)
    # without the decoration: the events' lines are those of -vcf -gt at -err 20, whatever the rows' costs are
    plain = gs.vcf_file(t, ev, ref, gs.params(min_depth=2, min_qual=3))
    assert [b"\t".join(c[:8]) for c in indels] == [b"\t".join(l.split(b"\t")[:8]) for l in plain.split(b"\n") if l and not l.startswith(b"#")
                                                    and len(l.split(b"\t")[3]) != len(l.split(b"\t")[4].split(b",")[0])]


@pytest.mark.parametrize("sb,fs", [(False, None), (True, None), (True, 30)])
@pytest.mark.parametrize("ploidy,err_q", [(2, 20), (1, 35)])
def test_host_formatter_against_the_spec(sb, fs, ploidy, err_q):
    ref, t, f, q, ev = wq_case()
    p = qs.params(ploidy=ploidy, min_depth=2, min_qual=3)
    want = qs.vcf_file(t, q, ev, ref, p, f if sb else None, fs, err_q)
    assert want.count(b"\n") > qs.vcf_header(ref, sb, fs).count(b"\n") + 4
    assert host_wq_vcf(ref, t, f, q, ev, p, sb, fs, err_q) == want


def test_large_sums_in_the_line():
    ref, t, f, q, ev = wq_case()
    q = q.copy()
    q[0, :2] = (2 ** 32 - 1, 2 ** 32 - 2)
    p = qs.params(min_depth=2, min_qual=0)
    got = host_wq_vcf(ref, t, f, q, ev, p)
    assert got == qs.vcf_file(t, q, ev, ref, p) and b":4294967295,4294967294\n" in got


def test_option_row_and_refusals_of_the_parser():
    assert ("wq", False) in hostlib.option_rows()
    L = hostlib.lib()
    L.slh_parse_wq.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    assert L.slh_parse_wq(5, hostlib.c_argv(["x", "-vcf", "-gt", "-WQ", "a"])) == 1 and L.slh_parse_wq(3, hostlib.c_argv(["x", "-win", "a"])) == 0
    o = hostlib.parse_options(["slaMEM", "-vcf", "-gt", "-wq", "ref.fa", "reads.fq"])  # (-wq takes no value: the files stay the files)
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fq"]
    for args, refusal in ((["-vcf", "-gt", "-wq"], None), (["-vcf", "-gt", "-wq", "-sb", "-bq", "10", "-err", "30"], None),
                          (["-vcf", "-wq"], "Option -wq needs -gt"), (["-pile", "-wq"], "Option -wq needs -gt"),
                          (["-gt", "-wq"], "Option -gt needs -vcf")):
        rc, msg, _ = hostlib.parse_run(["slaMEM"] + args + ["ref.fa", "reads.fa"])
        assert (rc, msg) == ((0, None) if refusal is None else (-1, refusal)), args


@pytest.mark.parametrize("args,message", [(["-wq"], b"Option -wq needs -gt"), (["-vcf", "-wq"], b"Option -wq needs -gt"),
                                          (["-sites", "-wq"], b"Option -wq needs -gt"), (["-gt", "-wq"], b"Option -gt needs -vcf")])
def test_cli_refusals_exit_before_any_gpu_work(args, message, tmp_path):
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"r", b"ACGT" * 30)])
    write_fasta(q_fa, [(b"q", b"ACGT" * 10)])
    r = subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))  # (no device: it never asks for one)
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout


def test_usage_lists_the_option():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    assert b"\t-wq\t" in r.stdout
