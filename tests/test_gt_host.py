"""-gt on the CPU: the definition (tests/gt_spec.py) itself on answers worked out by hand, the costs of a letter
in C and in Python, the tie rule and the saturation, then the host library's VCF formatter against the spec and the refusals of
the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import events_spec as es
import gt_spec as gs
import hostlib
import pile_spec
from test_map_host import FakeRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
DEFAULT = gs.params()  # q = 20, hp = 30000, depth 4, qual 20


def row(ref, alt, r=0, a=1):
    c = [0, 0, 0, 0, 0, 0]
    c[r], c[a] = ref, alt
    return c


# ---- known answers -------------------------------------------------------------------------------------------------------------

def test_costs_at_q_20_and_the_defaults():
    assert gs.gt_costs(20) == (44, 3039, 24771)
    assert DEFAULT == (2, 44, 3039, 24771, 30000, 4, 20)
    assert gs.GENOTYPE_DTYPE.itemsize == 56


def test_three_known_answers():
    # reference 10, alternative 10: het, S = 90780 against 248150
    g, variant = gs.snv(row(10, 10), 0, DEFAULT)
    assert variant and g[:6] == (157370, 157370, 0, 1, 2, 0)
    assert 20 * 3039 + 30000 == 90780 and 10 * 44 + 10 * 24771 == 248150 and 248150 - 90780 == 157370
    assert min(gs.phred(g[1]), 99) == 99
    assert g[6][gs.genotype_index(0, 1)] == 0 and g[6][gs.genotype_index(0, 0)] == 248150 - 60780
    # reference 3, alternative 1: hom-ref wins, 24903 against 42156
    g, variant = gs.snv(row(3, 1), 0, DEFAULT)
    assert not variant and (g[2], g[3]) == (0, 0) and g[0] == 0 and g[1] == 42156 - 24903
    # reference 2, alternative 2: het with qual 7474, below -qual 20
    g, variant = gs.snv(row(2, 2), 0, DEFAULT)
    assert not variant and (g[0], g[2], g[3]) == (7474, 0, 1)
    assert gs.snv(row(2, 2), 0, DEFAULT[:6] + (7,))[1] and not gs.snv(row(2, 2), 0, DEFAULT[:6] + (8,))[1]
    # the same through the table: rows of depth 20, 4 and 4 under A
    t = pile_spec.empty(6)
    t[1], t[2], t[3] = row(10, 10), row(3, 1), row(2, 2)
    pos, counts, gts = gs.genotypes(t, b"AAAAAA", DEFAULT)
    assert list(pos) == [1] and counts.tolist() == [row(10, 10)] and int(gts[0]["qual"]) == 157370 and gts[0]["pad"].tolist() == [0] * 4


def test_the_other_reference_letters_and_ploidy_1():
    # under T a het A/T is (a, b) = (0, 3): letters ascending, whatever the reference
    g, variant = gs.snv([10, 0, 0, 10, 0, 0], 3, DEFAULT)
    assert variant and (g[2], g[3], g[5]) == (0, 3, 3) and g[0] == 157370
    # two alternatives, no reference: C/G under A, two priors
    g, variant = gs.snv([0, 10, 10, 0, 0, 0], 0, DEFAULT)
    assert variant and (g[2], g[3]) == (1, 2) and g[0] == (20 * 24771) - (20 * 3039 + 60000)
    # ploidy 1: the plurality letter when the prior lets it; pl has four entries
    p1 = gs.params(ploidy=1)
    g, variant = gs.snv(row(3, 10), 0, p1)
    assert variant and (g[2], g[3], g[4]) == (1, 1, 1) and g[6][4:] == [0] * 6
    assert g[0] == (3 * 44 + 10 * 24771) - (10 * 44 + 3 * 24771 + 30000)
    g, variant = gs.snv(row(10, 10), 0, p1)
    assert not variant and (g[2], g[3]) == (0, 0)  # (equal likelihoods: the prior decides)
    # min_depth looks at A+C+G+T+D
    t = pile_spec.empty(3)
    t[0] = (2, 2, 0, 0, 0, 9)
    t[1] = (2, 2, 0, 0, 1, 0)
    assert list(gs.genotypes(t, b"AAA", gs.params(min_depth=5, min_qual=0))[0]) == [1]
    assert list(gs.genotypes(t, b"NAA", gs.params(min_depth=4, min_qual=0))[0]) == [1]


def test_events_known_answers():
    g, called = gs.event(10, 20, DEFAULT)
    assert called and g[:6] == (157370, 157370, 0, 1, 2, 0) and g[6][:3] == [248150 - 60780, 0, 248150 - 60780] and g[6][3:] == [0] * 7
    g, called = gs.event(20, 20, DEFAULT)
    assert called and (g[2], g[3]) == (1, 1) and g[0] == 20 * 24771 - (20 * 44 + 30000)
    # 1 of 4: L = 24903, 12156, 74357; the prior keeps 0/0, and pl is measured from the het's likelihood
    assert gs.event(1, 4, DEFAULT) == ((0, 42156 - 24903, 0, 0, 2, 0, [24903 - 12156, 0, 74357 - 12156] + [0] * 7), False)
    # more observations than depth: ro is 0
    g, called = gs.event(30, 20, DEFAULT)
    assert called and (g[2], g[3]) == (1, 1) and g[6][0] == 30 * 24771 - 30 * 44
    # depth below min_depth: genotyped, not called
    g, called = gs.event(3, 3, DEFAULT)
    assert not called and (g[2], g[3]) == (1, 1)
    # ploidy 1
    g, called = gs.event(15, 20, gs.params(ploidy=1))
    assert called and (g[2], g[3], g[4]) == (1, 1, 1) and g[6][2:] == [0] * 8


# ---- the costs in C and in Python ----------------------------------------------------------------------------------------------

def test_costs_agree_between_c_python_and_the_spec():
    from slamem_amd import capi, engine
    L = capi.lib()
    out = (C.c_uint32 * 3)()
    seen = set()
    for q in range(1, 94):
        assert L.slamem_gt_costs(q, out) == capi.SLAMEM_OK
        got = tuple(int(v) for v in out)
        assert got == engine.gt_costs(q) == gs.gt_costs(q), q
        M, H, E = got
        assert 0 <= M < H < E <= 97771 or q == 1  # (q = 1: e = 0.79, a letter is more likely wrong than right)
        seen.add(got)
    assert len(seen) == 93 and tuple(int(v) for v in out) == (0, 3010, 97771)
    for q in (0, 94, 2 ** 31):
        assert L.slamem_gt_costs(q, out) == capi.SLAMEM_ERR_ARG
        assert b"slamem_gt_costs" in L.slamem_last_error_message()
    for q in (0, 94):
        with pytest.raises(ValueError):
            engine.gt_costs(q)
        with pytest.raises(ValueError):
            gs.gt_costs(q)
    assert engine.GENOTYPE_DTYPE == gs.GENOTYPE_DTYPE


# ---- ties and saturation -------------------------------------------------------------------------------------------------------

def test_tie_rule():
    # equal S keeps the reference: with M = H = E every L is equal, and with hp = 0 so is every S
    flat = (2, 5, 5, 5, 0, 1, 0)
    for r in range(4):
        g, variant = gs.snv([3, 1, 4, 1, 0, 0], r, flat)
        assert not variant and (g[2], g[3]) == (r, r) and g[0] == 0 and g[1] == 0
    # het and hom-ref at the same score: 2 H c = M c + E c  (c reference, c alternative)
    tie = (2, 10, 30, 50, 0, 1, 0)
    g, variant = gs.snv(row(7, 7), 0, tie)
    assert not variant and (g[2], g[3]) == (0, 0) and g[1] == 0
    g, variant = gs.snv(row(7, 7, r=2, a=3), 2, tie)
    assert not variant and (g[2], g[3]) == (2, 2)
    # two equal alternatives take the smaller g: C and G seen alike under A -> CC (g = 2) before GG (g = 5); under T, AA before CC
    hom = (2, 1, 1000, 1000, 0, 1, 0)
    g, variant = gs.snv([0, 6, 6, 0, 0, 0], 0, hom)
    assert variant and (g[2], g[3]) == (1, 1) and g[1] == 0
    g, variant = gs.snv([6, 6, 0, 0, 0, 0], 3, hom)
    assert variant and (g[2], g[3]) == (0, 0)
    # ... and of the hets AC (g = 1) before AG (g = 3) before CG (g = 4)
    het = (2, 1000, 1, 1000, 0, 1, 0)
    g, variant = gs.snv([5, 5, 5, 0, 0, 0], 3, het)
    assert variant and (g[2], g[3]) == (0, 1) and g[1] == 0
    # ploidy 1
    g, variant = gs.snv([0, 6, 6, 0, 0, 0], 0, (1, 1, 1000, 1000, 0, 1, 0))
    assert variant and (g[2], g[3]) == (1, 1)
    # an event at a tie stays 0/0
    g, called = gs.event(7, 14, tie)
    assert not called and (g[2], g[3]) == (0, 0) and g[1] == 0


def test_saturation_at_the_largest_counts():
    big = 2 ** 31 - 1
    g, variant = gs.snv([big, big, 0, 0, 0, 0], 0, DEFAULT)
    assert variant and (g[2], g[3]) == (0, 1) and g[0] == gs.SAT and g[1] == gs.SAT
    assert g[6][gs.genotype_index(0, 1)] == 0 and all(v == gs.SAT for k, v in enumerate(g[6]) if k != 1)
    # the largest costs the interface takes, on every column: the sums stay below 2^64 (the spec asserts it)
    g, variant = gs.snv([2 ** 32 - 1] * 4, 0, (2, 2 ** 20, 2 ** 20, 2 ** 20, 2 ** 20, 1, 0))
    assert not variant and g[0] == 0
    g, called = gs.event(2 ** 33 - 2, 5 * (2 ** 32 - 1), (2, 0, 2 ** 20, 2 ** 20, 2 ** 20, 1, 999))
    assert g[0] in (0, gs.SAT)
    recs = gs.to_records([gs.snv([big, big, 0, 0, 0, 0], 0, DEFAULT)[0]])
    assert gs.from_records(recs)[0] == gs.snv([big, big, 0, 0, 0, 0], 0, DEFAULT)[0]


def test_parameters_are_checked():
    for bad in ((3, 44, 3039, 24771, 30000, 4, 20), (0, 44, 3039, 24771, 30000, 4, 20), (2, 44, 0, 24771, 30000, 4, 20),
                (2, 44, 3039, 0, 30000, 4, 20), (2, 2 ** 20 + 1, 3039, 24771, 30000, 4, 20), (2, 44, 3039, 2 ** 20 + 1, 30000, 4, 20),
                (2, 44, 3039, 24771, 2 ** 20 + 1, 4, 20), (2, 44, 3039, 24771, 30000, 0, 20), (2, 44, 3039, 24771, 30000, 2 ** 31, 20),
                (2, 44, 3039, 24771, 30000, 4, 1000)):
        with pytest.raises(ValueError):
            gs.check_params(bad)
    gs.check_params((1, 0, 1, 1, 0, 2 ** 31 - 1, 999))


# ---- the VCF lines -------------------------------------------------------------------------------------------------------------

def gt_case():
    """Two records (the second begins with a lower-case letter): a het, a hom-alt, a 1/2, a het under T (a is the alternative), a row
    that is not called, and events -- one at the second record's first base, one that is called 1/1, one that is not called."""
    recs = [b"ACGTTGCAAC", b"gGATCCATAG"]
    ref = FakeRef(recs, [b"first one", b"second\tx"])
    n = len(ref.chars)  # 10 + 1 + 10: the separator at 10
    t = pile_spec.empty(n)
    t[0] = (10, 10, 0, 0, 0, 0)     # A: 0/1 with C
    t[1] = (0, 1, 0, 19, 0, 0)      # C: 1/1 with T
    t[2] = (9, 0, 1, 9, 2, 0)       # G: 1/2, A and T; D counts in the depth
    t[3] = (12, 0, 0, 8, 0, 1)      # T: 0/1 with A
    t[4] = (1, 0, 0, 19, 0, 0)      # T: not called
    t[6] = (0, 20, 0, 0, 0, 0)      # C: the anchor of the event at 7
    t[10] = (9, 9, 0, 0, 0, 0)      # the separator
    t[11] = (0, 0, 20, 0, 0, 0)     # g: the anchor of the events at the second record's start
    t[14] = (0, 0, 0, 12, 0, 0)
    ev = [
        (3, 0, 1, b"", 3, 1),        # anchor row 2 (d = 21): 4 of 21, not called at the defaults
        (7, 1, 2, b"GA", 5, 4),      # anchor row 6 (d = 20): 0/1
        (7, 0, 2, b"", 10, 9),       # anchor row 6: 1/1
        (10, 1, 1, b"A", 9, 9),      # on the separator: no record's event
        (11, 0, 2, b"", 6, 6),       # the second record's first base: the following base anchors
        (11, 1, 3, b"TTA", 0, 20),   # the same place: 1/1
        (15, 1, 1, b"C", 1, 0),      # anchor row 14 (d = 12): not called
    ]
    return ref, t, sorted(ev, key=es.order_key)


def host_gt_vcf(ref, t, ev, p) -> bytes:
    L = hostlib.lib()
    L.slh_format_vcf_gt_header.argtypes = [C.POINTER(hostlib.Buffer), C.POINTER(hostlib.Record), C.c_int]
    L.slh_format_vcf_gt_rows.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    recs = (hostlib.Record * len(ref.names))(*[hostlib.Record(nm, sz) for nm, sz in zip(ref.names, ref.sizes)])
    b = hostlib.Buffer()
    assert L.slh_format_vcf_gt_header(C.byref(b), recs, len(ref.names)) == 0
    pos, counts, gts = gs.genotypes(t, ref.chars, p)
    for r, name in enumerate(ref.names):
        a, size = int(ref.merged_start[r]), int(ref.sizes[r])
        mine = (pos >= a) & (pos < a + size)
        evs = [e for e in ev if a <= e[0] < a + size]
        anchors = [e[0] - 1 if e[0] > a else e[0] for e in evs]
        rows = np.ascontiguousarray(t[anchors].astype(np.uint32).reshape(len(anchors), 6))
        eg, called = gs.genotype_events(evs, rows, p)
        e_ = es.to_records(evs)
        p_, c_, g_ = (np.ascontiguousarray(x[mine]) for x in (pos, counts, gts))
        assert L.slh_format_vcf_gt_rows(C.byref(b), name, a, size, ref.chars, p_.ctypes.data, c_.ctypes.data, g_.ctypes.data, len(p_),
                                        e_.ctypes.data, rows.ctypes.data, eg.ctypes.data, called.ctypes.data, len(evs)) == 0
    out = C.string_at(b.data, b.len) if b.len else b""
    L.slh_buffer_free(C.byref(b))
    return out


def test_vcf_file_written_out_by_hand():
    ref, t, ev = gt_case()
    got = gs.vcf_file(t, ev, ref, DEFAULT)
    head = gs.vcf_header(ref)
    assert head.startswith(b"##fileformat=VCFv4.2\n##contig=<ID=first,length=10>\n##contig=<ID=second,length=10>\n##INFO=<ID=DP,")
    assert head.endswith(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n")
    assert head.count(b"##INFO=<ID=") == 4 and [head.count(b"##FORMAT=<ID=%s," % k) for k in (b"GT", b"DP", b"AD", b"GQ", b"PL")] == [1] * 5
    body = got[len(head):].split(b"\n")
    assert body[-1] == b"" and len(body) == 9
    # the het of the issue: QUAL 157, GQ 99, PL over A/A, A/C, C/C
    assert body[0] == b"first\t1\t.\tA\tC\t157\t.\tDP=20;AO=10\tGT:DP:AD:GQ:PL\t0/1:20:10,10:99:187,0,187"
    assert body[1].startswith(b"first\t2\t.\tC\tT\t") and b"\tDP=20;AO=19\tGT:DP:AD:GQ:PL\t1/1:20:1,19:" in body[1]
    assert body[2].startswith(b"first\t3\t.\tG\tA,T\t") and b"\tDP=21;AO=9,9\tGT:DP:AD:GQ:PL\t1/2:21:1,9,9:" in body[2]
    assert body[2].split(b":")[-1].count(b",") == 5 and body[2].split(b":")[-1].split(b",")[4] == b"0"  # (six PL values, 1/2 the best)
    assert body[3].startswith(b"first\t4\t.\tT\tA\t") and b"\tGT:DP:AD:GQ:PL\t0/1:20:8,12:" in body[3]
    assert body[4].startswith(b"first\t7\t.\tCAA\tC\t") and b";AO=19;SF=10;SR=9\tGT:DP:AD:GQ:PL\t1/1:20:1,19:" in body[4]
    assert body[5].startswith(b"first\t7\t.\tC\tCGA\t") and b";AO=9;SF=5;SR=4\tGT:DP:AD:GQ:PL\t0/1:20:11,9:" in body[5]
    assert body[6].startswith(b"second\t1\t.\tGGA\tA\t") and b"\tDP=20;AO=12;SF=6;SR=6\tGT:DP:AD:GQ:PL\t0/1:20:8,12:" in body[6]
    assert body[7].startswith(b"second\t1\t.\tG\tTTAG\t") and b"\tGT:DP:AD:GQ:PL\t1/1:20:0,20:" in body[7]
    assert not any(b"first\t5\t" in line or b"\tTG\tT\t" in line or b"second\t4" in line for line in body)
    # ploidy 1: one allele number, as many PL values as alleles; the het rows fall to the reference or to the plurality letter
    one = gs.vcf_file(t, ev, ref, gs.params(ploidy=1))[len(head):]
    assert b"first\t2\t.\tC\tT\t" in one and b"\tGT:DP:AD:GQ:PL\t1:20:1,19:" in one and b"/" not in one.replace(b"GT:DP:AD:GQ:PL", b"")
    assert b"first\t1\t" not in one


CASES = [DEFAULT, gs.params(ploidy=1), gs.params(min_qual=0, min_depth=1), gs.params(err_q=40, het_q=0), gs.params(err_q=3, het_q=50),
         gs.params(min_depth=21), (2, 10, 30, 50, 0, 1, 0)]


@pytest.mark.parametrize("p", CASES)
def test_host_formatter_against_the_spec(p):
    ref, t, ev = gt_case()
    want = gs.vcf_file(t, ev, ref, p)
    assert host_gt_vcf(ref, t, ev, p) == want
    assert want.count(b"\n") > gs.vcf_header(ref).count(b"\n") or p[5] == 21


def test_host_formatter_large_counters():
    rng = np.random.default_rng(4)
    body = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=300))
    ref = FakeRef([body], [b"chr 1"])
    t = pile_spec.empty(len(body))
    col = b"ACGT".index(body[100:101])
    t[100] = (2 ** 32 - 1,) * 6
    t[101, col], t[101, (col + 1) % 4] = 2 ** 31 - 1, 2 ** 31 - 1
    p, _ = es.normalise(body, 150, 0, 127)
    ev = [(p, 0, 127, b"", 2 ** 32 - 1, 2 ** 32 - 1)]
    t[p - 1] = (2 ** 32 - 1,) * 6
    got = host_gt_vcf(ref, t, ev, DEFAULT)
    assert got == gs.vcf_file(t, ev, ref, DEFAULT)
    assert b"\t4294967\t.\tDP=" in got and b"AO=8589934590;SF=4294967295;SR=4294967295\tGT:DP:AD:GQ:PL\t" in got


# ---- the command line ----------------------------------------------------------------------------------------------------------

def test_options_of_the_parser():
    o = hostlib.parse_options(["slaMEM", "-vcf", "-gt", "ref.fa", "reads.fa"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"]
    o = hostlib.parse_options(["slaMEM", "ref.fa", "-ploidy", "1", "-err", "30", "-GT", "-hetq", "40", "reads.fa", "-qual", "10", "-VCF"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"]
    # -vcf without -gt is parsed as before
    o = hostlib.parse_options(["slaMEM", "ref.fa", "-evs", "1024", "-mdep", "3", "reads.fa", "-VCF"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"] and o["image_arg"] == -1
    L = hostlib.lib()
    L.slh_parse_gt_params.argtypes = [C.c_int, C.POINTER(C.c_char_p)] + [C.POINTER(C.c_int)] * 4

    def gt(args):
        argv = (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)
        v = [C.c_int() for _ in range(4)]
        return (L.slh_parse_gt_params(len(args), argv, *[C.byref(x) for x in v]),) + tuple(x.value for x in v)
    assert gt(["x", "-vcf", "-gt", "a", "b"]) == (0, 2, 20, 30, 20)
    assert gt(["x", "-PLOIDY", "1", "-err", "93", "-hetq", "0", "-qual", "999"]) == (1, 1, 93, 0, 999)
    assert gt(["x", "-err", "1", "-ext", "-pen", "3", "-evs", "64"]) == (1, 2, 1, 30, 20)
    for bad, code in ((["-ploidy", "0"], -1), (["-ploidy", "3"], -1), (["-ploidy"], -1), (["-ploidy", "2x"], -1), (["-err", "0"], -2),
                      (["-err", "94"], -2), (["-err"], -2), (["-hetq", "-1"], -3), (["-hetq", "1000"], -3), (["-qual", "1000"], -4),
                      (["-qual", "x"], -4), (["-qual"], -4)):
        assert gt(["x"] + bad)[0] == code, bad
    assert L.slh_parse_argument(3, (C.c_char_p * 4)(b"x", b"-vcf", b"-gt", None), b"GT", 0) == 1
    assert L.slh_parse_argument(2, (C.c_char_p * 3)(b"x", b"-vcf", None), b"GT", 0) == 0


def test_usage_lists_the_options():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    for opt in (b"\t-gt\t", b"\t-ploidy\t", b"\t-err\t", b"\t-hetq\t", b"\t-qual\t", b"\t-vcf\t", b"\t-evs\t"):
        assert opt in r.stdout


def write_fasta(path, records):
    with open(path, "wb") as f:
        for name, letters in records:
            f.write(b">" + name + b"\n" + bytes(letters) + b"\n")


REFUSALS = [
    (["-gt"], b"Option -gt needs -vcf"),
    (["-sites", "-gt"], b"Option -gt needs -vcf"),
    (["-cons", "-gt"], b"Option -gt needs -vcf"),
    (["-vcf", "-ploidy", "2"], b"Option -ploidy needs -gt"),
    (["-vcf", "-err", "20"], b"Option -err needs -gt"),
    (["-vcf", "-hetq", "30"], b"Option -hetq needs -gt"),
    (["-vcf", "-qual", "20"], b"Option -qual needs -gt"),
    (["-pile", "-qual", "20"], b"Option -qual needs -gt"),
    (["-vcf", "-gt", "-ploidy", "3"], b"Option -ploidy needs 1 or 2"),
    (["-vcf", "-gt", "-err", "0"], b"Option -err needs a whole number from 1 to 93"),
    (["-vcf", "-gt", "-err", "94"], b"Option -err needs a whole number from 1 to 93"),
    (["-vcf", "-gt", "-hetq", "1000"], b"Option -hetq needs a whole number from 0 to 999"),
    (["-vcf", "-gt", "-qual", "1000"], b"Option -qual needs a whole number from 0 to 999"),
    (["-vcf", "-gt", "-mpct", "30"], b"Option -mpct has no meaning with -gt: a call is made when its genotype's quality reaches -qual"),
    (["-vcf", "-gt", "-mdep", "0"], b"Option -mdep needs a whole number of at least 1"),
    # the wording of the earlier refusals stands
    (["-vcf", "-gt", "-sites"], b"Option -vcf excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile and -sites"),
    (["-cons", "-mpct", "30"], b"Option -mpct has no meaning with -cons: an allele is applied when more than half of the depth shows it"),
    (["-paf", "-mdep", "3"], b"Options -mdep and -mpct need -sites"),
    (["-sites", "-evs", "1024"], b"Option -evs needs -vcf"),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_cli_refusals_exit_before_any_gpu_work(args, message, tmp_path):
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"r", b"ACGT" * 30)])
    write_fasta(q_fa, [(b"q", b"ACGT" * 10)])
    r = subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))  # (no device: it never asks for one)
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout
    assert not os.path.exists(str(tmp_path / "ref-mems.txt"))
