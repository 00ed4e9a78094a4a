"""-sv on the CPU: the definition (tests/sv_spec.py) itself, without the engine -- splits written out by hand, the
planting rule, the order of the read-out -- then the catalogue of tests/sv_cases.py: from the oracle's MEM list and the specs alone
every designed read maps into its designed segments and yields exactly its designed junction or skip, three wrong rules each differ
from the definition on their family, and the random batch stores a junction for most of its planted reads."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import events_spec as es
import hostlib
import map_spec
import sites_spec
import sv_cases
import sv_spec as sv
from test_events_host import vcf_case, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")


# ---- the definition on texts written out by hand -----------------------------------------------------------------------------

def test_split_costs_and_the_smallest_t_of_least_cost():
    # a deletion of L = 7: A = "ACG" against B = "ACT" ... "TCG"; a's diagonal matches A[0:2], b's matches A[1:3]
    A, B = b"ACG", b"ACTGGGGTCG"
    assert sv.split_costs(A, B) == [1, 0, 0, 1]  # t = 1 and t = 2 are free: the smallest wins
    # an insertion: B = "AC", A = "AC" + "TTTT" + "AC": every split is free; the smallest wins
    assert sv.split_costs(b"ACTTTTAC", b"AC") == [0, 0, 0]
    # folded
    assert sv.split_costs(b"acg", B) == [1, 0, 0, 1]
    #      0123456789012345678901
    T = b"GGACTGGGGTCGAAGGCCTTAG"
    Q = b"GGACGAAGG"
    # a ends at (4, 4) [GGAC], b starts at (12, 5) [AAGG]: dr = 8, dq = 1 (the G), m = 1, L = 7
    # cost [0 (G on b's diagonal: T[11] = G), 1]: rows 4..10 = TGGGGTC are deleted, which is CTGGGGT from row 3 as well
    assert sv.classify(T, Q, 4, 4, 12, 5) == ("key", 3, 0, 7)
    assert sv.classify(T, Q, 4, 4, 12, 5, normalise=False) == ("key", 4, 0, 7)
    assert sv.classify(T, Q, 4, 4, 12, 4) == ("key", 4, 0, 8)        # m = 0: the break itself
    assert sv.classify(T, Q, 4, 4, 5, 5) == ("skip", 0)               # balanced
    assert sv.classify(T, b"GGACNAAGG", 4, 4, 12, 5) == ("skip", 2)   # a compared letter of the read
    assert sv.classify(T.replace(b"GGGG", b"GNGG"), Q, 4, 4, 12, 5) == ("skip", 2)  # a row of B
    assert sv.classify(T, b"GGACAAAGG", 4, 4, 12, 5, max_mis=0) == ("skip", 3)      # A fits neither diagonal
    assert sv.classify(T, b"GGACAAAGG", 4, 4, 12, 5, max_mis=1)[0] == "key"


def test_insertion_letters_rotate_through_the_text_without_being_kept():
    #      0123456789
    T = b"GATCACACTG"
    # AC inserted in front of row 8 (behind CACAC): walks to the first C at 3
    Q = b"GATCACACACTG"
    assert sv.classify(T, Q, 8, 8, 8, 10) == ("key", 3, 1, 2)
    assert sv.classify(T, Q, 8, 8, 8, 10, normalise=False) == ("key", 8, 1, 2)
    # the inserted letters are no part of the key: another insertion of the same length at a place that does not move
    t = sv.Table(T)
    t.observe(9, 1, 2, 1, 0)
    t.observe(9, 1, 2, 0, 2)
    assert t.junctions() == [(9, 1, 2, 1, 2)]


def test_planting_rule_read_out_order_and_filters():
    #      01234567890123456789
    T = b"GATTACAAAAAAAAGTCNAC"
    t = sv.Table(T)
    t.observe(10, 0, 2, 1, 0)       # a deletion inside the run of A (6..13) normalises to 6
    t.observe(6, 0, 2, 0, 3)
    t.observe(10, 1, 2, 1, 0)       # an insertion stays where it is given
    t.observe(6, 1, 200, 1, 1)      # any length
    t.observe(6, 0, 1, 2 ** 32 - 1, 0)
    t.observe(6, 0, 1, 2, 0)        # modulo 2^32
    t.observe(15, 0, 3, 1, 0)       # over the N
    t.observe(19, 0, 2, 0, 2)       # beyond n
    t.observe(20, 1, 1, 1, 0)       # at n
    t.observe(3, 2, 1, 1, 0)        # no such kind
    t.observe(3, 0, 0, 1, 0)        # no length
    t.observe(3, 0, 1, 0, 0)        # no observation
    assert t.skipped == [0, 0, 6, 0]
    assert t.junctions() == [(6, 0, 1, 1, 0), (6, 0, 2, 1, 3), (6, 1, 200, 1, 1), (10, 1, 2, 1, 0)]
    assert t.junctions(min_count=2) == [(6, 0, 2, 1, 3), (6, 1, 200, 1, 1)] and t.junctions(min_count=5) == []
    assert t.junctions(min_len=2) == [(6, 0, 2, 1, 3), (6, 1, 200, 1, 1), (10, 1, 2, 1, 0)] and t.junctions(min_len=201) == []
    assert t.junctions(7, 4) == [(10, 1, 2, 1, 0)] and t.junctions(7, 3) == [] and t.junctions(6, 1) == t.junctions()[:3]
    recs = sv.to_records(t.junctions())
    assert recs.dtype.itemsize == 24 and sv.from_records(recs) == t.junctions()


# ---- the catalogue -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mapped():
    """The catalogue's batch mapped by map_spec over the oracle's MEM list."""
    from oracle import pyoracle as po
    T, cases = sv_cases.catalogue()
    q, off = sv_cases.batch(cases)
    mem, counts = po.OracleIndex(bytes(T)).match_batch(q, off, sv_cases.MIN_LEN, True)
    boff = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    res = map_spec.filter_reads(mem, boff, T, q, off, True)
    return T, cases, q, off, res


def test_every_designed_read_maps_into_its_segments_and_yields_its_junction(mapped):
    T, cases, q, off, res = mapped
    Tb = bytes(T)
    assert len({c["name"] for c in cases}) == len(cases) == 21
    for i, c in enumerate(cases):
        for strand in (1, 2):
            r = 2 * i + strand - 1
            read = q[int(off[r]):int(off[r + 1])]
            assert res[r][0] == strand, (c["name"], strand, res[r][:4])
            assert len(res[r][4]) == c["segments"], (c["name"], strand, [s[:4] for s in res[r][4]])
            assert sv.read_junctions(res[r], read, Tb, 3) == c["expect"], (c["name"], strand)
            assert sv.read_junctions(res[r], read, Tb, 4) == c["expect4"], (c["name"], strand)
    for which, mis in (("expect", 3), ("expect4", 4)):
        assert sv.junctions(res, q, off, T, mis) == sv_cases.expected_table(cases, which)
    want, skipped = sv_cases.expected_table(cases)
    assert skipped[0] == 2 and skipped[1] == 0 and skipped[2] == 6 and skipped[3] == 4 and len(want) == 15
    assert any(k[1] == 1 for k in want) and all(k[3:] == (1, 1) for k in want)


def test_the_families_sit_on_their_edges(mapped):
    """What each family is there for, read off the mapping: the slop and the mismatches are the designed ones, the tandem
    deletion and the duplication move by more than 64 and by at least 40 rows, the closing deletion closes."""
    T, cases, q, off, res = mapped
    Tb = bytes(T)
    by = {c["name"]: i for i, c in enumerate(cases)}

    def slop_and_cost(name):
        i = by[name]
        asc = list(reversed(res[2 * i][4]))
        a, b = asc[0], asc[1]
        pe, qe, ps, qs = a[0] + a[2], a[1] + a[3], b[0], b[1]
        read = bytes(q[int(off[2 * i]):int(off[2 * i + 1])])
        return min(ps - pe, qs - qe), sv.split_costs(read[qe:qs], Tb[pe:ps])
    assert slop_and_cost("del300")[0] == 0
    for name, m, least in (("slop64", 64, 4), ("slop65", 65, 4), ("mis3", 60, 3), ("mis_a3", 3, 1), ("mis_b20", 20, 1)):
        got = slop_and_cost(name)
        assert (got[0], min(got[1])) == (m, least), (name, got[0], min(got[1]))
    for name in ("mis_a1", "mis_b1"):  # the ties
        assert slop_and_cost(name) == (1, [1, 1])
    for name, least_move in (("tandem", 65), ("dup40", 40)):
        i = by[name]
        read = q[int(off[2 * i]):int(off[2 * i + 1])]
        raw = sv.read_junctions(res[2 * i], read, Tb, normalise=False)
        assert raw[0][0] == "key" and raw[0][1] - cases[i]["expect"][0][1] >= least_move, (name, raw)
    i = by["del_maxed"]
    assert sum(k for c, k in res[2 * i][4][0][5] if c == "D") == sv_cases.MAXED


@pytest.mark.parametrize("rule,families", [
    (dict(tie="largest"), ("mis_a1", "mis_b1")),
    (dict(normalise=False), ("tandem", "dup40")),
    (dict(slop="query"), ("ins120",)),
])
def test_wrong_rules_differ_from_the_definition_on_their_family(mapped, rule, families):
    T, cases, q, off, res = mapped
    Tb = bytes(T)
    seen = 0
    for i, c in enumerate(cases):
        if c["name"] not in families:
            continue
        for r in (2 * i, 2 * i + 1):
            got = sv.read_junctions(res[r], q[int(off[r]):int(off[r + 1])], Tb, 3, **rule)
            assert got != c["expect"] and len(got) == len(c["expect"]), (c["name"], rule, got)
            seen += 1
    assert seen == 2 * len(families)


# ---- the random batch ----------------------------------------------------------------------------------------------------------

def test_random_batch_stores_a_junction_for_most_planted_reads():
    """Asserted on the CPU so that the GPU comparison of tests/test_gpu_sv.py cannot be one between empty tables."""
    from oracle import pyoracle as po
    T, q, off, plants = sv_cases.random_batch()
    assert len(plants) == 400 and all(130 <= L <= 2000 for _, _, L in plants) and {k for k, _, _ in plants} == {0, 1}
    mem, counts = po.OracleIndex(bytes(T)).match_batch(q, off, sv_cases.MIN_LEN, True)
    boff = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    res = map_spec.filter_reads(mem, boff, T, q, off, True)
    Tb = bytes(T)
    stored = 0
    for r, (kind, d, L) in enumerate(plants):
        got = sv.read_junctions(res[r], q[int(off[r]):int(off[r + 1])], Tb)
        want = es.normalise(Tb, d, 0, L)[0] if kind == 0 else None
        hit = [j for j in (got or []) if j[0] == "key" and j[2] == kind and j[3] == L and (kind == 1 or j[1] == want)]
        stored += 1 if hit else 0
    print("planted reads with their junction stored: %d of %d" % (stored, len(plants)))
    assert 4 * stored >= 3 * len(plants)
    table = sv.Table(T).add_batch(res, q, off)
    assert sum(c[0] + c[1] for c in table.keys.values()) + sum(table.skipped) == table.observed >= stored


# ---- the VCF lines ---------------------------------------------------------------------------------------------------------

def sv_vcf_case():
    """test_events_host.vcf_case (three records: rows 0..9, 11..20, 22..24) with junctions: at a POS with an SNV and events, at
    the call rule's equality, at a record's first row and on a separator, a deletion and an insertion of one key's place."""
    ref, t, ev = vcf_case()
    jn = [
        (3, 0, 40, 1, 1),     # anchor row 2 (d = 10): POS 3 behind the SNV and the two events; 2 of 10 is equality at mpct 20
        (3, 1, 40, 2, 0),     # the same place, an insertion: behind the deletion
        (3, 1, 2000, 0, 5),
        (4, 0, 35, 1, 0),     # anchor row 3 (d = 10): 1 of 10 is not called at 20
        (7, 1, 120, 3, 3),    # anchor row 6 (d = 10)
        (10, 0, 50, 9, 9),    # on the separator: no record's junction
        (11, 0, 33, 4, 4),    # the second record's first row: no anchor, no line
        (12, 1, 64, 0, 4),    # anchor row 11 (d = 20): POS 1, behind the events of POS 1
        (15, 0, 5, 5, 5),     # shorter than min_len 32: not written
        (15, 0, 32, 2 ** 32 - 1, 2 ** 32 - 1),
        (22, 1, 33, 1, 0),    # the third record's first row
    ]
    return ref, t, ev, sorted(jn)


def host_sv_vcf(ref, t, ev, jn, mdep, mpct, min_len):
    L = hostlib.lib()
    vp = C.c_void_p
    L.slh_format_vcf_sv_header.argtypes = [C.POINTER(hostlib.Buffer), C.POINTER(hostlib.Record), C.c_int]
    L.slh_format_vcf_sv_rows.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, vp, vp, vp, C.c_uint64,
                                         vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]
    recs = (hostlib.Record * len(ref.names))(*[hostlib.Record(nm, sz) for nm, sz in zip(ref.names, ref.sizes)])
    b = hostlib.Buffer()
    assert L.slh_format_vcf_sv_header(C.byref(b), recs, len(ref.names)) == 0
    pos, counts, alleles = sites_spec.sites(t, ref.chars, sites_spec.VARIANT, mdep, mpct)
    arr = es.to_records(ev)
    jarr = sv.to_records([j for j in jn if j[2] >= min_len])  # (the read-out's min_len is the command line's -svmin)
    counts_out = (C.c_uint64 * 2)()
    for r, name in enumerate(ref.names):
        a, size = int(ref.merged_start[r]), int(ref.sizes[r])
        mine = (pos >= a) & (pos < a + size)
        e = np.ascontiguousarray(arr[(arr["pos"] >= a) & (arr["pos"] < a + size)])
        j = np.ascontiguousarray(jarr[(jarr["pos"] >= a) & (jarr["pos"] < a + size)])
        anchors = [int(p) - 1 if int(p) > a else int(p) for p in e["pos"]]
        rows = np.ascontiguousarray(t[anchors].astype(np.uint32).reshape(len(anchors), 6))
        janchors = [max(int(p) - 1, 0) for p in j["pos"]]
        jrows = np.ascontiguousarray(t[janchors].astype(np.uint32).reshape(len(janchors), 6))
        p_, c_, a_ = (np.ascontiguousarray(x[mine]) for x in (pos, counts, alleles))
        assert L.slh_format_vcf_sv_rows(C.byref(b), name, a, size, ref.chars, p_.ctypes.data, c_.ctypes.data, a_.ctypes.data, len(p_),
                                        e.ctypes.data, rows.ctypes.data, len(e), j.ctypes.data, jrows.ctypes.data, len(j), mdep, mpct,
                                        C.addressof(counts_out)) == 0
    out = C.string_at(b.data, b.len) if b.len else b""
    L.slh_buffer_free(C.byref(b))
    return out, list(counts_out)


def test_sv_vcf_file_written_out_by_hand():
    ref, t, ev, jn = sv_vcf_case()
    got = sv.vcf_file(t, ev, jn, ref, 4, 20)
    head = sv.vcf_header(ref)
    assert got.startswith(head) and head.endswith(b'##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Inserted letters, or the deleted positions '
                                                  b'as a negative number">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
    assert head.count(b"##ALT=<ID=") == 2 and head.count(b"##INFO=<ID=") == 7 and head.replace(sv.VCF_HEADER_SV, b"") == es.vcf_header(ref)
    plain = es.vcf_file(t, ev, ref, 4, 20)[len(es.vcf_header(ref)):].split(b"\n")[:-1]
    body = got[len(head):].split(b"\n")[:-1]
    sv_lines = [ln for ln in body if b"SVTYPE=" in ln]
    assert [ln for ln in body if b"SVTYPE=" not in ln] == plain  # (the other lines are 4.18's, in their order)
    assert sv_lines == [b"first\t3\t.\tG\t<DEL>\t.\t.\tSVTYPE=DEL;END=43;SVLEN=-40;DP=10;AO=2;SF=1;SR=1",
                        b"first\t3\t.\tG\t<INS>\t.\t.\tSVTYPE=INS;END=3;SVLEN=40;DP=10;AO=2;SF=2;SR=0",
                        b"first\t3\t.\tG\t<INS>\t.\t.\tSVTYPE=INS;END=3;SVLEN=2000;DP=10;AO=5;SF=0;SR=5",
                        b"first\t7\t.\tC\t<INS>\t.\t.\tSVTYPE=INS;END=7;SVLEN=120;DP=10;AO=6;SF=3;SR=3",
                        b"second\t1\t.\tG\t<INS>\t.\t.\tSVTYPE=INS;END=1;SVLEN=64;DP=20;AO=4;SF=0;SR=4",
                        b"second\t4\t.\tT\t<DEL>\t.\t.\tSVTYPE=DEL;END=36;SVLEN=-32;DP=10;AO=8589934590;SF=4294967295;SR=4294967295"]
    # at one POS: the SNV, the events, then the junctions
    at3 = [ln for ln in body if ln.startswith(b"first\t3\t")]
    assert [b"SVTYPE" in ln for ln in at3] == [False, False, False, True, True, True]
    assert b"SVLEN=-5;" in sv.vcf_file(t, ev, jn, ref, 4, 20, min_len=5) and b"SVLEN=-35" in sv.vcf_file(t, ev, jn, ref, 4, 10)
    assert b"SVLEN=-40" not in sv.vcf_file(t, ev, jn, ref, 4, 21)


@pytest.mark.parametrize("mdep,mpct,min_len", [(4, 20, 32), (4, 21, 32), (11, 0, 32), (1, 0, 1), (2, 100, 33), (4, 10, 41)])
def test_host_sv_formatter_against_the_spec(mdep, mpct, min_len):
    ref, t, ev, jn = sv_vcf_case()
    got, counts = host_sv_vcf(ref, t, ev, jn, mdep, mpct, min_len)
    want = sv.vcf_file(t, ev, jn, ref, mdep, mpct, min_len)
    assert got == want
    assert counts == [want.count(b"SVTYPE="), sum(1 for j in jn if j[2] >= min_len and j[0] in (0, 11, 22))]


# ---- the command line ----------------------------------------------------------------------------------------------------------

def test_options_of_the_parser():
    L = hostlib.lib()
    L.slh_parse_sv.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]

    def parse(args):
        argv = (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)
        a, b, c = C.c_int(), C.c_int(), C.c_uint64()
        return L.slh_parse_sv(len(args), argv, C.byref(a), C.byref(b), C.byref(c)), a.value, b.value, c.value
    assert parse(["x", "-vcf", "a", "b"]) == (0, -1, 3, 0)
    assert parse(["x", "a", "-sv", "b", "-vcf"]) == (1, -1, 3, 0) and parse(["x", "-SV"])[0] == 1
    assert parse(["x", "-sv", "-svmin", "50", "-SVMIS", "0", "-svslots", "64"]) == (15, 50, 0, 64)
    assert parse(["x", "-svmin", "50"]) == (2, 50, 3, 0) and parse(["x", "-svmis", "64"]) == (4, -1, 64, 0)
    for bad, rc in ((["-svmin", "0"], -2), (["-svmin", "x"], -2), (["-svmin"], -2), (["-svmis", "65"], -3), (["-svmis", "-1"], -3),
                    (["-svslots", "63"], -4), (["-svslots", "100"], -4), (["-svslots", "32"], -4), (["-svslots", "4294967296"], -4)):
        assert parse(["x", "-sv"] + bad)[0] == rc, bad
    # no other option is one of the four, and none of them is another: the names that begin alike
    for other in ("-s", "-sam", "-sb", "-sites", "-smem", "-stats", "-svx", "-svm", "-svmi", "-svmins", "-svslot"):
        assert parse(["x", other, "a", "b"])[0] == 0, other
    rows = dict(hostlib.option_rows())
    assert rows["sv"] is False and rows["svmin"] is True and rows["svmis"] is True and rows["svslots"] is True
    o = hostlib.parse_options(["slaMEM", "ref.fa", "-sv", "reads.fa", "-vcf", "-svmin", "40"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"]
    assert hostlib.parse_options(["slaMEM", "-sv", "ref.fa", "reads.fa"])["match_type"] == 0  # (-sv is no mode of its own)


def test_usage_lists_the_options():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    for opt in (b"\t-sv\t", b"\t-svmin\t", b"\t-svmis\t", b"\t-svslots\t"):
        assert opt in r.stdout


REFUSALS = [
    (["-sv"], b"Option -sv needs -vcf"),
    (["-sites", "-sv"], b"Option -sv needs -vcf"),
    (["-cons", "-sv"], b"Option -sv needs -vcf"),
    (["-vcf", "-svmin", "40"], b"Option -svmin needs -sv"),
    (["-vcf", "-svmis", "2"], b"Option -svmis needs -sv"),
    (["-svslots", "64", "-vcf"], b"Option -svslots needs -sv"),
    (["-vcf", "-gt", "-sv"], b"Option -sv excludes -gt"),
    (["-sv", "-vcf", "-svmin", "0"], b"Option -svmin needs a whole number of at least 1"),
    (["-sv", "-vcf", "-svmis", "65"], b"Option -svmis needs a whole number from 0 to 64"),
    (["-sv", "-vcf", "-svslots", "96"], b"Option -svslots needs a power of two of at least 64"),
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
