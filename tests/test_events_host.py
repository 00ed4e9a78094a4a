"""-vcf on the CPU: the definition (tests/events_spec.py) itself, without the engine -- normalisation on texts
written out by hand, the order of the read-out, the packing of the letters -- then the host library's VCF formatter against the
spec, and the refusals of the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import events_spec as es
import hostlib
import pile_spec
from test_map_host import FakeRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")

#          0         1         2         3         4
#          0123456789012345678901234567890123456789012345
TEXT = b"GATTACAAAAAAAAGTCACACACACGTNAAACCGGTTcacaCAGT"
#        run of A: 6..13; (AC) repeat: 16..24 = CACACACAC; N at 27; AAA right behind it; lower-case caca at 37..40


def test_normalisation_inside_a_homopolymer_lands_on_one_key():
    # a deletion of two A anywhere in the run 6..13 (GATTAC|AAAAAAAA|GT; row 5 is C)
    keys = {es.normalise(TEXT, p, 0, 2) for p in range(6, 13)}
    assert keys == {(6, b"")}
    # an insertion of AA in front of any row of the run, and right behind it
    assert {es.normalise(TEXT, p, 1, 2, b"AA") for p in range(6, 15)} == {(6, b"AA")}
    # ... and of a single A
    assert {es.normalise(TEXT, p, 1, 1, b"A") for p in range(6, 15)} == {(6, b"A")}
    # another letter does not move
    assert es.normalise(TEXT, 9, 1, 1, b"C") == (9, b"C")


def test_normalisation_inside_a_tandem_repeat_rotates_the_letters():
    # TEXT[15:25] = TCACACACAC: the unit CA from 16; a deletion of one unit anywhere lands on 16
    assert TEXT[16:25] == b"CACACACAC"
    assert {es.normalise(TEXT, p, 0, 2) for p in range(16, 24)} == {(16, b"")}
    # an inserted unit: CA in front of 18 is AC in front of 17 is CA in front of 16
    assert es.normalise(TEXT, 18, 1, 2, b"CA") == (16, b"CA")
    assert es.normalise(TEXT, 17, 1, 2, b"AC") == (16, b"CA")
    assert es.normalise(TEXT, 25, 1, 2, b"AC") == (16, b"CA")
    # lower case folds: caca at 37..40 then CA: a deletion of CA at 41 goes back to 37 (row 36 is T)
    assert es.normalise(TEXT, 41, 0, 2) == (37, b"")
    assert es.normalise(TEXT, 43, 1, 2, b"CA") == (37, b"CA")


def test_normalisation_stops_at_a_separator_and_at_row_0_and_is_idempotent():
    # AAA behind the N at 27: a deletion of one A at 30 stops at 28
    assert es.normalise(TEXT, 30, 0, 1) == (28, b"")
    assert es.normalise(TEXT, 30, 1, 1, b"A") == (28, b"A")
    # row 0
    t = b"AAAACGT"
    assert es.normalise(t, 3, 0, 1) == (0, b"") and es.normalise(t, 4, 1, 2, b"AA") == (0, b"AA")
    rng = np.random.default_rng(1)
    text = bytes(rng.choice(np.frombuffer(b"ACGTacN", dtype=np.uint8), size=400, p=[.3, .3, .15, .15, .04, .04, .02]))
    for _ in range(300):
        kind = int(rng.integers(0, 2))
        k = int(rng.integers(1, 6))
        p = int(rng.integers(0, len(text) - k))
        S = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=k)) if kind else b""
        if es.which_skip(text, p, kind, k, S) is not None:
            continue
        p1, S1 = es.normalise(text, p, kind, k, S)
        assert es.normalise(text, p1, kind, k, S1) == (p1, S1) and p1 <= p
        assert es.which_skip(text, p1, kind, k, S1) is None  # (the canonical form is a valid event)
        if kind == 0:  # the same haplotype: the text without the rows
            assert es.fold(text[:p] + text[p + k:]) == es.fold(text[:p1] + text[p1 + k:])
        else:
            assert es.fold(text[:p] + S + text[p:]) == es.fold(text[:p1] + S1 + text[p1:])


def test_skips_and_counts():
    t = es.Table(TEXT)
    t.observe(9, 1, 32, b"A" * 32, 1, 0)        # too long: [0], whatever else is wrong with it
    t.observe(len(TEXT), 1, 33, b"A" * 33, 0, 2)
    t.observe(9, 1, 2, b"AN", 1, 0)             # a letter outside A,C,G,T
    t.observe(len(TEXT), 1, 1, b"A", 1, 0)      # at n
    t.observe(26, 0, 3, b"", 1, 0)              # over the N
    t.observe(len(TEXT) - 2, 0, 3, b"", 0, 1)   # beyond n
    t.observe(2, 0, 128, b"", 1, 0)
    t.observe(9, 0, 2, b"", 0, 0)               # no observation
    assert t.skipped == [3, 0, 5] and t.keys == {}
    t.observe(9, 0, 2, b"", 2, 1)
    t.observe(12, 0, 2, b"", 0, 5)
    t.observe(8, 1, 1, b"A", 2 ** 32 - 1, 0)
    t.observe(8, 1, 1, b"A", 3, 0)              # modulo 2^32
    assert t.events() == [(6, 0, 2, b"", 2, 6), (6, 1, 1, b"A", 2, 0)]
    assert t.events(min_count=3) == [(6, 0, 2, b"", 2, 6)] and t.events(min_count=8) == [(6, 0, 2, b"", 2, 6)] and t.events(min_count=9) == []
    assert t.events(6, 1) == t.events() and t.events(7, 10) == [] and t.events(0, 6) == [] and t.events(6, 0) == []


def test_order_of_the_read_out():
    text = bytearray(b"GCGCGCGTGCATGCATGCAT" * 3)
    text[29] = ord("N")  # (whatever is planted at 30 stays there)
    t = es.Table(bytes(text))
    plants = [(30, 1, 2, b"TT"), (30, 1, 2, b"AG"), (30, 1, 2, b"AC"), (30, 1, 1, b"T"), (30, 0, 3, b""), (30, 0, 1, b""), (30, 1, 3, b"AAA"),
              (12, 1, 1, b"A"), (31, 0, 1, b"")]
    for p, kind, k, S in plants:
        assert es.normalise(t.T, p, kind, k, S) == (p, S)
        t.observe(p, kind, k, S, 1, 0)
    got = [e[:4] for e in t.events()]
    assert got == [(12, 1, 1, b"A"), (30, 0, 1, b""), (30, 0, 3, b""), (30, 1, 1, b"T"), (30, 1, 2, b"AC"), (30, 1, 2, b"AG"), (30, 1, 2, b"TT"),
                   (30, 1, 3, b"AAA"), (31, 0, 1, b"")]


def test_packing_of_the_letters_is_invertible_and_keeps_the_order():
    assert es.pack_letters(b"A") == 0 and es.pack_letters(b"T") == 3 and es.pack_letters(b"CA") == 4 and es.pack_letters(b"AC") == 1
    rng = np.random.default_rng(2)
    for k in (1, 2, 31):
        words = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=k)) for _ in range(50)] + [b"A" * k, b"T" * k]
        for w in words:
            v = es.pack_letters(w)
            assert 0 <= v < 4 ** k and es.unpack_letters(v, k) == w
        assert sorted(words, key=es.pack_letters) == sorted(words, key=lambda w: tuple(b"ACGT".index(c) for c in w))
    assert es.pack_letters(b"T" * 31) == 2 ** 62 - 1  # (bit 63 is the marker's, bit 62 stays free)
    recs = es.to_records([(5, 1, 31, b"ACGT" * 7 + b"ACG", 7, 9), (6, 0, 127, b"", 1, 0)])
    assert recs.dtype.itemsize == 32 and es.from_records(recs) == [(5, 1, 31, b"ACGT" * 7 + b"ACG", 7, 9), (6, 0, 127, b"", 1, 0)]


# ---- a known answer ------------------------------------------------------------------------------------------------------------

def planted_deletion(seed: int = 77, n: int = 3000, read_len: int = 150):
    """A random reference with a run of eight A from 1500 (C in front, G behind), a sample genome without three of them, and 20
    error-free reads of the sample that hold the place at least 40 letters from either end, alternating strands.  Returns
    (reference, the run's first position, reads, offsets)."""
    import ext_spec
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=n)
    run = 1500
    ref[run - 1], ref[run:run + 8], ref[run + 8] = ord("C"), ord("A"), ord("G")
    sample = np.delete(ref, [run + 2, run + 3, run + 4])
    reads = []
    for k in range(20):
        r = sample[1390 + 3 * k:1390 + 3 * k + read_len]
        reads.append(ext_spec.revcomp(r) if k % 2 else r.copy())
    off = np.arange(len(reads) + 1, dtype=np.uint64) * np.uint64(read_len)
    return ref, run, np.concatenate(reads), off


def test_planted_deletion_answer_holds_on_the_definition():
    """The known answer of test_gpu_events.py, on the CPU: map_spec.filter_reads over the oracle's MEM list, its events by
    events_spec: one deletion of 3 at the run's first letter, 10 observations a strand."""
    import map_spec
    from oracle import pyoracle as po
    ref, run, q, off = planted_deletion()
    mem, counts = po.OracleIndex(bytes(ref)).match_batch(q, off, 20, True)
    boff = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    res = map_spec.filter_reads(mem, boff, ref, q, off, True)
    assert all(r[0] == 1 + k % 2 for k, r in enumerate(res))
    assert es.events(res, q, off, ref) == ([(run, 0, 3, b"", 10, 10)], [0, 0, 0])


# ---- the VCF lines ---------------------------------------------------------------------------------------------------------

def vcf_case():
    """Two records (the second begins with a lower-case letter) and a third that a deletion empties to its end."""
    recs = [b"ACGTTGCAAC", b"gGATCCATAG", b"TTT"]
    ref = FakeRef(recs, [b"first one", b"second\tx", b"third"])
    n = len(ref.chars)  # 10 + 1 + 10 + 1 + 3: separators at 10 and 21
    t = pile_spec.empty(n)
    t[0] = (8, 2, 0, 0, 0, 0)       # A with C
    t[2] = (1, 1, 6, 2, 0, 0)       # G with A, C, T: the SNVs of POS 3 in ALT order
    t[3] = (0, 0, 0, 10, 0, 0)
    t[4] = (0, 0, 0, 6, 4, 0)       # D alone: no SNV line
    t[6] = (0, 10, 0, 0, 0, 3)      # I alone: no SNV line
    t[10] = (0, 0, 0, 0, 5, 0)      # the separator
    t[11] = (0, 0, 20, 0, 0, 0)     # g: the anchor of the events at the second record's start
    t[12] = (0, 0, 16, 0, 4, 0)
    t[14] = (5, 0, 0, 5, 0, 0)      # T with A, and events anchored here (POS 4 of the second record)
    t[22] = (0, 0, 0, 4, 0, 0)
    ev = [
        (3, 0, 1, b"", 3, 1),        # x > 0: anchor row 2 (d = 10), 4 of 10
        (3, 1, 2, b"GA", 1, 1),      # the same POS: 2 of 10 -- equality at mpct 20
        (4, 0, 2, b"", 1, 0),        # anchor row 3, d = 10: 1 of 10 is not called at 20
        (7, 1, 31, b"ACGT" * 7 + b"ACG", 2, 1),  # anchor row 6 (d = 10)
        (10, 1, 1, b"A", 9, 9),      # on the separator: no record's event
        (11, 0, 2, b"", 2, 2),       # x == 0: the following base anchors; depth of row 11
        (11, 1, 3, b"TTA", 0, 4),    # x == 0
        (12, 0, 1, b"", 4, 0),       # x == 1: anchor row 11, POS 1 as well, behind the x == 0 events
        (15, 1, 1, b"C", 1, 1),      # anchor row 14 (d = 10): POS 4, behind the SNV of row 14
        (15, 0, 3, b"", 2, 0),
        (22, 0, 3, b"", 3, 0),       # x == 0 and the record ends with it: omitted
        (22, 0, 2, b"", 3, 0),       # x == 0, one letter left
    ]
    return ref, t, sorted(ev, key=es.order_key)


def host_vcf(ref, t, ev, mdep, mpct) -> bytes:
    import sites_spec
    L = hostlib.lib()
    L.slh_format_vcf_header.argtypes = [C.POINTER(hostlib.Buffer), C.POINTER(hostlib.Record), C.c_int]
    L.slh_format_vcf_rows.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    recs = (hostlib.Record * len(ref.names))(*[hostlib.Record(nm, sz) for nm, sz in zip(ref.names, ref.sizes)])
    b = hostlib.Buffer()
    assert L.slh_format_vcf_header(C.byref(b), recs, len(ref.names)) == 0
    pos, counts, alleles = sites_spec.sites(t, ref.chars, sites_spec.VARIANT, mdep, mpct)
    arr = es.to_records(ev)
    for r, name in enumerate(ref.names):
        a, size = int(ref.merged_start[r]), int(ref.sizes[r])
        mine = (pos >= a) & (pos < a + size)
        emine = (arr["pos"] >= a) & (arr["pos"] < a + size)
        e = np.ascontiguousarray(arr[emine])
        anchors = [int(p) - 1 if int(p) > a else int(p) for p in e["pos"]]
        rows = np.ascontiguousarray(t[anchors].astype(np.uint32).reshape(len(anchors), 6))
        p_, c_, a_ = (np.ascontiguousarray(x[mine]) for x in (pos, counts, alleles))
        assert L.slh_format_vcf_rows(C.byref(b), name, a, size, ref.chars, p_.ctypes.data, c_.ctypes.data, a_.ctypes.data, len(p_),
                                     e.ctypes.data, rows.ctypes.data, len(e), mdep, mpct) == 0
    out = C.string_at(b.data, b.len) if b.len else b""
    L.slh_buffer_free(C.byref(b))
    return out


def test_vcf_file_written_out_by_hand():
    ref, t, ev = vcf_case()
    got = es.vcf_file(t, ev, ref, 4, 20)
    head = es.vcf_header(ref)
    assert head.startswith(b"##fileformat=VCFv4.2\n##contig=<ID=first,length=10>\n##contig=<ID=second,length=10>\n##contig=<ID=third,length=3>\n##INFO=<ID=DP,")
    assert head.endswith(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n") and head.count(b"##INFO=<ID=") == 4
    body = got[len(head):]
    assert body == (b"first\t1\t.\tA\tC\t.\t.\tDP=10;AO=2\n"
                    b"first\t3\t.\tG\tT\t.\t.\tDP=10;AO=2\n"          # A and C have 1 of 10: below 20 percent
                    b"first\t3\t.\tGT\tG\t.\t.\tDP=10;AO=4;SF=3;SR=1\n"
                    b"first\t3\t.\tG\tGGA\t.\t.\tDP=10;AO=2;SF=1;SR=1\n"
                    b"first\t7\t.\tC\tCACGTACGTACGTACGTACGTACGTACGTACG\t.\t.\tDP=10;AO=3;SF=2;SR=1\n"
                    b"second\t1\t.\tGGA\tA\t.\t.\tDP=20;AO=4;SF=2;SR=2\n"
                    b"second\t1\t.\tG\tTTAG\t.\t.\tDP=20;AO=4;SF=0;SR=4\n"
                    b"second\t1\t.\tGG\tG\t.\t.\tDP=20;AO=4;SF=4;SR=0\n"
                    b"second\t4\t.\tT\tA\t.\t.\tDP=10;AO=5\n"
                    b"second\t4\t.\tTCCA\tT\t.\t.\tDP=10;AO=2;SF=2;SR=0\n"
                    b"second\t4\t.\tT\tTC\t.\t.\tDP=10;AO=2;SF=1;SR=1\n"
                    b"third\t1\t.\tTTT\tT\t.\t.\tDP=4;AO=3;SF=3;SR=0\n")
    # thresholds at equality and one off: 2 of 10 is 20 percent; depth 4 is the third record's
    assert b"GGA\t" in es.vcf_file(t, ev, ref, 4, 20) and b"\tGGA\t" not in es.vcf_file(t, ev, ref, 4, 21)
    assert b"third" in es.vcf_file(t, ev, ref, 4, 20)[len(head):] and b"third" not in es.vcf_file(t, ev, ref, 5, 20)[len(head):]
    # rows with only D / I bits give no SNV line, whatever the thresholds
    loose = es.vcf_file(t, ev, ref, 1, 0)[len(head):]
    assert b"first\t5\t" not in loose.replace(b"first\t5\t.\tT", b"") and b"first\t7\t.\tC\tA" not in loose
    assert b"first\t4\t.\tTTG\tT\t" in loose  # (the event that 20 percent left out)


@pytest.mark.parametrize("mdep,mpct", [(4, 20), (4, 21), (5, 20), (1, 0), (11, 0), (2, 100)])
def test_host_formatter_against_the_spec(mdep, mpct):
    ref, t, ev = vcf_case()
    assert host_vcf(ref, t, ev, mdep, mpct) == es.vcf_file(t, ev, ref, mdep, mpct)


def test_host_formatter_large_counters_and_a_long_deletion():
    rng = np.random.default_rng(4)
    body = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=400))
    ref = FakeRef([body], [b"chr 1"])
    t = pile_spec.empty(len(body))
    t[99] = (2 ** 32 - 1,) * 6
    t[100] = (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 0)
    ev = []
    p, _ = es.normalise(body, 100, 0, 127)
    ev.append((p, 0, 127, b"", 2 ** 32 - 1, 2 ** 32 - 1))
    t[p - 1] = (2 ** 32 - 1,) * 6
    assert host_vcf(ref, t, ev, 1, 0) == es.vcf_file(t, ev, ref, 1, 0)
    assert b"AO=8589934590;SF=4294967295;SR=4294967295" in host_vcf(ref, t, ev, 1, 0) and b"DP=21474836475;" in host_vcf(ref, t, ev, 1, 0)


# ---- the command line ----------------------------------------------------------------------------------------------------------

def test_options_of_the_parser():
    o = hostlib.parse_options(["slaMEM", "-vcf", "ref.fa", "reads.fa"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"] and o["image_arg"] == -1
    o = hostlib.parse_options(["slaMEM", "ref.fa", "-evs", "1024", "-mdep", "3", "reads.fa", "-VCF"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"]
    # -v alone is still the image tool and still takes a value
    o = hostlib.parse_options(["slaMEM", "-v", "mems.txt", "ref.fa", "reads.fa"])
    assert o["image_arg"] == 2 and o["files"] == ["ref.fa", "reads.fa"] and o["match_type"] == 0
    for other in ("-mam", "-mum", "-smem", "-chain", "-ext", "-aln", "-paf", "-pile", "-sites"):
        assert hostlib.parse_options(["slaMEM", "ref.fa", other, "reads.fa", "-vcf"])["match_type"] == -1
    L = hostlib.lib()
    L.slh_parse_event_slots.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)]

    def slots(args):
        argv = (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)
        v = C.c_uint64()
        return L.slh_parse_event_slots(len(args), argv, C.byref(v)), v.value
    assert slots(["x", "-vcf", "a", "b"]) == (0, 0)
    assert slots(["x", "-evs", "64"]) == (1, 64) and slots(["x", "-EVS", "2147483648", "-vcf"]) == (1, 2 ** 31)
    assert slots(["x", "-ext", "-vcf"]) == (0, 0)
    for bad in (["-evs", "63"], ["-evs", "32"], ["-evs", "100"], ["-evs", "0"], ["-evs", "-64"], ["-evs", "64x"], ["-evs", "4294967296"], ["-evs"]):
        assert slots(["x"] + bad)[0] == -1, bad


def test_usage_lists_the_options():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    for opt in (b"\t-vcf\t", b"\t-evs\t", b"\t-sites\t", b"\t-v\t"):
        assert opt in r.stdout


def write_fasta(path, records):
    with open(path, "wb") as f:
        for name, letters in records:
            f.write(b">" + name + b"\n" + bytes(letters) + b"\n")


VCF_EXCLUDES = b"Option -vcf excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile and -sites"
REFUSALS = [
    (["-vcf", "-sites"], VCF_EXCLUDES),
    (["-pile", "-vcf"], VCF_EXCLUDES),
    (["-vcf", "-paf"], VCF_EXCLUDES),
    (["-mam", "-vcf"], VCF_EXCLUDES),
    (["-sites", "-evs", "1024"], b"Option -evs needs -vcf"),
    (["-evs", "1024"], b"Option -evs needs -vcf"),
    (["-vcf", "-evs", "100"], b"Option -evs needs a power of two of at least 64"),
    (["-vcf", "-evs", "32"], b"Option -evs needs a power of two of at least 64"),
    (["-vcf", "-mdep", "0"], b"Option -mdep needs a whole number of at least 1"),
    (["-vcf", "-mpct", "101"], b"Option -mpct needs a whole number from 0 to 100"),
    (["-vcf", "-minq", "61"], b"Option -minq needs a whole number from 0 to 60"),
    # the wording of the earlier refusals stands
    (["-pile", "-sites"], b"Option -sites excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf and -pile"),
    (["-paf", "-mdep", "3"], b"Options -mdep and -mpct need -sites"),
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
