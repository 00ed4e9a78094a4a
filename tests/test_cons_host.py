"""-cons without a GPU: tests/cons_spec.py (the definition of DESIGN.md 4.19) on tables worked out by hand, the property that a
range's consensus is a slice of the whole text's, the FASTA record writer of the front end against the spec's, and the options."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cons_spec as cs
import events_spec as es
import hostlib
from test_events_host import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")


def table_of(text, rows, default=None):
    t = np.zeros((len(text), 6), dtype=np.int64)
    if default is not None:
        for p, c in enumerate(text):
            if es.is_acgt(c):
                t[p][b"ACGT".index(bytes([c & 0xDF]))] = default
    for p, r in rows.items():
        t[p] = r
    return t


def test_rows_without_events_every_rule_and_tie():
    #        0123456789 1
    text = b"ACGTNACGTAcg"
    t = table_of(text, {
        0: [5, 0, 0, 0, 0, 0],   # A: the plurality is the text's letter
        1: [3, 0, 0, 0, 0, 0],   # C: called A
        2: [2, 0, 2, 0, 0, 0],   # G: A and G tie, the text's letter is among them
        3: [0, 2, 2, 0, 0, 0],   # T: C and G tie, the text's letter is not: the first, C
        4: [9, 0, 0, 0, 0, 0],   # N whatever the counters say
        5: [1, 0, 0, 0, 0, 0],   # A: depth 1 < 2
        6: [0, 0, 0, 0, 5, 0],   # C: deep enough, but no letter was seen
        7: [0, 1, 0, 0, 1, 0],   # G: depth 2 with the D column, called C
        9: [0, 0, 0, 3, 0, 7],   # A: called T; the I column plays no part
        10: [0, 4, 0, 0, 0, 0],  # c: a called row is in upper case
    })
    seq, offs, stats = cs.consensus(text, t, [], 2, bounds=[0, 5, 12])
    assert seq == b"AAGCNacCtTCg" and offs == [0, 5, 12] and stats == [4, 4, 0, 0, 0]
    assert [cs.row(text, t, p, 2)[2] for p in (0, 2, 3)] == ["", "own", "first"]
    # a larger least depth leaves more rows uncalled; the letter N stays
    assert cs.consensus(text, t, [], 4)[0] == b"AcGCNacgtaCg"
    assert cs.consensus(text, t, [], 2 ** 31 - 1)[0] == b"acgtNacgtacg"


def event_case():
    #        01234567890123456
    text = b"ACGTACGTNACGTACGT"
    t = table_of(text, {15: [0, 0, 2, 0, 0, 0]}, default=10)
    ev = [
        (0, 0, 1, b"", 6, 0),      # anchor: row 0 itself; row 0 goes
        (2, 1, 1, b"A", 3, 3),     # a tie of 6 observations at row 2: the first in the read-out's order, A
        (2, 1, 2, b"TT", 6, 0),
        (3, 0, 2, b"", 6, 0),      # rows 3 and 4 go
        (4, 1, 1, b"C", 9, 0),     # in front of a deleted row: emitted
        (5, 1, 1, b"G", 6, 0),
        (5, 1, 1, b"T", 5, 0),     # 2 * 5 is not more than 10
        (5, 1, 3, b"CAT", 4, 4),   # the most observations at row 5
        (9, 1, 2, b"GG", 6, 0),    # a record's first row: row 8 is no A,C,G,T, the anchor is row 9
        (11, 0, 3, b"", 6, 0),     # rows 11..13 and 12..14: the union goes
        (12, 0, 3, b"", 0, 7),
        (16, 1, 1, b"A", 2, 0),    # the anchor's depth is 2 < 4
    ]
    assert ev == sorted(ev, key=es.order_key)
    return text, t, ev


def test_events_written_out_by_hand():
    text, t, ev = event_case()
    seq, offs, stats = cs.consensus(text, t, ev, 4, bounds=[0, 2, 3, 9, 17])
    assert seq == b"CAGCCATCGTNGGACgT"
    assert offs == [0, 1, 3, 11, 17] and stats == [1, 0, 7, 4, 7]
    assert [cs.anchor(text, p) for p in (0, 1, 8, 9, 10)] == [0, 0, 7, 9, 9]
    # with a least depth of 1 the last insertion is applied too and row 15 is called
    assert cs.consensus(text, t, ev, 1)[0] == b"CAGCCATCGTNGGACGAT"
    # no events: the table alone
    assert cs.consensus(text, t, [], 4)[0] == b"ACGTACGTNACGTACgT"
    # the file: two records, the separator's row left out
    class Ref:
        pass
    ref, ref.s = Ref(), Ref()
    ref.s.num, ref.chars, ref.names, ref.sizes, ref.merged_start = 2, text, [b"one first", b"two\tsecond"], [8, 8], [0, 9]
    assert cs.fasta_file(t, ev, ref, 4) == b">one\nCAGCCATCGT\n>two\nGGACgT\n"


def random_case(rng):
    n = int(rng.integers(8, 41))
    text = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=n, p=[.2, .2, .2, .2, .04, .04, .04, .04, .04]))
    t = rng.integers(0, 4, size=(n, 6)) * rng.integers(0, 3, size=(n, 1))
    ev = []
    for _ in range(int(rng.integers(0, 12))):
        pos, kind = int(rng.integers(0, n)), int(rng.integers(0, 2))
        k = int(rng.integers(1, 4))
        if kind == 0 and pos + k > n:
            continue
        S = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=k)) if kind else b""
        ev.append((pos, kind, k, S, int(rng.integers(0, 5)), int(rng.integers(0, 5))))
    ev = sorted({e[:4]: e for e in ev}.values(), key=es.order_key)
    return text, t, ev


def test_any_range_is_a_slice_of_the_whole():
    rng = np.random.default_rng(191)
    seen = set()
    for _ in range(200):
        text, t, ev = random_case(rng)
        n = len(text)
        md = int(rng.integers(1, 6))
        whole, offs, stats = cs.consensus(text, t, ev, md, bounds=range(n + 1))
        assert offs[0] == 0 and offs[n] == len(whole) and offs == sorted(offs)
        assert stats[4] + n - stats[2] == len(whole)
        seen.update(r for _, r, _ in cs.emissions(text, t, ev, md))
        seen.update(["ins"] if stats[3] else [])
        for first, count in [(0, 0), (n, 0), (0, n)] + [(int(a), int(rng.integers(0, n - a + 1))) for a in rng.integers(0, n + 1, size=6)]:
            b = list(range(first, first + count + 1))
            part, poffs, pstats = cs.consensus(text, t, ev, md, first, count, bounds=b)
            assert part == whole[offs[first]:offs[first + count]]
            assert poffs == [offs[x] - offs[first] for x in b]
            rest = cs.consensus(text, t, ev, md, first + count, n - first - count)[2]
            head = cs.consensus(text, t, ev, md, 0, first)[2]
            assert [a + b_ + c for a, b_, c in zip(head, pstats, rest)] == stats
    assert seen == set(cs.RULES) | {"ins"}


def host_record(name: bytes, letters: bytes) -> bytes:
    L = hostlib.lib()
    L.slh_format_fasta_record.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_char_p, C.c_uint64]
    b = hostlib.Buffer()
    assert L.slh_format_fasta_record(C.byref(b), name, letters, len(letters)) == 0
    out = C.string_at(b.data, b.len)
    L.slh_buffer_free(C.byref(b))
    return out


@pytest.mark.parametrize("length", [0, 59, 60, 61, 120])
def test_host_fasta_record_against_the_spec(length):
    rng = np.random.default_rng(length)
    letters = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=length))
    got = host_record(b"chr1 the first\tone", letters)
    assert got == cs.fasta_record(b"chr1 the first\tone", letters)
    assert got.startswith(b">chr1\n") and got.count(b"\n") == 1 + (length + 59) // 60
    assert host_record(b"a\tb", letters) == cs.fasta_record(b"a\tb", letters)
    # records follow each other in one buffer
    L = hostlib.lib()
    b = hostlib.Buffer()
    for name in (b"x", b"y z"):
        assert L.slh_format_fasta_record(C.byref(b), name, letters, len(letters)) == 0
    both = C.string_at(b.data, b.len)
    L.slh_buffer_free(C.byref(b))
    assert both == cs.fasta_record(b"x", letters) + cs.fasta_record(b"y z", letters)


def test_options_of_the_parser():
    o = hostlib.parse_options(["slaMEM", "-cons", "ref.fa", "reads.fa"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"] and o["hidden_clean"] == 0
    o = hostlib.parse_options(["slaMEM", "ref.fa", "-evs", "1024", "-mdep", "3", "reads.fa", "-CONS", "-b"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"] and o["both_strands"] == 1
    for other in ("-mam", "-mum", "-smem", "-chain", "-ext", "-aln", "-paf", "-pile", "-sites", "-vcf"):
        assert hostlib.parse_options(["slaMEM", "ref.fa", other, "reads.fa", "-cons"])["match_type"] == -1
    # -c alone is still the clean tool, and the other modes are what they were
    assert hostlib.parse_options(["slaMEM", "-c", "x.fa"])["hidden_clean"] == 1
    assert hostlib.parse_options(["slaMEM", "-vcf", "ref.fa", "reads.fa"])["match_type"] == 8
    assert hostlib.parse_options(["slaMEM", "-chain", "ref.fa", "reads.fa"])["match_type"] == 4


def run_exe(args, tmp_path):
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"r", b"ACGT" * 30)])
    write_fasta(q_fa, [(b"q", b"ACGT" * 10)])
    return subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))  # (no device: it never asks for one)


def test_usage_lists_the_option():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    for opt in (b"\t-cons\t", b"\t-vcf\t", b"\t-evs\t", b"\t-sites\t"):
        assert opt in r.stdout


CONS_EXCLUDES = b"Option -cons excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites and -vcf"
VCF_EXCLUDES = b"Option -vcf excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile and -sites"
REFUSALS = [
    (["-cons", "-vcf"], CONS_EXCLUDES),
    (["-vcf", "-cons"], CONS_EXCLUDES),
    (["-sites", "-cons"], CONS_EXCLUDES),
    (["-cons", "-pile"], CONS_EXCLUDES),
    (["-paf", "-cons"], CONS_EXCLUDES),
    (["-aln", "-cons"], CONS_EXCLUDES),
    (["-cons", "-ext"], CONS_EXCLUDES),
    (["-chain", "-cons"], CONS_EXCLUDES),
    (["-cons", "-smem"], CONS_EXCLUDES),
    (["-mum", "-cons"], CONS_EXCLUDES),
    (["-cons", "-mam"], CONS_EXCLUDES),
    (["-cons", "-mpct", "20"], b"Option -mpct has no meaning with -cons"),
    (["-mdep", "3", "-mpct", "0", "-cons"], b"Option -mpct has no meaning with -cons"),
    (["-cons", "-mdep", "0"], b"Option -mdep needs a whole number of at least 1"),
    (["-cons", "-mpct", "101"], b"Option -mpct needs a whole number from 0 to 100"),
    (["-cons", "-evs", "100"], b"Option -evs needs a power of two of at least 64"),
    (["-cons", "-minq", "61"], b"Option -minq needs a whole number from 0 to 60"),
    (["-cons", "-occ", "3"], b"Option -occ needs -smem"),
    # the wording of the earlier refusals stands, for every combination that printed it
    (["-vcf", "-sites"], VCF_EXCLUDES),
    (["-pile", "-vcf"], VCF_EXCLUDES),
    (["-pile", "-sites"], b"Option -sites excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf and -pile"),
    (["-paf", "-mdep", "3"], b"Options -mdep and -mpct need -sites"),
    (["-pile", "-mpct", "3"], b"Options -mdep and -mpct need -sites"),
    (["-sites", "-evs", "1024"], b"Option -evs needs -vcf"),
    (["-pile", "-evs", "64"], b"Option -evs needs -vcf"),
    (["-evs", "1024"], b"Option -evs needs -vcf"),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_cli_refusals_exit_before_any_gpu_work(args, message, tmp_path):
    r = run_exe(args, tmp_path)
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout
    assert not os.path.exists(str(tmp_path / "ref-mems.txt"))
