"""-sites on the CPU: the definition (tests/sites_spec.py) itself, without the engine -- hand-written tables over
a short text whose rows and masks are written out by hand, the thresholds at equality, products beyond 2^32, the -sites file of
a reference of two records, the host library's formatter against the spec, the usage text and the refusals of the command
line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ext_spec
import hostlib
import map_spec
import pile_spec
import sites_spec
from sites_spec import NONZERO, VARIANT
from test_map_host import FakeRef

#        0123456789012345678901
TEXT = b"ACGTTGCAAGCTNACGgATCCA"  # an N at 12, a lower-case g at 16
N = len(TEXT)
A, Cc, G, T, D, I = range(6)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
PLANTED_SEED = 20261  # (fixed: test_planted_sample_answer_holds_on_the_definition confirms the known answer on the definition alone)


def table(rows):
    """{position: (A, C, G, T, D, I)} -> the table"""
    t = pile_spec.empty(N)
    for p, row in rows.items():
        t[p] = row
    return t


def got(t, *a, **kw):
    pos, counts, alleles = sites_spec.sites(t, TEXT, *a, **kw)
    assert pos.dtype == np.uint64 and counts.dtype == np.uint32 and alleles.dtype == np.uint8 and counts.shape == (len(pos), 6)
    assert np.array_equal(counts.astype(np.int64), t[pos.astype(np.int64)])
    return {int(p): int(m) for p, m in zip(pos, alleles)}


def test_each_bit_on_its_own_and_the_own_column_never():
    # position: letter -- 0: A, 1: C, 2: G, 3: T
    for p, own in ((0, A), (1, Cc), (2, G), (3, T)):
        for k in range(6):
            row = [0] * 6
            row[own] += 10
            row[k] += 10
            sel = got(table({p: row}), VARIANT, 1, 0)
            assert sel == ({} if k == own else {p: 1 << k}), (p, k)
    # a row that only restates the text is not a site, whatever its depth
    assert got(table({5: (0, 0, 1000, 0, 0, 0)}), VARIANT, 1, 0) == {}
    # several bits at once, in ascending position
    t = table({9: (3, 0, 4, 3, 2, 1), 4: (0, 5, 0, 5, 0, 0)})
    assert got(t, VARIANT, 1, 0) == {4: 1 << Cc, 9: (1 << A) | (1 << T) | (1 << D) | (1 << I)}
    assert list(sites_spec.sites(t, TEXT, VARIANT, 1, 0)[0]) == [4, 9]


def test_lower_case_letter_is_its_upper_case():
    # TEXT[16] = g: the G column is its own
    assert got(table({16: (0, 0, 7, 0, 0, 0)}), VARIANT, 1, 0) == {}
    assert got(table({16: (7, 0, 7, 0, 0, 0)}), VARIANT, 1, 0) == {16: 1 << A}


def test_row_on_n_is_mode_0_only():
    t = table({12: (3, 0, 0, 2, 1, 1)})
    assert got(t, VARIANT, 1, 0) == {}
    assert got(t, NONZERO) == {12: 0b111001}
    # mode 0 takes no notice of the thresholds or of the letter's own column
    t = table({12: (3, 0, 0, 2, 1, 1), 0: (1, 0, 0, 0, 0, 0), 21: (0, 0, 0, 0, 0, 9)})
    assert got(t, NONZERO, 10 ** 9, 100) == {0: 1, 12: 0b111001, 21: 1 << I}
    assert got(pile_spec.empty(N), NONZERO) == {} and got(pile_spec.empty(N), VARIANT, 1, 0) == {}


def test_thresholds_at_equality():
    # d = 20, C = 4: 100 * 4 == 20 * 20
    assert got(table({0: (16, 4, 0, 0, 0, 0)}), VARIANT, 4, 20) == {0: 1 << Cc}
    assert got(table({0: (17, 4, 0, 0, 0, 0)}), VARIANT, 4, 20) == {}          # d = 21: 400 < 420
    assert got(table({0: (16, 3, 0, 0, 1, 0)}), VARIANT, 4, 20) == {}          # one less of C, the same d
    assert got(table({0: (16, 4, 0, 0, 0, 0)}), VARIANT, 4, 21) == {}
    # the insertions are measured against the depth they are not part of
    assert got(table({0: (20, 0, 0, 0, 0, 4)}), VARIANT, 4, 20) == {0: 1 << I}
    assert got(table({0: (20, 0, 0, 0, 0, 3)}), VARIANT, 4, 20) == {}
    # d == min_depth selects, one below does not
    assert got(table({0: (2, 2, 0, 0, 0, 0)}), VARIANT, 4, 20) == {0: 1 << Cc}
    assert got(table({0: (1, 2, 0, 0, 0, 0)}), VARIANT, 4, 20) == {}
    assert got(table({0: (1, 2, 0, 0, 0, 0)}), VARIANT, 3, 20) == {0: 1 << Cc}
    # D counts towards the depth, I does not
    assert got(table({0: (1, 2, 0, 0, 1, 0)}), VARIANT, 4, 20) == {0: (1 << Cc) | (1 << D)}
    assert got(table({0: (1, 2, 0, 0, 0, 1)}), VARIANT, 4, 20) == {}
    # min_pct 100: only a row where everything is one other letter
    assert got(table({0: (0, 5, 0, 0, 0, 0), 2: (1, 5, 0, 0, 0, 0)}), VARIANT, 2, 100) == {0: 1 << Cc}


def test_min_pct_0_with_a_zero_counter_sets_no_bit():
    assert got(table({0: (9, 0, 0, 0, 0, 0)}), VARIANT, 1, 0) == {}
    assert got(table({0: (9, 0, 1, 0, 0, 0)}), VARIANT, 1, 0) == {0: 1 << G}


def test_products_beyond_32_bits():
    # 100 * 50,000,000 = 5e9 and 3 * 2,050,000,000 = 6.15e9 both pass 2^32
    row = (2_000_000_000, 0, 50_000_000, 0, 0, 0)
    assert got(table({0: row}), VARIANT, 1, 3) == {}
    # at 2 percent the row is selected, and products taken modulo 2^32 would say otherwise
    assert (100 * row[G]) % 2 ** 32 < 2 * sum(row) <= 100 * row[G]
    assert got(table({0: row}), VARIANT, 1, 2) == {0: 1 << G}
    assert got(table({0: row}), VARIANT, 2_050_000_000, 2) == {0: 1 << G} and got(table({0: row}), VARIANT, 2_050_000_001, 2) == {}
    # counters just below 2^31 in every column: the depth is a 64-bit sum
    assert sites_spec.row_mask((2 ** 31 - 1,) * 6, ord("A"), VARIANT, 2 ** 31 - 1, 20) == 0b111110
    assert sites_spec.row_mask((2 ** 31 - 1,) * 6, ord("A"), VARIANT, 2 ** 31 - 1, 21) == 0


def test_ranges_and_refused_rules():
    t = table({0: (1, 1, 0, 0, 0, 0), 5: (1, 0, 1, 0, 0, 0), N - 1: (1, 1, 0, 0, 0, 0)})
    assert got(t, VARIANT, 1, 0) == {0: 2, 5: 1, N - 1: 2}
    assert got(t, VARIANT, 1, 0, first=1, count=N - 2) == {5: 1}
    assert got(t, VARIANT, 1, 0, first=5, count=1) == {5: 1}
    assert got(t, VARIANT, 1, 0, first=N, count=0) == {} and got(t, VARIANT, 1, 0, first=0, count=0) == {}
    for bad in ((2, 4, 20), (VARIANT, 0, 20), (VARIANT, 2 ** 31, 20), (VARIANT, 4, 101), (NONZERO, 4, 101)):
        with pytest.raises(ValueError):
            sites_spec.sites(t, TEXT, *bad)


def test_calls_column():
    assert sites_spec.calls(1 << G) == b"G" and sites_spec.calls((1 << T) | (1 << D)) == b"T,D"
    assert sites_spec.calls(0b111111) == b"A,C,G,T,D,I" and sites_spec.calls(1 << I) == b"I"


def two_record_case():
    recs = [b"ACGTTGCA", b"GGaTCCAT"]
    ref = FakeRef(recs, [b"first one", b"second\tx"])
    n = len(ref.chars)  # 8 + 1 + 8: the separator sits at 8
    t = pile_spec.empty(n)
    t[0] = (2, 0, 0, 0, 0, 0)      # restates the text
    t[3] = (0, 0, 1, 3, 2, 0)      # T with a G and two deletions
    t[7] = (4, 0, 0, 0, 0, 1)      # A with an insertion in front
    t[8] = (0, 0, 0, 0, 5, 0)      # the separator: belongs to no record
    t[9] = (0, 0, 3, 1, 0, 0)      # G with a T
    t[11] = (2, 2, 0, 0, 0, 0)     # a (lower case) with a C
    t[16] = (0, 0, 0, 1, 4, 0)     # T, mostly deleted
    want = (b"first\t4\tT\t0\t0\t1\t3\t2\t0\tG,D\n" b"first\t8\tA\t4\t0\t0\t0\t0\t1\tI\n"
            b"second\t1\tG\t0\t0\t3\t1\t0\t0\tT\n" b"second\t3\tA\t2\t2\t0\t0\t0\t0\tC\n" b"second\t8\tT\t0\t0\t0\t1\t4\t0\tD\n")
    return ref, t, want


def test_sites_file_of_a_two_record_reference():
    ref, t, want = two_record_case()
    assert sites_spec.sites_file(t, ref, 1, 0) == want and b">" not in want
    # at the defaults the rows of depth 4 and more remain, and of those the calls of at least a fifth
    assert sites_spec.sites_file(t, ref) == (b"first\t4\tT\t0\t0\t1\t3\t2\t0\tD\n" b"first\t8\tA\t4\t0\t0\t0\t0\t1\tI\n"
                                             b"second\t1\tG\t0\t0\t3\t1\t0\t0\tT\n" b"second\t3\tA\t2\t2\t0\t0\t0\t0\tC\n"
                                             b"second\t8\tT\t0\t0\t0\t1\t4\t0\tD\n")
    assert sites_spec.sites_file(pile_spec.empty(len(ref.chars)), ref) == b""


def planted_sample(seed: int, n: int = 12000, subs: int = 20, read_len: int = 150, step: int = 5):
    """A random reference over A,C,G,T and a sample genome that equals it but for `subs` substitutions, at least 300 letters
    apart and at least 300 from the ends; error-free reads of read_len letters that start every `step` letters of the sample,
    alternating strands.  Returns (reference, sample, the substituted positions ascending, reads, offsets)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=n)
    slack = n - 600 - 300 * (subs - 1)  # what the spacing of 300 leaves free, shared out among the gaps
    at = 300 + 300 * np.arange(subs) + np.sort(rng.integers(0, slack, size=subs))
    sample = ref.copy()
    for x in at:
        sample[x] = rng.choice(acgt[acgt != ref[x]])
    reads = []
    for k, a in enumerate(range(0, n - read_len + 1, step)):
        r = sample[a:a + read_len]
        reads.append(ext_spec.revcomp(r) if k % 2 else r.copy())
    off = np.arange(len(reads) + 1, dtype=np.uint64) * np.uint64(read_len)
    return ref, sample, at, np.concatenate(reads), off


def planted_answer_holds(ref, sample, at, pos, counts, alleles) -> bool:
    """Exactly the planted positions, each with the one bit of the sample's letter, a depth of at least 4 and nothing in the
    reference letter's column."""
    col = {ord(c): k for k, c in enumerate("ACGT")}
    return (list(pos) == list(at) and len(at) == 20 and
            all(int(alleles[i]) == 1 << col[int(sample[x])] for i, x in enumerate(at)) and
            all(int(counts[i, :5].sum()) >= 4 and int(counts[i, col[int(ref[x])]]) == 0 for i, x in enumerate(at)))


def test_planted_sample_answer_holds_on_the_definition():
    """The known answer of test_gpu_sites.py, on the CPU: map_spec.filter_reads over the oracle's MEM list, piled by pile_spec,
    read out by sites_spec at (4, 20)."""
    from oracle import pyoracle as po
    ref, sample, at, q, off = planted_sample(PLANTED_SEED)
    mem, counts = po.OracleIndex(bytes(ref)).match_batch(q, off, 20, True)
    boff = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    res = map_spec.filter_reads(mem, boff, ref, q, off, True)
    assert all(r[0] == 1 + k % 2 for k, r in enumerate(res))
    table = pile_spec.pile(res, q, off, len(ref))
    assert planted_answer_holds(ref, sample, at, *sites_spec.sites(table, ref, VARIANT, 4, 20))


def format_site_rows(name: bytes, start: int, text: bytes, pos, counts, alleles) -> bytes:
    L = hostlib.lib()
    L.slh_format_site_rows.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint64]
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    alleles = np.ascontiguousarray(alleles, dtype=np.uint8)
    b = hostlib.Buffer()
    assert L.slh_format_site_rows(C.byref(b), name, start, text, pos.ctypes.data, counts.ctypes.data, alleles.ctypes.data, len(pos)) == 0
    out = C.string_at(b.data, b.len) if b.len else b""
    L.slh_buffer_free(C.byref(b))
    return out


def test_host_formatter_against_the_spec():
    ref, t, want = two_record_case()
    pos, counts, alleles = sites_spec.sites(t, ref.chars, VARIANT, 1, 0)
    out = b""
    for r, name in enumerate(ref.names):
        a = int(ref.merged_start[r])
        mine = (pos >= a) & (pos < a + ref.sizes[r])
        out += format_site_rows(name, a, ref.chars, pos[mine], counts[mine], alleles[mine])
    assert out == want
    # every mask, large counters, a position far into a record
    text = b"C" * 70000
    pos = np.arange(64, dtype=np.uint64) + 69000
    counts = np.tile(np.array([[4294967295, 0, 1, 22, 333, 2147483647]], dtype=np.uint32), (64, 1))
    alleles = np.arange(64, dtype=np.uint8)
    out = format_site_rows(b"chr 1", 1000, text, pos, counts, alleles)
    want = b"".join(b"chr\t%d\tC\t4294967295\t0\t1\t22\t333\t2147483647\t%s\n" % (69000 - 1000 + 1 + k, sites_spec.calls(k)) for k in range(64))
    assert out == want
    assert format_site_rows(b"r", 0, text, pos[:0], counts[:0], alleles[:0]) == b""


def test_options_of_the_parser():
    o = hostlib.parse_options(["slaMEM", "-sites", "-mdep", "3", "-mpct", "7", "ref.fa", "-minq", "5", "reads.fa"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"] and not o["hidden_sort"] and o["min_seq_len"] == 0
    assert hostlib.parse_options(["slaMEM", "-pile", "ref.fa", "reads.fa"])["match_type"] == 8
    for other in ("-mam", "-mum", "-smem", "-chain", "-ext", "-aln", "-paf", "-pile"):
        assert hostlib.parse_options(["slaMEM", "ref.fa", other, "reads.fa", "-sites"])["match_type"] == -1
    L = hostlib.lib()
    L.slh_parse_sites_params.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def params(args):
        argv = (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)
        d, p = C.c_int(), C.c_int()
        return L.slh_parse_sites_params(len(args), argv, C.byref(d), C.byref(p)), d.value, p.value
    assert params(["x", "-sites", "a", "b"]) == (0, 4, 20)
    assert params(["x", "-mdep", "2147483647", "-sites", "-mpct", "0"]) == (1, 2147483647, 0)
    assert params(["x", "-MPCT", "100"]) == (1, 4, 100)
    # the other options that begin with -m are none of the two
    assert params(["x", "-mam", "-maxed", "3", "-mgap", "9", "-minq", "1", "-m", "50", "-mum"]) == (0, 4, 20)
    for bad in (["-mdep", "0"], ["-mdep", "2147483648"], ["-mdep", "x"], ["-mdep", "3x"], ["-mdep"]):
        assert params(["x"] + bad)[0] == -1
    for bad in (["-mpct", "-1"], ["-mpct", "101"], ["-mpct", "1.5"], ["-mpct"]):
        assert params(["x"] + bad)[0] == -2


def test_usage_lists_the_options():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    for opt in (b"\t-sites\t", b"\t-mdep\t", b"\t-mpct\t", b"\t-pile\t", b"\t-minq\t"):
        assert opt in r.stdout


def write_fasta(path, records):
    with open(path, "wb") as f:
        for name, letters in records:
            f.write(b">" + name + b"\n" + bytes(letters) + b"\n")


SITES_EXCLUDES = b"Option -sites excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf and -pile"


@pytest.mark.parametrize("args,message", [
    (["-pile", "-sites"], SITES_EXCLUDES),
    (["-sites", "-paf"], SITES_EXCLUDES),
    (["-chain", "-sites"], SITES_EXCLUDES),
    (["-paf", "-mdep", "3"], b"Options -mdep and -mpct need -sites"),
    (["-pile", "-mpct", "3"], b"Options -mdep and -mpct need -sites"),
    (["-mdep", "3"], b"Options -mdep and -mpct need -sites"),
    (["-sites", "-mdep", "0"], b"Option -mdep needs a whole number of at least 1"),
    (["-sites", "-mdep", "x"], b"Option -mdep needs a whole number of at least 1"),
    (["-sites", "-mpct", "101"], b"Option -mpct needs a whole number from 0 to 100"),
    (["-sites", "-mpct", "-1"], b"Option -mpct needs a whole number from 0 to 100"),
    # the wording of -pile's own refusals stands
    (["-pile", "-paf"], b"Option -pile excludes -mam, -mum, -smem, -chain, -ext, -aln and -paf"),
    (["-minq", "5"], b"Option -minq needs -pile"),
])
def test_cli_refusals_exit_before_any_gpu_work(args, message, tmp_path):
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"r", b"ACGT" * 30)])
    write_fasta(q_fa, [(b"q", b"ACGT" * 10)])
    r = subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))  # (no device: it never asks for one)
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout
    assert not os.path.exists(str(tmp_path / "ref-mems.txt"))
