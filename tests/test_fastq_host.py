"""FASTQ queries and -bq on the host, no GPU: slh_load_file_q and slh_pieces_next_q against the reader of
tests/lowq_spec.py, their refusals, FASTA as it was, slamem_pack_lowq against the spec's pack, the parsing of -bq beside every
option there was, and a run of the loader and the pack under AddressSanitizer and UBSan as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fastq_host
import hostlib
import lowq_spec
from golden_cases import CASES, case_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(hostlib.HOST_DIR, "slaMEM-hip")
CSRC = os.path.join(ROOT, "slamem_amd", "csrc")
NO_GPU = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")  # (these runs end before they ask for a device)


def rand_record(rng, k, n, alphabet=b"ACGT"):
    letters = bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n))
    quals = bytes(rng.integers(33, 127, size=n, dtype=np.uint8))
    return b"read%d some words" % k, letters, quals


def small_files():
    """name -> (bytes, what the file is about)"""
    rng = np.random.default_rng(5)
    one = [rand_record(rng, 0, 37)]
    many = [rand_record(rng, k, int(rng.integers(1, 300))) for k in range(200)]
    lead = [(b"at", b"ACGTACGT", b"@IIIIII@"), (b"plus", b"ACGTAC", b"+@+@+@"), (b"both @ +", b"TTGA", b"@+@+"), (b"+", b"A", b"@")]
    dropped = [(b"d0", b"AC-GT 12*NnRy.acgt", bytes(range(40, 58))), (b"d1", b"NNNN", b"!!!!"), (b"d2", b"acgtACGT", b"ABCDEFGH"),
               (b"short", b"AC", b"II"), (b"none", b"--**", b"IIII")]
    return {
        "one": lowq_spec.write_fastq(one),
        "many": lowq_spec.write_fastq(many),
        "crlf": lowq_spec.write_fastq(many[:50], eol=b"\r\n"),
        "no_final_newline": lowq_spec.write_fastq(many[:7], final_newline=False),
        "crlf_no_final_newline": lowq_spec.write_fastq(many[:7], eol=b"\r\n", final_newline=False),
        "leading_at_and_plus": lowq_spec.write_fastq(lead),
        "dropped_letters": lowq_spec.write_fastq(dropped),
        "plus_line_repeats_name": b"@r1 x\nACGT\n+r1 x\nIIII\n",
    }


FILES = small_files()


def check_against_spec(path, data, acgt_only, min_len):
    got = fastq_host.LoadedQ(path, 0, acgt_only, min_len)
    names, letters, quals = lowq_spec.read_fastq(data, bool(acgt_only), min_len)
    assert got.n == len(names)
    if not names:
        assert got.quals is None
        return got
    assert got.names == names and got.sizes == [len(l) for l in letters]
    assert got.chars == b"".join(letters) and got.quals == b"".join(quals)  # (parallel: the same offsets cut both)
    assert got.offsets == [0] + list(np.cumsum([len(l) for l in letters]))
    return got


@pytest.mark.parametrize("name", sorted(FILES))
def test_parser_against_the_spec(name, tmp_path):
    path = str(tmp_path / (name + ".fq"))
    open(path, "wb").write(FILES[name])
    for acgt_only, min_len in ((0, 0), (1, 0), (0, 3), (1, 3), (0, 100)):
        check_against_spec(path, FILES[name], acgt_only, min_len)
    # the whole-line path and the byte loop give the same (as for FASTA)
    os.environ["SLAMEM_LOADER_BYTEWISE"] = "1"
    try:
        out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import fastq_host as f; l = f.LoadedQ(%r); "
                              "sys.stdout.buffer.write(l.chars + b'|' + (l.quals or b''))" % (os.path.dirname(__file__), path)],
                             stdout=subprocess.PIPE, check=True).stdout
    finally:
        del os.environ["SLAMEM_LOADER_BYTEWISE"]
    l = fastq_host.LoadedQ(path)
    assert out == l.chars + b"|" + (l.quals or b"")


def test_what_the_small_files_cover(tmp_path):
    """(the files are what they claim to be)"""
    names, letters, quals = lowq_spec.read_fastq(FILES["dropped_letters"])
    assert names == [b"d0", b"d1", b"d2", b"short"] and letters[0] == b"ACGTNNNNACGT"
    assert quals[0] == bytes(40 + i for i, c in enumerate(b"AC-GT 12*NnRy.acgt") if chr(c).isalpha())
    names, letters, quals = lowq_spec.read_fastq(FILES["dropped_letters"], True, 3)
    assert names == [b"d0", b"d2"] and letters[0] == b"ACGTACGT" and quals[0] == bytes([40, 41, 43, 44, 54, 55, 56, 57])
    assert [q[:1] for q in lowq_spec.read_fastq(FILES["leading_at_and_plus"])[2]] == [b"@", b"+", b"@", b"@"]
    path = str(tmp_path / "m.fq")
    open(path, "wb").write(FILES["many"])
    assert 0 < check_against_spec(path, FILES["many"], 0, 100).n < 200  # (-m drops records, the numbering and the offsets follow)
    log = fastq_host.LoadedQ(path, 0, 0, 100).log
    assert b"TOO SHORT" in log and b"# 01 [read" in log and b" bp) OK\n" in log


@pytest.mark.parametrize("name,data", [
    ("unequal_lengths", b"@r\nACGT\n+\nIII\n"),
    ("unequal_lengths_second_record", b"@r\nACGT\n+\nIIII\n@s\nAC\n+\nIIII\n"),
    ("missing_plus", b"@r\nACGT\nIIII\n@s\nAC\n+\nII\n"),
    ("missing_plus_line", b"@r\nACGT\n-\nIIII\n"),
    ("truncated_after_letters", b"@r\nACGT\n+\nIIII\n@s\nACGT\n"),
    ("truncated_after_plus", b"@r\nACGT\n+\nIIII\n@s\nACGT\n+\n"),
    ("truncated_name_only", b"@r\nACGT\n+\nIIII\n@s"),
    ("blank_line_at_the_end", b"@r\nACGT\n+\nIIII\n\n"),
    ("second_record_without_at", b"@r\nACGT\n+\nIIII\nr\nACGT\n+\nIIII\n"),
])
def test_refusals(name, data, tmp_path):
    path = str(tmp_path / (name + ".fq"))
    open(path, "wb").write(data)
    with pytest.raises(lowq_spec.InvalidFastq):
        lowq_spec.read_fastq(data)
    got = fastq_host.LoadedQ(path)
    assert got.n == -1 and got.log.endswith(b"> ERROR: Invalid FASTQ file\n") and got.quals is None
    pieces, last = fastq_host.pieces(path, 1 << 20)
    assert pieces == [] and last == -1
    # the front end: the message, status 255, no output file, no GPU asked for
    ref_fa = case_paths("acgt_l20_fwd")[0]
    for env in ({}, {"SLAMEM_OVERLAP_MB": "0", "SLAMEM_FOREGROUND": "1"}):
        out = str(tmp_path / "o.txt")
        r = subprocess.run([EXE, "-o", out, ref_fa, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                           env=dict(os.environ, **NO_GPU, **env))
        assert r.returncode == 255 and b"> ERROR: Invalid FASTQ file\n" in r.stdout, r.stdout[-2000:]
        if not env:  # (read in front of the search: nothing was opened.  The loader thread beside the search says so when it gets there)
            assert not os.path.exists(out) and b"Building index" not in r.stdout


def test_fastq_as_reference_is_refused(tmp_path):
    path = str(tmp_path / "ref.fq")
    open(path, "wb").write(FILES["many"])
    got = fastq_host.LoadedQ(path, merge=1)
    assert got.n == -1 and b"> ERROR: The reference file is FASTQ: the reference must be FASTA\n" in got.log
    q_fa = case_paths("acgt_l20_fwd")[1]
    r = subprocess.run([EXE, "-o", str(tmp_path / "o.txt"), path, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       env=dict(os.environ, **NO_GPU))
    assert r.returncode == 255 and b"> ERROR: The reference file is FASTQ: the reference must be FASTA\n" in r.stdout
    assert b"Building index" not in r.stdout and not os.path.exists(str(tmp_path / "o.txt"))
    # the loader without FASTQ (slh_load_file) sees what it saw before: a file that is not FASTA
    old = hostlib.Loaded(path, 0)
    assert old.n == 0


@pytest.mark.parametrize("case", CASES)
def test_fasta_stays_as_it_was(case):
    ref_fa, q_fa, _, _ = case_paths(case)
    for path, merge in ((ref_fa, 1), (q_fa, 0)):
        old = hostlib.Loaded(path, merge)
        new = fastq_host.LoadedQ(path, merge)
        assert new.n == old.n and new.quals is None
        if merge:
            assert new.merged_chars == (old.chars if old.n else None)
        else:
            assert (new.names, new.sizes, new.chars, new.offsets) == (old.names, old.sizes, old.chars, old.offsets)
            pieces, last = fastq_host.pieces(path, 1 << 20)
            assert last == 0 and all(p[4] is None for p in pieces) and b"".join(p[2] for p in pieces) == old.chars


def test_pieces_equal_the_whole_file(tmp_path):
    """slh_pieces_next_q in pieces of 1 MB: the records, letters and qualities of slh_load_file_q, in order; every quality line
    starts with '@' or '+', so a cut at "newline + '@'" would go wrong."""
    rng = np.random.default_rng(9)
    recs = []
    for k in range(12000):
        n = int(rng.integers(1, 400))
        name, letters, quals = rand_record(rng, k, n, b"ACGTacgtNRYn-")
        recs.append((name, letters, (b"@" if k % 2 else b"+") + quals[1:]))
    data = lowq_spec.write_fastq(recs, final_newline=False)
    path = str(tmp_path / "q.fq")
    open(path, "wb").write(data)
    for acgt_only, min_len in ((0, 0), (1, 50)):
        whole = fastq_host.LoadedQ(path, 0, acgt_only, min_len)
        names, letters, quals = lowq_spec.read_fastq(data, bool(acgt_only), min_len)
        assert whole.names == names and whole.chars == b"".join(letters) and whole.quals == b"".join(quals)
        pieces, last = fastq_host.pieces(path, 1 << 20, acgt_only, min_len)
        assert last == 0 and len(pieces) >= 4
        assert sum((p[0] for p in pieces), []) == whole.names and sum((p[1] for p in pieces), []) == whole.sizes
        assert b"".join(p[2] for p in pieces) == whole.chars and b"".join(p[4] for p in pieces) == whole.quals
        for p in pieces:
            assert p[3][0] == 0 and list(np.diff(p[3])) == p[1]


def test_parser_threads_equal_one_thread(tmp_path):
    """A file above the multi-thread threshold (64 MB; 16 MB for a piece): records of one size whose quality lines all start with
    '@', so that wherever the threads' cuts fall a '@' stands behind a newline in front of them and behind them -- compared with
    the one-thread parse; and the pieces of 20 MB, parsed by four threads each, with the same."""
    rng = np.random.default_rng(11)
    nrec, L = 340000, 100
    head = np.frombuffer(b"".join(b"@r%07d\n" % k for k in range(nrec)), dtype=np.uint8).reshape(nrec, 10)
    letters = rng.choice(np.frombuffer(b"ACGTacgtN-", dtype=np.uint8), size=(nrec, L), p=[.22, .22, .22, .22, .02, .02, .02, .02, .02, .02])
    quals = rng.integers(33, 127, size=(nrec, L), dtype=np.uint8)
    quals[:, 0] = ord("@")
    nl = np.full((nrec, 1), 10, dtype=np.uint8)
    plus = np.tile(np.frombuffer(b"+\n", dtype=np.uint8), (nrec, 1))
    rows = np.concatenate([head, letters, nl, plus, quals, nl], axis=1)
    assert rows.nbytes > (64 << 20)
    path = str(tmp_path / "big.fq")
    rows.tofile(path)
    old = os.environ.get("SLAMEM_THREADS")
    try:
        os.environ["SLAMEM_THREADS"] = "1"
        a = fastq_host.LoadedQ(path, 0, 0, 95)
        os.environ["SLAMEM_THREADS"] = "7"
        b = fastq_host.LoadedQ(path, 0, 0, 95)
        os.environ["SLAMEM_THREADS"] = "4"
        pieces, last = fastq_host.pieces(path, 20 << 20, 0, 95)
    finally:
        if old is None:
            del os.environ["SLAMEM_THREADS"]
        else:
            os.environ["SLAMEM_THREADS"] = old
    assert nrec > a.n == b.n > 100000 and a.names == b.names and a.sizes == b.sizes and a.offsets == b.offsets
    assert a.chars == b.chars and a.quals == b.quals and len(a.quals) == len(a.chars)
    assert last == 0 and len(pieces) >= 3
    assert sum((p[0] for p in pieces), []) == a.names and b"".join(p[2] for p in pieces) == a.chars
    assert b"".join(p[4] for p in pieces) == a.quals
    # a sample of the records against the definition: the dropped letters took their quality bytes with them
    off = a.offsets
    for k in (0, 1, a.n // 2, a.n - 1):
        r = int(a.names[k][1:])
        l, v = lowq_spec._normalise(bytes(letters[r]), bytes(quals[r]), False)
        assert a.chars[off[k]:off[k + 1]] == l and a.quals[off[k]:off[k + 1]] == v


# ---- slamem_pack_lowq ----------------------------------------------------------------------------------------------------------

def c_pack(quals: bytes, min_bq, phred=33, threads=3, guard=2):
    from slamem_amd import capi
    L = capi.lib()
    words = (len(quals) + 63) // 64
    out = np.full(words + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    buf = np.frombuffer(quals, dtype=np.uint8).copy()
    rc = L.slamem_pack_lowq(buf.ctypes.data if len(buf) else None, len(buf), min_bq, phred, out.ctypes.data, threads)
    assert bool((out[words:] == 0xA5A5A5A5A5A5A5A5).all())  # (nothing behind the mask's last word is written)
    return rc, out[:words]


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 4097])
def test_pack_lowq_against_the_spec(total):
    from slamem_amd import capi
    rng = np.random.default_rng(total)
    quals = bytes(rng.integers(0, 256, size=total, dtype=np.uint8))  # (bytes below the offset among them)
    for min_bq in (0, 1, 20, 93):
        for phred in (33, 64, 0, 126):
            rc, got = c_pack(quals, min_bq, phred)
            assert rc == capi.SLAMEM_OK and np.array_equal(got, lowq_spec.pack(quals, min_bq, phred)), (min_bq, phred)
    assert not c_pack(quals, 0)[1].any()
    below = bytes([32, 0, 33, 34]) * (total // 4)  # a byte below phred_offset counts as quality 0: low for every min_bq >= 1
    rc, got = c_pack(below, 1)
    assert np.array_equal(got, lowq_spec.pack(below, 1)) and [lowq_spec.bit(got, j) for j in range(min(4, len(below)))] == [1, 1, 1, 0][:min(4, len(below))]
    if total % 64:
        assert int(c_pack(b"!" * total, 93)[1][-1]) == (1 << (total % 64)) - 1  # (all low: the tail's unused bits stay 0)


def test_pack_lowq_threads_and_argument_errors():
    from slamem_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(1)
    quals = bytes(rng.integers(33, 80, size=(1 << 22) + 77, dtype=np.uint8))  # (above the size at which the threads share the words)
    want = c_pack(quals, 20, threads=1)[1]
    assert np.array_equal(c_pack(quals, 20, threads=7)[1], want) and np.array_equal(c_pack(quals, 20, threads=99)[1], want)
    q = np.frombuffer(quals[:4096], dtype=np.uint8)
    assert np.array_equal(want[:64], np.packbits((q.astype(np.int64) - 33 < 20), bitorder="little").view(np.uint64))
    for min_bq, phred, word in ((94, 33, b"minimum base quality"), (20, 127, b"quality offset"), (1 << 31, 33, b"minimum base quality")):
        rc, _ = c_pack(quals[:10], min_bq, phred)
        assert rc == capi.SLAMEM_ERR_ARG and word in L.slamem_last_error_message()
    assert L.slamem_pack_lowq(None, 5, 20, 33, None, 1) == capi.SLAMEM_ERR_ARG


# ---- -bq on the command line ---------------------------------------------------------------------------------------------------

def test_bq_value_parsing():
    p = fastq_host.parse_min_bq
    assert p(["slaMEM", "-pile", "r.fa", "q.fq"]) == (0, 0)
    for v in (0, 1, 20, 93):
        assert p(["slaMEM", "-pile", "-bq", str(v), "r.fa", "q.fq"]) == (1, v)
        assert p(["slaMEM", "-BQ", str(v), "-pile", "r.fa", "q.fq"]) == (1, v)
    for bad in ("94", "-1", "x", "2x", "", "1.5", "99999999999999999999"):
        assert p(["slaMEM", "-pile", "-bq", bad, "r.fa", "q.fq"])[0] == -1, bad
    assert p(["slaMEM", "-pile", "r.fa", "q.fq", "-bq"])[0] == -1
    assert p(["slaMEM", "-b", "-pile", "r.fa", "q.fq"]) == (0, 0)  # -b is not -bq


OLD_LINES = [  # (arguments, files, match type, both strands): every option there was, as it parsed before -bq
    (["-b", "-l", "10", "r.fa", "q.fa"], ["r.fa", "q.fa"], 0, 1),
    (["-B", "-N", "-L", "7", "-O", "x.txt", "-M", "50", "r.fa", "q.fa"], ["r.fa", "q.fa"], 0, 1),
    (["-mam", "r.fa", "q.fa"], ["q.fa"], 1, 0),  # (an 'm' option eats the next argument: the quirk stays)
    (["-mum", "x", "r.fa", "q.fa"], ["r.fa", "q.fa"], 2, 0),
    (["-smem", "-occ", "5", "r.fa", "q.fa"], ["r.fa", "q.fa"], 3, 0),
    (["-chain", "-mgap", "100", "r.fa", "q.fa"], ["r.fa", "q.fa"], 4, 0),
    (["-ext", "-pen", "3", "-xdrop", "9", "r.fa", "q.fa"], ["r.fa", "q.fa"], 5, 0),
    (["-aln", "-maxed", "5", "r.fa", "q.fa"], ["r.fa", "q.fa"], 6, 0),
    (["-paf", "-b", "r.fa", "q.fa"], ["r.fa", "q.fa"], 7, 1),
    (["-pile", "-minq", "3", "r.fa", "q.fa"], ["r.fa", "q.fa"], 8, 0),
    (["-sites", "-mdep", "2", "-mpct", "10", "r.fa", "q.fa"], ["r.fa", "q.fa"], 8, 0),
    (["-vcf", "-evs", "64", "r.fa", "q.fa"], ["r.fa", "q.fa"], 8, 0),
    (["-cons", "r.fa", "q.fa"], ["r.fa", "q.fa"], 8, 0),
    (["-depth", "-lev", "1,5", "r.fa", "q.fa"], ["r.fa", "q.fa"], 8, 0),
    (["-depth", "-win", "100", "-b", "r.fa", "q.fa"], ["r.fa", "q.fa"], 8, 1),
    (["-bx", "r.fa", "q.fa"], ["r.fa", "q.fa"], 0, 0),
    (["-r", "chrB", "r.fa", "q.fa"], ["r.fa", "q.fa"], 0, 0),
]


@pytest.mark.parametrize("args,files,match_type,both", OLD_LINES)
def test_every_existing_option_parses_as_before(args, files, match_type, both):
    o = hostlib.parse_options(["slaMEM"] + args)
    assert (o["files"], o["match_type"], o["both_strands"]) == (files, match_type, both)
    assert fastq_host.parse_min_bq(["slaMEM"] + args) == (0, 0)
    # with -bq N in front, behind and in the middle: the same, and N is no file name
    for at in (0, len(args) - 2, len(args)):
        if at > 0 and args[at - 1].startswith("-") and args[at - 1].lower()[1:2] in "lomvrepxw":
            continue  # (not between an option and its value)
        more = args[:at] + ["-bq", "20"] + args[at:]
        o2 = hostlib.parse_options(["slaMEM"] + more)
        assert (o2["files"], o2["match_type"], o2["both_strands"]) == (files, match_type, both), more
        assert {k: v for k, v in o2.items() if k != "out_arg"} == {k: v for k, v in o.items() if k != "out_arg"}, more
        assert fastq_host.parse_min_bq(["slaMEM"] + more) == (1, 20)


@pytest.mark.parametrize("mode", ["-pile", "-sites", "-vcf", "-cons", "-depth"])
def test_bq_is_accepted_with_the_pileup_modes(mode, tmp_path):
    """(no device: the run gets as far as the GPU and stops there -- the option was not what stopped it)"""
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    r = subprocess.run([EXE, mode, "-bq", "20", "-o", str(tmp_path / "o.txt"), ref_fa, q_fa], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120, env=dict(os.environ, **NO_GPU))
    assert r.returncode == 255 and b"Option -bq" not in r.stdout and b"Loading sequences" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("args,message", [
    (["-bq", "20"], b"Option -bq needs -pile"),
    (["-paf", "-bq", "20"], b"Option -bq needs -pile"),
    (["-mam", "-bq", "20"], b"Option -bq needs -pile"),
    (["-aln", "-bq", "0"], b"Option -bq needs -pile"),
    (["-pile", "-bq", "94"], b"Option -bq needs a whole number from 0 to 93"),
    (["-vcf", "-bq", "x"], b"Option -bq needs a whole number from 0 to 93"),
    (["-depth", "-bq", "-1"], b"Option -bq needs a whole number from 0 to 93"),
])
def test_bq_refusals_exit_before_any_gpu_work(args, message, tmp_path):
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    shutil.copy(ref_fa, tmp_path / "ref.fa")
    r = subprocess.run([EXE] + args + [str(tmp_path / "ref.fa"), q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, **NO_GPU))
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout and b"Loading sequences" not in r.stdout
    assert not os.path.exists(str(tmp_path / "ref-mems.txt"))


def test_usage_names_bq():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, timeout=60)
    assert b"\t-bq\t" in r.stdout and b"\t-minq\t" in r.stdout


# ---- the sanitizer run ---------------------------------------------------------------------------------------------------------

def test_loader_and_pack_under_asan_and_ubsan(tmp_path):
    """slamem_host.c and tests/fastq_asan_driver.c (a program of its own) built with -fsanitize=address,undefined and run on the
    files above, on invalid ones, on FASTA and on a file of several pieces: no report, and the numbers the spec gives."""
    cc = shutil.which("cc") or shutil.which("gcc")
    exe = str(tmp_path / "fastq_asan_driver")
    subprocess.check_call([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu99",
                           "-I", os.path.join(ROOT, "include"), "-I", hostlib.HOST_DIR, "-o", exe,
                           os.path.join(ROOT, "tests", "fastq_asan_driver.c"), os.path.join(hostlib.HOST_DIR, "slamem_host.c"),
                           os.path.join(hostlib.HOST_DIR, "mem_image.c"), "-L", CSRC, "-lslamem_hip", "-Wl,-rpath," + CSRC,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-lpthread", "-lm"])
    paths = []
    for name, data in FILES.items():
        paths.append(str(tmp_path / (name + ".fq")))
        open(paths[-1], "wb").write(data)
    rng = np.random.default_rng(2)
    big = [rand_record(rng, k, int(rng.integers(1, 400)), b"ACGTacgtNRYn-") for k in range(9000)]
    big = [(n, l, b"@" + v[1:]) for n, l, v in big]
    paths.append(str(tmp_path / "pieces.fq"))
    open(paths[-1], "wb").write(lowq_spec.write_fastq(big))
    for k, data in enumerate((b"@r\nACGT\n+\nIII\n", b"@r\nACGT\nIIII\n", b"@r\nACGT\n+\nIIII\n@s\nACGT\n", b"@", b"@r\n\n+\n\n")):
        paths.append(str(tmp_path / ("odd%d.fq" % k)))
        open(paths[-1], "wb").write(data)
    paths += list(case_paths("normalise_default")[:2])
    r = subprocess.run([exe] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, SLAMEM_THREADS="3", **NO_GPU))
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    out = r.stdout.decode()
    names, letters, quals = lowq_spec.read_fastq(FILES["many"])
    low = int(sum(bin(int(w)).count("1") for w in lowq_spec.pack(b"".join(quals), 20)))
    assert "many.fq query n=%d acgt_only=0 letters=%d quals=1 low=%d\n" % (len(names), sum(map(len, letters)), low) in out
    assert "many.fq reference n=-1\n" in out and "odd0.fq query n=-1 acgt_only=0\n" in out and "odd2.fq pieces=0 last=-1 low=0\n" in out
    names, letters, quals = lowq_spec.read_fastq(lowq_spec.write_fastq(big))
    low = int(sum(bin(int(w)).count("1") for w in lowq_spec.pack(b"".join(quals), 20)))
    assert "pieces.fq query n=%d acgt_only=0 letters=%d quals=1 low=%d\n" % (len(names), sum(map(len, letters)), low) in out
    assert "ref.fa query n=" in out and "quals=0" in out
