"""-sam without a GPU: the spec's own worked examples, the replay checker on the spec's files, the front end's
writer slh_format_read_sam against sam_spec.sam_lines byte for byte, and the -sam option."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import aln_spec
import hostlib
import map_spec
import sam_spec
from golden_cases import CASES, MANIFEST
from test_map_host import FakeRef

MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
#            0         1         2
#            0123456789012345678901234567
TEXT = b"ACGTTGCAAGGCTTACGATCCGATTAGC"


def seg(p, q, ops):
    rl = aln_spec.runs(ops) if isinstance(ops, str) else ops
    rlen = sum(k for c, k in rl if c in "=XD")
    qlen = sum(k for c, k in rl if c in "=XI")
    return (p, q, rlen, qlen, sum(k for c, k in rl if c != "="), rl)


# ---- the spec's own examples ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ops,md", [
    ([("=", 10)], b"10"),
    ([("=", 5), ("X", 1), ("=", 4)], b"5G4"),
    ([("=", 3), ("X", 2), ("=", 3)], b"3T0T3"),
    ([("=", 4), ("D", 2), ("=", 4)], b"4^TG4"),
    ([("=", 4), ("D", 2), ("X", 1), ("=", 3)], b"4^TG0C3"),
    ([("=", 5), ("I", 2), ("=", 5)], b"10"),
    ([("X", 1), ("=", 3)], b"0A3"),
    ([("=", 3), ("D", 1)], b"3^T0"),
    ([("=", 2), ("D", 1), ("=", 2), ("D", 1), ("=", 1)], b"2^G2^G1"),
])
def test_md_of_hand_written_segments(ops, md):
    """The issue's shapes (10=, 5=1X4=, 3=2X3=, 4=2D4=, 4=2D1X3=, 5=2I5=) on TEXT from position 0: the letters are TEXT's."""
    s = seg(0, 0, ops)
    e = sam_spec.md_entries(s, TEXT)
    assert len(e) == sum(k for c, k in s[5] if c in "XD") + 1 and len(e) <= s[4] + 1
    assert sam_spec.md_text(e) == md and sam_spec.MD_RE.match(md)
    assert sum(x >> 4 for x in e) == sam_spec.seg_eq(s)


def test_entries_are_the_documented_words():
    e = sam_spec.md_entries(seg(2, 0, [("=", 3), ("X", 1), ("I", 2), ("=", 2), ("D", 2), ("=", 1)]), TEXT)
    # p: 2..4 =, 5 X (G), 6..7 =, 8..9 D (A, G), 10 =
    assert e == [3 << 4 | 2, 2 << 4 | 4 | 0, 0 << 4 | 4 | 2, 1 << 4 | 8]
    assert sam_spec.md_text(e) == b"3G2^AG1"


def test_a_letter_that_is_none_of_acgt_under_x_is_an_error():
    with pytest.raises(AssertionError):
        sam_spec.md_entries(seg(0, 0, [("=", 2), ("X", 1)]), b"ACNT")


def test_primary_is_the_largest_eq_first_on_a_tie():
    a, b, c = seg(0, 20, "=====X"), seg(8, 10, "======"), seg(16, 0, "===I===")
    assert sam_spec.primary([a, b, c]) == 1 and sam_spec.primary([b, c]) == 0 and sam_spec.primary([a]) == 0
    assert sam_spec.primary([]) == sam_spec.NO_SEGMENT


REF2 = FakeRef([TEXT, b"GGATCCAATTGGCC"], [b"chrA first", b"chrB\tx"])


def three_segment_read():
    """A read of 30 letters on the forward strand in three segments (4.15's order: query start descending), the middle one with
    a mismatch, the last one in the second record."""
    start_b = REF2.merged_start[1]
    letters = bytearray(b"N" * 30)
    letters[20:28] = TEXT[0:8]
    letters[10:18] = TEXT[10:14] + b"C" + TEXT[15:18]  # (TEXT[14] is A)
    letters[1:9] = REF2.chars[start_b + 2:start_b + 10]
    segl = [seg(0, 20, "========"), seg(10, 10, "====X==="), seg(start_b + 2, 1, "========")]
    return bytes(letters), (1, 37, 16, 6, segl)


def test_lines_flags_clips_and_the_turned_strand():
    letters, res = three_segment_read()
    quals = bytes(range(40, 70))
    lines = sam_spec.sam_lines(b"r1 a read", letters, quals, res, REF2).split(b"\n")[:-1]
    f = [l.split(b"\t") for l in lines]
    assert [x[1] for x in f] == [b"0", b"2048", b"2048"]  # (8, 7 and 8 letters under =: the first on the tie)
    assert [x[5] for x in f] == [b"20S8=2S", b"10S4=1X3=12S", b"1S8=21S"]
    assert [(x[2], x[3]) for x in f] == [(b"chrA", b"1"), (b"chrA", b"11"), (b"chrB", b"3")]
    assert all(x[0] == b"r1" and x[4] == b"37" and x[6:9] == [b"*", b"0", b"0"] and x[9] == letters and x[10] == quals for x in f)
    assert f[1][11:15] == [b"NM:i:1", b"MD:Z:4A3", b"s1:i:16", b"s2:i:6"]
    assert f[0][15] == b"SA:Z:chrA,11,+,10S4=1X3=12S,37,1;chrB,3,+,1S8=21S,37,0;"
    assert sam_spec.replay_check(sam_spec.header(REF2) + b"\n".join(lines) + b"\n", REF2, [b"r1 a read"], [letters], [res], [quals]) == 3
    # the reverse strand: flag 16, SEQ the reverse complement (anything but A,C,G,T: N), QUAL turned, the clips in the scanned strand
    rc = bytes(reversed(TEXT[3:15].translate(bytes.maketrans(b"ACGT", b"TGCA")))) + b"nn"
    res2 = (2, 60, 12, 0, [seg(3, 2, "============")])
    g = sam_spec.sam_lines(b"r2", rc, bytes(range(50, 64)), res2, REF2).split(b"\t")
    assert g[1] == b"16" and g[5] == b"2S12=" and g[9] == b"NN" + TEXT[3:15] and g[10] == bytes(range(50, 64))[::-1]
    assert len(g) == 15  # (one segment: no SA)
    # unmapped: one line, SEQ and QUAL as given
    assert sam_spec.sam_lines(b"r3 x", b"acgtn", None, (0, 0, 0, 0, []), REF2) == b"r3\t4\t*\t0\t0\t*\t*\t0\t0\tacgtn\t*\n"
    assert sam_spec.sam_lines(b"r3", b"ACG", b"!!#", (0, 0, 0, 0, []), REF2).endswith(b"\tACG\t!!#\n")


def test_header():
    assert sam_spec.header(REF2) == (b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrA\tLN:28\n@SQ\tSN:chrB\tLN:14\n"
                                     b"@PG\tID:slaMEM-hip\tPN:slaMEM-hip\n")


def test_the_replay_checker_refuses_a_wrong_md_a_wrong_nm_and_a_wrong_pos():
    letters, res = three_segment_read()
    good = sam_spec.header(REF2) + sam_spec.sam_lines(b"r1", letters, None, res, REF2)
    args = (REF2, [b"r1"], [letters], [res])
    assert sam_spec.replay_check(good, *args) == 3
    for a, b in ((b"MD:Z:4A3", b"MD:Z:4C3"), (b"MD:Z:4A3", b"MD:Z:8"), (b"NM:i:1", b"NM:i:2"), (b"\tchrA\t11\t", b"\tchrA\t12\t"),
                 (b"\t2048\tchrB", b"\t0\tchrB"), (b"chrB,3,+", b"chrB,4,+")):
        assert good.count(a) >= 1
        with pytest.raises(AssertionError):
            sam_spec.replay_check(good.replace(a, b, 1), *args)


@pytest.mark.parametrize("case", MEM_CASES)
def test_the_spec_file_of_the_golden_cases_replays(case):
    results, _, ref, qs, _ = map_spec.golden_map(case)
    letters = [qs.chars[qs.offsets[i]:qs.offsets[i + 1]] for i in range(qs.n)]
    quals = [bytes(33 + (k % 40) for k in range(len(l))) for l in letters]
    sam = sam_spec.sam_file(results, qs.names, letters, quals, ref)
    assert sam_spec.replay_check(sam, ref, qs.names, letters, results, quals) == sum(len(r[4]) for r in results if r[0])


# ---- the front end's writer -------------------------------------------------------------------------------------------------

def _sam_lib():
    L = hostlib.lib()
    L.slh_format_read_sam.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.c_uint64, C.POINTER(hostlib.Record), C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]
    L.slh_format_sam_header.argtypes = [C.POINTER(hostlib.Buffer), C.POINTER(hostlib.Record), C.c_int]
    return L


def _c_sam(L, name, letters, quals, res, T, ref_recs, merged_start, num):
    strand, mapq, s1, s2, segl = res
    segs, _, ops, ooff = aln_spec.pack([segl])
    segs32 = np.ascontiguousarray(segs, dtype=np.uint32)
    oo = np.ascontiguousarray(ooff, dtype=np.uint64)
    md, moff, _, prim = sam_spec.pack_md([res], T)
    mo = np.ascontiguousarray(moff, dtype=np.uint64)
    buf, s = hostlib.Buffer(), C.c_uint64()
    assert L.slh_format_read_sam(C.byref(buf), name, bytes(letters), bytes(quals) if quals is not None else None, len(letters), strand,
                                 mapq, s1, s2, segs32.ctypes.data if len(segl) else None, ops.ctypes.data if len(ops) else None,
                                 oo.ctypes.data, md.ctypes.data if len(md) else None, mo.ctypes.data, int(prim[0]), len(segl), ref_recs,
                                 merged_start, num, C.byref(s)) == 0
    out = C.string_at(buf.data, buf.len) if buf.len else b""
    L.slh_buffer_free(C.byref(buf))
    assert s.value == (sum(x[3] for x in segl) if strand else 0)
    return out


@pytest.mark.parametrize("with_quals", [False, True])
@pytest.mark.parametrize("case", MEM_CASES)
def test_front_end_writer_equals_the_spec_writer(case, with_quals):
    L = _sam_lib()
    results, _, ref, qs, _ = map_spec.golden_map(case)
    got, want = [], []
    for i, res in enumerate(results):
        letters = qs.chars[qs.offsets[i]:qs.offsets[i + 1]]
        quals = bytes(33 + ((7 * i + k) % 60) for k in range(len(letters))) if with_quals else None
        got.append(_c_sam(L, qs.names[i], letters, quals, res, ref.chars, ref.s.recs, ref.s.merged_start, ref.s.num))
        want.append(sam_spec.sam_lines(qs.names[i], letters, quals, res, ref))
    assert got == want
    assert b"".join(got).count(b"\n") == sum(len(r[4]) if r[0] else 1 for r in results)


@pytest.mark.parametrize("with_quals", [False, True])
def test_front_end_writer_on_an_unmapped_and_a_three_segment_read(with_quals):
    L = _sam_lib()
    recs = (hostlib.Record * 2)(hostlib.Record(b"chrA first", 28), hostlib.Record(b"chrB\tx", 14))
    starts = (C.c_uint32 * 2)(*REF2.merged_start)
    letters, res = three_segment_read()
    rev = (2, 12, 9, 3, [seg(5, 4, "===X==DD=="), seg(REF2.merged_start[1] + 1, 16, "==II===")])
    for name, l, r in ((b"r1 a read", letters, res), (b"r2", b"acgtnACGTN" * 3, (0, 0, 0, 0, [])), (b"r3\tz", b"ACGTNNacgtnnACGTACGTACGTAC", rev),
                       (b"r4", b"ACGT", (1, 0, 5, 5, []))):
        q = bytes(35 + k for k in range(len(l))) if with_quals else None
        assert _c_sam(L, name, l, q, r, REF2.chars, recs, starts, 2) == sam_spec.sam_lines(name, l, q, r, REF2)
    buf = hostlib.Buffer()
    assert L.slh_format_sam_header(C.byref(buf), recs, 2) == 0
    assert C.string_at(buf.data, buf.len) == sam_spec.header(REF2)
    L.slh_buffer_free(C.byref(buf))


def test_writer_under_asan_and_ubsan(tmp_path):
    """slamem_host.c and tests/sam_asan_driver.c (a program of its own) built with -fsanitize=address,undefined and run: no
    report, and the lines are the spec's."""
    cc = shutil.which("cc") or shutil.which("gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "slamem_amd", "csrc")
    exe = str(tmp_path / "sam_asan_driver")
    subprocess.check_call([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu99",
                           "-I", os.path.join(root, "include"), "-I", hostlib.HOST_DIR, "-o", exe,
                           os.path.join(root, "tests", "sam_asan_driver.c"), os.path.join(hostlib.HOST_DIR, "slamem_host.c"),
                           os.path.join(hostlib.HOST_DIR, "mem_image.c"), "-L", csrc, "-lslamem_hip", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-lpthread", "-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    letters, res = three_segment_read()
    assert letters == b"NATCCAATTNGCTTCCGANNACGTTGCANN"  # (the driver's read)
    q1 = bytes(range(40, 70))
    rev = (2, 60, 9, 0, [seg(5, 2, [("=", 3), ("X", 1), ("=", 2), ("D", 2), ("X", 1), ("=", 2)])])
    want = sam_spec.header(REF2)
    want += sam_spec.sam_lines(b"r1 a read", letters, q1, res, REF2) + sam_spec.sam_lines(b"r1 a read", letters, None, res, REF2)
    want += sam_spec.sam_lines(b"r2", b"acgtnACGTNACGT", b"0123456789:;<=", rev, REF2)
    want += sam_spec.sam_lines(b"r3 x", b"acgtn", None, (0, 0, 0, 0, []), REF2) + sam_spec.sam_lines(b"r3", b"ACG", b"!!#", (0, 0, 0, 0, []), REF2)
    assert r.stdout.startswith(want)
    big = r.stdout[len(want):].split(b"\t")
    assert big[0] == b"r4" and big[5] == b"2=2X" * 10000 and big[9] == b"A" * 40000 and big[12] == b"MD:Z:" + b"2C0G" * 10000 + b"0"
    assert r.stdout.endswith(b"s2:i:0\n")


# ---- the command line ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [["-sam", "ref.fa", "q.fq"], ["ref.fa", "-sam", "q.fq"], ["ref.fa", "q.fq", "-SAM"],
                                  ["-sam", "-maxed", "5", "-mgap", "100", "-pen", "2", "-xdrop", "3", "-b", "ref.fa", "q.fq"]])
def test_sam_sets_match_type_7_anywhere_and_takes_no_value(args):
    o = hostlib.parse_options(["slaMEM"] + args)
    assert o["match_type"] == 7 and o["num_files"] == 2 and o["files"] == ["ref.fa", "q.fq"] and not o["hidden_sort"]


OTHERS = ["-mam", "-mum", "-smem", "-chain", "-ext", "-aln", "-paf", "-pile", "-sites", "-vcf", "-cons", "-depth"]


@pytest.mark.parametrize("other", OTHERS)
def test_sam_with_another_mode_is_refused_before_any_work(other, tmp_path):
    assert hostlib.parse_options(["slaMEM", "-sam", other, "ref.fa", "q.fa"])["match_type"] == -1
    assert hostlib.parse_options(["slaMEM", other, "ref.fa", "-sam", "q.fa"])["match_type"] == -1
    exe = os.path.join(hostlib.HOST_DIR, "slaMEM-hip")
    out = tmp_path / "out.sam"
    for args in ([other, "-sam"], ["-sam", other]):
        r = subprocess.run([exe] + args + ["-o", str(out), "ref.fa", "q.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 255 and not out.exists()
        assert b"> ERROR: Option -sam excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites, -vcf, -cons and -depth" in r.stdout


@pytest.mark.parametrize("args,message", [
    (["-sam", "-maxed", "200"], b"> ERROR: Option -maxed needs a whole number from 0 to 127"),
    (["-sam", "-mgap", "0"], b"> ERROR: Option -mgap needs a whole number of at least 1"),
    (["-sam", "-occ", "3"], b"> ERROR: Option -occ needs -smem"),
    (["-sam", "-minq", "3"], b"> ERROR: Option -minq needs -pile"),
    (["-sam", "-bq", "3"], b"> ERROR: Option -bq needs -pile")])
def test_sam_takes_the_parameters_of_paf_and_no_others(args, message, tmp_path):
    exe = os.path.join(hostlib.HOST_DIR, "slaMEM-hip")
    out = tmp_path / "out.sam"
    r = subprocess.run([exe] + args + ["-o", str(out), "ref.fa", "q.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and not out.exists() and message in r.stdout


def test_the_hidden_sort_and_smem_are_untouched():
    assert hostlib.parse_options(["slaMEM", "-s", "mems.txt"])["hidden_sort"] == 1
    assert hostlib.parse_options(["slaMEM", "-sam", "ref.fa", "q.fa"])["hidden_sort"] == 0
    assert hostlib.parse_options(["slaMEM", "-smem", "ref.fa", "q.fa"])["match_type"] == 3
    assert hostlib.parse_options(["slaMEM", "-sites", "ref.fa", "q.fa"])["match_type"] == 8
    for tail, mt in (([], 0), (["-mam"], 1), (["-mum"], 2), (["-chain"], 4), (["-ext"], 5), (["-aln"], 6), (["-paf"], 7), (["-pile"], 8)):
        assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa"] + tail)["match_type"] == mt
