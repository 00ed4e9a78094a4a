"""-sb on the CPU: FS in C, through the engine and in tests/sb_spec.py, the host library's two formatters against
the spec on a list made by hand, the refusals of the command line, and the same formatters under the sanitizers in a program of
their own (tests/sb_asan_driver.c)."""
import ctypes as C
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import events_spec as es
import gt_spec as gs
import hostlib
import pile_spec
import sb_spec as ss
from test_map_host import FakeRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
CSRC = os.path.join(ROOT, "slamem_amd", "csrc")
DEFAULT = gs.params()

# the tables FS is compared on: every table with cells 0 .. 6, the issue's, one-sided ones, sums above the 400 of step 1
TABLES = list(itertools.product(range(7), repeat=4)) + [
    (10, 10, 10, 10), (20, 20, 20, 0), (0, 0, 0, 0), (50, 0, 0, 0), (0, 50, 0, 0), (0, 0, 50, 0), (0, 0, 0, 50), (30, 0, 0, 30), (0, 30, 30, 0),
    (30, 0, 30, 0), (0, 30, 0, 30), (100, 100, 100, 100), (100, 100, 100, 101), (200, 200, 0, 0), (200, 0, 200, 0), (200, 0, 0, 200),
    (3000, 2900, 40, 0), (3000, 2900, 0, 40), (2 ** 32 - 1,) * 4, (2 ** 32 - 1, 0, 0, 2 ** 32 - 1), (2 ** 32 - 1, 1, 1, 0), (401, 0, 0, 0),
    (100, 100, 100, 99), (150, 50, 50, 150), (1, 399, 1, 0), (250, 3, 2, 146), (1000000, 999999, 17, 3), (199, 1, 1, 199)]


def near(a: bytes, b: bytes) -> bool:
    """Two %.3f strings at most one unit of the last printed digit apart."""
    return a == b or abs(round(float(a) * 1000) - round(float(b) * 1000)) <= 1


# ---- FS ------------------------------------------------------------------------------------------------------------------------

def test_known_values_of_the_spec():
    assert ss.fisher_strand((10, 10, 10, 10)) == 0.0 and ss.fs_text((10, 10, 10, 10)) == b"0.000"
    assert ss.fisher_strand((0, 0, 0, 0)) == 0.0
    # (20, 20, 20, 0): the one-sided tail is C(40,20) / C(60,20) = 3.29e-5; the other side adds the tables at most as likely
    one_sided = math_comb(40, 20) / math_comb(60, 20)
    p = 10 ** (-ss.fisher_strand((20, 20, 20, 0)) / 10)
    assert one_sided <= p < 2 * one_sided and ss.fs_text((20, 20, 20, 0)) == b"44.507"
    # a table and its mirror images have one FS
    for t in ((5, 1, 0, 7), (20, 20, 20, 0), (3, 9, 4, 2)):
        rf, rr, af, ar = t
        assert len({ss.fs_text(t), ss.fs_text((rr, rf, ar, af)), ss.fs_text((af, ar, rf, rr))}) == 1
    assert ss.normalise((3000, 2900, 40, 0)) == (101, 97, 1, 0) and ss.normalise((100, 100, 100, 100)) == (100, 100, 100, 100)
    assert ss.normalise((100, 100, 100, 101)) == (49, 49, 49, 50) and ss.normalise((2 ** 32 - 1,) * 4) == (50, 50, 50, 50)


def math_comb(n, k):
    import math
    return math.comb(n, k)


def test_fs_agrees_between_c_the_engine_and_the_spec():
    from slamem_amd import capi, engine
    L = capi.lib()
    out = (C.c_uint32 * 4)()
    seen = set()
    for t in TABLES:
        arr = (C.c_uint32 * 4)(*t)
        L.slamem_fisher_strand_table(arr, out)
        assert tuple(int(v) for v in out) == engine.fisher_strand_table(t) == ss.normalise(t), t
        c, e, s = (b"%.3f" % float(L.slamem_fisher_strand(arr)), b"%.3f" % engine.fisher_strand(t), ss.fs_text(t))
        assert near(c, s) and near(e, s) and near(c, e), (t, c, e, s)
        assert float(s) >= 0.0 and not s.startswith(b"-")
        seen.add(s)
    assert len(seen) > 100 and ss.fs_text((10, 10, 10, 10)) == b"0.000" and float(ss.fs_text((20, 20, 20, 0))) > 40
    assert L.slamem_fisher_strand(None) == 0.0
    for bad in ((1, 2, 3), (1, 2, 3, -1), (0, 0, 0, 2 ** 32)):
        with pytest.raises(ValueError):
            engine.fisher_strand(bad)


# ---- the formatter -------------------------------------------------------------------------------------------------------------

def sb_case():
    """(ref, table, forward table, events): a het seen on both strands, a 1/2, a hom-alt seen on the forward strand only, an SNV
    under T, and events -- one whose anchor row has fewer forward observations than the event (df < af: rf stops at 0), one at the
    second record's first base, one that is not called."""
    recs = [b"ACGTTGCAAC", b"gGATCCATAG"]
    ref = FakeRef(recs, [b"first one", b"second\tx"])
    n = len(ref.chars)
    t, f = pile_spec.empty(n), pile_spec.empty(n)
    t[0], f[0] = (10, 10, 0, 0, 0, 0), (5, 5, 0, 0, 0, 0)        # A: 0/1 with C, balanced
    t[1], f[1] = (0, 1, 0, 19, 0, 0), (0, 0, 0, 19, 0, 0)        # C: 1/1 with T, T on forward reads only
    t[2], f[2] = (9, 0, 1, 9, 2, 0), (9, 0, 1, 0, 1, 0)          # G: 1/2, A forward and T reverse
    t[3], f[3] = (12, 0, 0, 8, 0, 1), (0, 0, 0, 8, 0, 1)         # T: 0/1 with A, the alternative on reverse reads only
    t[6], f[6] = (0, 20, 0, 0, 0, 0), (0, 3, 0, 0, 0, 0)         # C: the anchor of the events at 7: df = 3
    t[11], f[11] = (0, 0, 20, 0, 0, 0), (0, 0, 10, 0, 0, 0)      # g: the anchor of the events at the second record's start
    t[14], f[14] = (0, 0, 0, 12, 0, 0), (0, 0, 0, 12, 0, 0)
    ev = [(7, 1, 2, b"GA", 5, 4),       # anchor row 6: af = 5 > df = 3 -> rf = 0; rr = 17 - 4
          (7, 0, 2, b"", 10, 9),        # the same anchor: 1/1
          (11, 0, 2, b"", 6, 6),        # the second record's first base
          (11, 1, 3, b"TTA", 0, 20),    # the same place: reverse only, rr = 10 - 20 -> 0
          (15, 1, 1, b"C", 1, 0)]       # not called
    return ref, t, f, sorted(ev, key=es.order_key)


def record_inputs(ref, t, f, ev, p):
    """Per record what slh_format_vcf_sb_rows takes: name, start, size and the arrays."""
    pos, counts, gts = gs.genotypes(t, ref.chars, p)
    out = []
    for r, name in enumerate(ref.names):
        a, size = int(ref.merged_start[r]), int(ref.sizes[r])
        mine = (pos >= a) & (pos < a + size)
        evs = [e for e in ev if a <= e[0] < a + size]
        anchors = [e[0] - 1 if e[0] > a else e[0] for e in evs]
        rows = np.ascontiguousarray(t[anchors].astype(np.uint32).reshape(len(anchors), 6))
        frows = np.ascontiguousarray(f[anchors].astype(np.uint32).reshape(len(anchors), 6))
        eg, called = gs.genotype_events(evs, rows, p)
        p_, c_, g_ = (np.ascontiguousarray(x[mine]) for x in (pos, counts, gts))
        sf = np.ascontiguousarray(f[p_.astype(np.int64)].astype(np.uint32).reshape(len(p_), 6))
        out.append((name, a, size, p_, c_, sf, g_, es.to_records(evs), rows, frows, eg, called))
    return out


def host_sb_vcf(ref, t, f, ev, p, fs=None) -> bytes:
    L = hostlib.lib()
    vp = C.c_void_p
    L.slh_format_vcf_sb_header.argtypes = [C.POINTER(hostlib.Buffer), C.POINTER(hostlib.Record), C.c_int, C.c_int]
    L.slh_format_vcf_sb_rows.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, vp, vp, vp, vp, C.c_uint64,
                                         vp, vp, vp, vp, vp, C.c_uint64, C.c_int]
    recs = (hostlib.Record * len(ref.names))(*[hostlib.Record(nm, sz) for nm, sz in zip(ref.names, ref.sizes)])
    b = hostlib.Buffer()
    filt = -1 if fs is None else fs
    assert L.slh_format_vcf_sb_header(C.byref(b), recs, len(ref.names), filt) == 0
    for name, a, size, pos, counts, sf, gts, evs, rows, frows, eg, called in record_inputs(ref, t, f, ev, p):
        assert L.slh_format_vcf_sb_rows(C.byref(b), name, a, size, ref.chars, pos.ctypes.data, counts.ctypes.data, sf.ctypes.data,
                                        gts.ctypes.data, len(pos), evs.ctypes.data, rows.ctypes.data, frows.ctypes.data, eg.ctypes.data,
                                        called.ctypes.data, len(evs), filt) == 0
    out = C.string_at(b.data, b.len) if b.len else b""
    L.slh_buffer_free(C.byref(b))
    return out


def undecorate(vcf: bytes) -> bytes:
    """The -vcf -gt file inside a -vcf -gt -sb file."""
    out = []
    for line in vcf.split(b"\n")[:-1]:
        if line.startswith(b"##FILTER=") or line.startswith(b"##INFO=<ID=FS,") or line.startswith(b"##FORMAT=<ID=SB,"):
            continue
        if not line.startswith(b"#"):
            c = line.split(b"\t")
            c[6], c[7], c[8], c[9] = b".", c[7][:c[7].rindex(b";FS=")], c[8][:-3], c[9][:c[9].rindex(b":")]
            line = b"\t".join(c)
        out.append(line + b"\n")
    return b"".join(out)


def test_spec_file_written_out_by_hand():
    ref, t, f, ev = sb_case()
    got = ss.vcf_file(t, f, ev, ref, DEFAULT)
    head = ss.vcf_header(ref)
    assert got.startswith(head) and head.count(b"##INFO=<ID=") == 5 and head.count(b"##FORMAT=<ID=") == 6 and b"##FILTER" not in head
    assert b'##FORMAT=<ID=SB,Number=4,Type=Integer,' in head and b'##INFO=<ID=FS,Number=1,Type=Float,' in head
    body = got[len(head):].split(b"\n")[:-1]
    assert len(body) == 8
    assert body[0] == b"first\t1\t.\tA\tC\t157\t.\tDP=20;AO=10;FS=0.000\tGT:DP:AD:GQ:PL:SB\t0/1:20:10,10:99:187,0,187:5,5,5,5"
    assert body[1].startswith(b"first\t2\t.\tC\tT\t") and body[1].endswith(b":0,1,19,0") and b";FS=" + ss.fs_text((0, 1, 19, 0)) + b"\t" in body[1]
    assert body[2].startswith(b"first\t3\t.\tG\tA,T\t") and body[2].endswith(b":1,0,9,9")  # (two alternatives: summed)
    assert body[3].startswith(b"first\t4\t.\tT\tA\t") and body[3].endswith(b":8,0,0,12") and float(body[3].split(b";FS=")[1].split(b"\t")[0]) > 30
    assert body[4].startswith(b"first\t7\t.\tCAA\tC\t") and body[4].endswith(b":0,8,10,9")  # (df = 3 < af = 10; rr = 17 - 9)
    assert body[5].startswith(b"first\t7\t.\tC\tCGA\t") and body[5].endswith(b":0,13,5,4")
    assert body[6].startswith(b"second\t1\t.\tGGA\tA\t") and body[6].endswith(b":4,4,6,6")
    assert body[7].startswith(b"second\t1\t.\tG\tTTAG\t") and body[7].endswith(b":10,0,0,20")
    assert undecorate(got) == gs.vcf_file(t, ev, ref, DEFAULT)
    # -fs 30: a line on each side
    filt = ss.vcf_file(t, f, ev, ref, DEFAULT, 30)
    assert filt.startswith(ss.vcf_header(ref, 30)) and b'##FILTER=<ID=sb,Description="Strand bias: FS above 30">\n' in filt
    cols = [line.split(b"\t") for line in filt[len(ss.vcf_header(ref, 30)):].split(b"\n")[:-1]]
    assert [c[6] for c in cols].count(b"sb") >= 2 and [c[6] for c in cols].count(b"PASS") >= 2 and cols[0][6] == b"PASS" and cols[3][6] == b"sb"
    assert undecorate(filt) == gs.vcf_file(t, ev, ref, DEFAULT)
    # ploidy 1
    one = ss.vcf_file(t, f, ev, ref, gs.params(ploidy=1))
    assert b"\tGT:DP:AD:GQ:PL:SB\t1:20:1,19:" in one and undecorate(one) == gs.vcf_file(t, ev, ref, gs.params(ploidy=1))


CASES = [(DEFAULT, None), (DEFAULT, 30), (DEFAULT, 0), (DEFAULT, 999), (gs.params(ploidy=1), None), (gs.params(ploidy=1), 10),
         (gs.params(min_qual=0, min_depth=1), 5), (gs.params(min_depth=21), None)]


@pytest.mark.parametrize("p,fs", CASES)
def test_host_formatter_against_the_spec(p, fs):
    ref, t, f, ev = sb_case()
    want = ss.vcf_file(t, f, ev, ref, p, fs)
    assert host_sb_vcf(ref, t, f, ev, p, fs) == want
    assert undecorate(want) == gs.vcf_file(t, ev, ref, p)


def test_host_formatter_large_counters():
    rng = np.random.default_rng(4)
    body = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=300))
    ref = FakeRef([body], [b"chr 1"])
    t, f = pile_spec.empty(len(body)), pile_spec.empty(len(body))
    col = b"ACGT".index(body[101:102])
    t[101, col], t[101, (col + 1) % 4] = 2 ** 31 - 1, 2 ** 31 - 1
    f[101, col], f[101, (col + 1) % 4] = 2 ** 31 - 1, 7
    p, _ = es.normalise(body, 150, 0, 127)
    ev = [(p, 0, 127, b"", 2 ** 32 - 1, 2 ** 32 - 1)]
    t[p - 1] = (2 ** 32 - 1,) * 6
    f[p - 1] = (2 ** 32 - 1, 2 ** 32 - 1, 5, 0, 0, 0)
    got = host_sb_vcf(ref, t, f, ev, DEFAULT, 60)
    assert got == ss.vcf_file(t, f, ev, ref, DEFAULT, 60)
    assert b":2147483647,0,7,2147483640\n" in got and b":4294967295,4294967295,4294967295,4294967295\n" in got


# ---- the command line ----------------------------------------------------------------------------------------------------------

def test_options_of_the_parser():
    o = hostlib.parse_options(["slaMEM", "-vcf", "-gt", "ref.fa", "reads.fa"])  # -vcf -gt parses as before
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"]
    assert hostlib.parse_run(["slaMEM", "-vcf", "-gt", "ref.fa", "reads.fa"])[:2] == (0, None)
    o = hostlib.parse_options(["slaMEM", "-vcf", "-gt", "-sb", "ref.fa", "-FS", "30", "reads.fa"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"]
    assert ("sb", False) in hostlib.option_rows() and ("fs", True) in hostlib.option_rows()
    L = hostlib.lib()
    L.slh_parse_sb_params.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int)]

    def sb(args):
        v = C.c_int()
        return L.slh_parse_sb_params(len(args), hostlib.c_argv(args), C.byref(v)), v.value
    assert sb(["x", "-vcf", "-gt", "a", "b"]) == (0, -1)
    assert sb(["x", "-sb", "a", "b"]) == (1, -1) and sb(["x", "-SB", "-fs", "0"]) == (3, 0) and sb(["x", "-fs", "999"]) == (2, 999)
    assert sb(["x", "-fs", "1", "-fs", "7", "-sb"]) == (3, 7)
    for bad in (["-fs", "1000"], ["-fs", "-1"], ["-fs", "x"], ["-fs", "3x"], ["-sb", "-fs"]):
        assert sb(["x"] + bad)[0] == -1, bad
    for args, refusal in ((["-vcf", "-gt", "-sb"], None), (["-vcf", "-gt", "-sb", "-fs", "30"], None), (["-vcf", "-sb"], "Option -sb needs -gt"),
                          (["-vcf", "-gt", "-fs", "30"], "Option -fs needs -sb"), (["-vcf", "-gt", "-sb", "-fs", "1000"],
                                                                                  "Option -fs needs a whole number from 0 to 999")):
        rc, msg, _ = hostlib.parse_run(["slaMEM"] + args + ["ref.fa", "reads.fa"])
        assert (rc, msg) == ((0, None) if refusal is None else (-1, refusal)), args


def write_fasta(path, records):
    with open(path, "wb") as fh:
        for name, letters in records:
            fh.write(b">" + name + b"\n" + bytes(letters) + b"\n")


REFUSALS = [
    (["-sb"], b"Option -sb needs -gt"),
    (["-vcf", "-sb"], b"Option -sb needs -gt"),
    (["-pile", "-sb"], b"Option -sb needs -gt"),
    (["-gt", "-sb"], b"Option -gt needs -vcf"),
    (["-vcf", "-gt", "-fs", "30"], b"Option -fs needs -sb"),
    (["-vcf", "-fs", "30"], b"Option -fs needs -sb"),
    (["-vcf", "-gt", "-sb", "-fs", "1000"], b"Option -fs needs a whole number from 0 to 999"),
    (["-vcf", "-gt", "-sb", "-fs", "-1"], b"Option -fs needs a whole number from 0 to 999"),
    (["-vcf", "-gt", "-sb", "-fs"], b"Option -fs needs a whole number from 0 to 999"),
    # the wording of the earlier refusals stands
    (["-vcf", "-gt", "-sb", "-mpct", "30"], b"Option -mpct has no meaning with -gt: a call is made when its genotype's quality reaches -qual"),
    (["-vcf", "-qual", "20", "-sb"], b"Option -qual needs -gt"),
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


def test_usage_lists_the_options():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    assert b"\t-sb\t" in r.stdout and b"\t-fs\t" in r.stdout and b"\t-gt\t" in r.stdout


# ---- the sanitizer run ---------------------------------------------------------------------------------------------------------

def case_blob(ref, t, f, ev, p, fs) -> bytes:
    """The case as tests/sb_asan_driver.c reads it: little-endian 64-bit numbers and the arrays as they are."""
    def u64(*v):
        return struct.pack("<%dQ" % len(v), *v)
    out = [struct.pack("<q", -1 if fs is None else fs), u64(len(ref.names))]
    for name, size in zip(ref.names, ref.sizes):
        out += [u64(len(name)), name, u64(size)]
    out += [u64(len(ref.chars)), ref.chars]
    for name, a, size, pos, counts, sf, gts, evs, rows, frows, eg, called in record_inputs(ref, t, f, ev, p):
        out += [u64(a, size, len(pos)), pos.tobytes(), counts.tobytes(), sf.tobytes(), gts.tobytes(), u64(len(evs)), evs.tobytes(),
                rows.tobytes(), frows.tobytes(), eg.tobytes(), called.tobytes()]
    return b"".join(out)


def test_fs_and_formatters_under_asan_and_ubsan(tmp_path):
    """slamem_host.c and tests/sb_asan_driver.c (a program of its own) built with -fsanitize=address,undefined: slamem_fisher_strand on
    the tables above and the two formatters on the hand-made cases -- no report, and the bytes the spec gives."""
    cc = shutil.which("cc") or shutil.which("gcc")
    exe = str(tmp_path / "sb_asan_driver")
    subprocess.check_call([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu99",
                           "-I", os.path.join(ROOT, "include"), "-I", hostlib.HOST_DIR, "-o", exe,
                           os.path.join(ROOT, "tests", "sb_asan_driver.c"), os.path.join(hostlib.HOST_DIR, "slamem_host.c"),
                           os.path.join(hostlib.HOST_DIR, "mem_image.c"), "-L", CSRC, "-lslamem_hip", "-Wl,-rpath," + CSRC,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-lpthread", "-lm"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", ASAN_OPTIONS="detect_leaks=1")
    tables = str(tmp_path / "tables.txt")
    with open(tables, "w") as fh:
        for t in TABLES:
            fh.write("%d %d %d %d\n" % t)
    r = subprocess.run([exe, "tables", tables], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode(errors="replace")[-3000:]
    lines = r.stdout.split(b"\n")[:-1]
    assert len(lines) == len(TABLES)
    for t, line in zip(TABLES, lines):
        norm, fs = line.rsplit(b" ", 1)
        assert norm == b"%d %d %d %d" % ss.normalise(t) and near(fs, ss.fs_text(t)), (t, line)
    ref, t, f, ev = sb_case()
    for k, (p, fs) in enumerate(CASES):
        path = str(tmp_path / ("case%d.bin" % k))
        open(path, "wb").write(case_blob(ref, t, f, ev, p, fs))
        r = subprocess.run([exe, "case", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert r.returncode == 0 and r.stderr == b"", r.stderr.decode(errors="replace")[-3000:]
        assert r.stdout == ss.vcf_file(t, f, ev, ref, p, fs), (p, fs)
