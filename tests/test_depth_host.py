"""-depth without a GPU: tests/depth_spec.py (the definition of DESIGN.md 4.20) on a table worked out by hand, the property that a
range's runs and sums are a slice of the whole table's, the host library's formatters against the spec's files (fed range by
range as the front end feeds them), the options, and the closed form of the known answer of test_gpu_depth.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_spec as ds
import ext_spec
import hostlib
from test_map_host import FakeRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
COVER_SEED = 20262  # (fixed: test_cover_sample_answer_holds_on_the_definition confirms the closed form on the definition alone)


def table_of(depths, column=0):
    t = np.zeros((len(depths), 6), dtype=np.int64)
    t[:, column] = depths
    return t


def pairs(r):
    return [(int(p), int(v)) for p, v in zip(*r)]


# ---- the definition ------------------------------------------------------------------------------------------------------------

def hand_table():
    #    row 0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15  16  17 18 19
    d = [0, 0, 3, 3, 4, 4, 4, 29, 30, 31, 30, 0, 0, 1, 1, 5, 2 ** 33, 5, 0, 0]
    t = table_of(d)
    t[3] = (1, 0, 0, 0, 2, 9)        # the same depth in other columns, and an I that counts nowhere
    t[5] = (0, 1, 1, 1, 1, 0)
    t[16] = (2 ** 32 - 1, 2 ** 32 - 1, 2, 0, 0, 7)
    assert ds.depth(t) == d[:16] + [2 ** 33, 5, 0, 0]
    return t


def test_runs_written_out_by_hand():
    t = hand_table()
    exact = [(0, 0), (2, 3), (4, 4), (7, 29), (8, 30), (9, 31), (10, 30), (11, 0), (13, 1), (15, 5), (16, 2 ** 33), (17, 5), (18, 0)]
    assert pairs(ds.runs(t)) == exact
    pos, val = ds.runs(t)
    assert pos.dtype == np.uint64 and val.dtype == np.uint64
    # one level: covered or not
    assert pairs(ds.runs(t, (1,))) == [(0, 0), (2, 1), (11, 0), (13, 1), (18, 0)]
    # a level met exactly (30, at rows 8 and 10) and missed by one (29, at row 7; 4 against 3, 5 against 4)
    assert pairs(ds.runs(t, (4, 30))) == [(0, 0), (4, 1), (8, 2), (11, 0), (15, 1), (16, 2), (17, 1), (18, 0)]
    assert pairs(ds.runs(t, (5, 31))) == [(0, 0), (7, 1), (9, 2), (10, 1), (11, 0), (15, 1), (16, 2), (17, 1), (18, 0)]
    assert pairs(ds.runs(t, (1, 4, 30))) == [(0, 0), (2, 1), (4, 2), (8, 3), (11, 0), (13, 1), (15, 2), (16, 3), (17, 2), (18, 0)]
    assert pairs(ds.runs(t, tuple(range(1, 17))))[:4] == [(0, 0), (2, 3), (4, 4), (7, 16)]
    # ranges: the first row of a range is a head whatever stands in front of it; an empty range has no run
    assert pairs(ds.runs(t, (), 5, 4)) == [(5, 4), (7, 29), (8, 30)]
    assert pairs(ds.runs(t, (), 12, 1)) == [(12, 0)] and pairs(ds.runs(t, (), 20, 0)) == [] and pairs(ds.runs(t, (), 0, 0)) == []
    # the sums: depth and rows of at least min_depth in front of each bound
    assert ds.cum(t, 1, 0, [0, 2, 4, 11, 20]).tolist() == [[0, 0], [0, 0], [6, 2], [138, 9], [138 + 12 + 2 ** 33, 14]]
    assert ds.cum(t, 4, 4, [4, 4, 11, 17, 20]).tolist() == [[0, 0], [0, 0], [132, 7], [139 + 2 ** 33, 9], [144 + 2 ** 33, 10]]
    assert ds.cum(t, 2 ** 31 - 1, 0, [20]).tolist() == [[138 + 12 + 2 ** 33, 1]]
    assert ds.cum(t, 1, 7, []).shape == (0, 2)
    for bad in ((0,), (3, 3), (4, 2), tuple(range(1, 18)), (2 ** 32,)):
        with pytest.raises(ValueError):
            ds.runs(t, bad)


def clip(whole, first, count):
    """The whole table's runs clipped to [first, first + count)."""
    pos, val = whole
    out = []
    for i in range(len(pos)):
        s, e = int(pos[i]), int(pos[i + 1]) if i + 1 < len(pos) else first + count
        if max(s, first) < min(e, first + count):
            out.append((max(s, first), int(val[i])))
    return out


def test_any_range_is_a_slice_of_the_whole():
    rng = np.random.default_rng(193)
    runs_seen = 0
    for _ in range(200):
        n = int(rng.integers(1, 60))
        t = rng.integers(0, 3, size=(n, 6)) * rng.integers(0, 2, size=(n, 1)) * (rng.random((n, 1)) < 0.7)
        t = np.repeat(t, rng.integers(1, 4, size=n), axis=0)[:n]  # (stretches of equal rows)
        m = int(rng.integers(0, 4))
        levels = tuple(sorted(set(int(x) for x in rng.integers(1, 8, size=m))))
        md = int(rng.integers(1, 5))
        whole = ds.runs(t, levels)
        assert len(whole[0]) and int(whole[0][0]) == 0 and all(a != b for a, b in zip(whole[1], whole[1][1:]))
        wc = ds.cum(t, md, 0, range(n + 1))
        runs_seen += len(whole[0])
        for first, count in [(0, 0), (n, 0), (0, n)] + [(int(a), int(rng.integers(0, n - a + 1))) for a in rng.integers(0, n + 1, size=6)]:
            assert pairs(ds.runs(t, levels, first, count)) == clip(whole, first, count)
            b = list(range(first, first + count + 1))
            part = ds.cum(t, md, first, b)
            assert np.array_equal(part, wc[first:first + count + 1] - wc[first])
    assert runs_seen > 1000


# ---- the host library's formatters ---------------------------------------------------------------------------------------------

class Run(C.Structure):
    _fields_ = [("pos", C.c_uint64), ("value", C.c_uint64)]


class Pending(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("value", C.c_uint64), ("open", C.c_int)]


def host():
    L = hostlib.lib()
    B = C.POINTER(hostlib.Buffer)
    L.slh_format_depth_runs.argtypes = [B, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(Run), C.c_uint64, C.POINTER(Pending)]
    L.slh_format_depth_flush.argtypes = [B, C.c_char_p, C.POINTER(Pending)]
    L.slh_format_depth_windows.argtypes = [B, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    L.slh_format_depth_summary.argtypes = [B, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64]
    return L


def front_end(t, ref, levels=(), window=0, min_depth=1, chunk=1 << 24):
    """(file, summary) as the front end builds them: ranges of `chunk` rows, of each the spec's runs and its cum at the bounds
    the front end asks for, the host library's formatters on the records' pieces."""
    L = host()
    buf, sbuf, pend = hostlib.Buffer(), hostlib.Buffer(), Pending()
    n = len(t)
    recs = [(ref.names[r], a, size) for r, (_, a, size) in enumerate(ds.records(ref))]
    r, rec_sum, rec_cov, wacc = 0, 0, 0, 0
    for x0 in range(0, n, chunk):
        cnt = min(chunk, n - x0)
        bnd = []
        for name, start, size in recs[r:]:
            if start >= x0 + cnt:
                break
            a, b = max(start, x0), min(start + size, x0 + cnt)
            bnd.append(a)
            if window:
                bnd += [start + q * window for q in range((a - start) // window + 1, (b - start - 1) // window + 1)]
            bnd.append(b)
        pos, val = ds.runs(t, levels, x0, cnt) if not window else ([], [])
        runs = (Run * max(len(pos), 1))(*[Run(int(p), int(v)) for p, v in zip(pos, val)])
        cum = np.ascontiguousarray(ds.cum(t, min_depth, x0, bnd))
        j = 0
        while j < len(bnd):
            name, start, size = recs[r]
            end, ja, a = start + size, j, bnd[j]
            j += 1
            while bnd[j] < end and bnd[j] < x0 + cnt:
                j += 1
            b = bnd[j]
            if window:
                k = j - ja - (0 if b == end or (b - start) % window == 0 else 1)
                sum0 = (int(cum[ja][0]) - wacc) % 2 ** 64
                assert L.slh_format_depth_windows(C.byref(buf), name, size, window, (a - start) // window, sum0,
                                                  cum[ja + 1:].ctypes.data if ja + 1 < len(cum) else None, k) == 0
                wacc = int(cum[j][0]) - (int(cum[ja + k][0]) if k else int(cum[ja][0]) - wacc)
            else:
                assert L.slh_format_depth_runs(C.byref(buf), name, start, a, b, runs, len(pos), C.byref(pend)) == 0
            rec_sum += int(cum[j][0]) - int(cum[ja][0])
            rec_cov += int(cum[j][1]) - int(cum[ja][1])
            j += 1
            if b < end:
                break
            assert L.slh_format_depth_flush(C.byref(buf), name, C.byref(pend)) == 0
            assert L.slh_format_depth_summary(C.byref(sbuf), name, size, rec_cov, rec_sum) == 0
            r, rec_sum, rec_cov, wacc = r + 1, 0, 0, 0
    assert r == len(recs) and not pend.open
    out = [C.string_at(x.data, x.len) if x.len else b"" for x in (buf, sbuf)]
    for x in (buf, sbuf):
        L.slh_buffer_free(C.byref(x))
    return out


def three_records():
    """Records of 9, 5 and 12 rows behind each other (separators at 9 and 15).  The first ends inside a run of depth 7 that goes
    on over the separator into the second; the third starts with depth 0 and ends with it."""
    ref = FakeRef([b"ACGTACGTA", b"CCGGT", b"ACGTACGTACGT"], [b"one first", b"two\tsecond", b"three"])
    #     one: 0..8                      sep  two: 10..14    sep  three: 16..27
    d = [2, 2, 0, 0, 5, 7, 7, 7, 7] + [7] + [7, 7, 1, 1, 1] + [1] + [0, 0, 3, 3, 3, 3, 2 ** 32 + 5, 4, 4, 0, 0, 0]
    assert len(d) == len(ref.chars) == 28
    t = table_of(d, 4)
    t[22] = (2 ** 32 - 1, 0, 0, 0, 6, 1)
    return ref, t


def test_spec_files_of_three_records_by_hand():
    ref, t = three_records()
    assert ds.bedgraph_file(t, ref) == (b"one\t0\t2\t2\n" b"one\t2\t4\t0\n" b"one\t4\t5\t5\n" b"one\t5\t9\t7\n"
                                        b"two\t0\t2\t7\n" b"two\t2\t5\t1\n"
                                        b"three\t0\t2\t0\n" b"three\t2\t6\t3\n" b"three\t6\t7\t4294967301\n" b"three\t7\t9\t4\n"
                                        b"three\t9\t12\t0\n")
    assert ds.bedgraph_file(t, ref, (1, 4)) == (b"one\t0\t2\t1\n" b"one\t2\t4\t0\n" b"one\t4\t9\t2\n" b"two\t0\t2\t2\n" b"two\t2\t5\t1\n"
                                                b"three\t0\t2\t0\n" b"three\t2\t6\t1\n" b"three\t6\t9\t2\n" b"three\t9\t12\t0\n")
    # windows of 4: 9 = 4 + 4 + 1, 5 = 4 + 1, 12 = 4 + 4 + 4; means floored to hundredths
    assert ds.window_file(t, ref, 4) == (b"one\t0\t4\t1.00\n" b"one\t4\t8\t6.50\n" b"one\t8\t9\t7.00\n" b"two\t0\t4\t4.00\n" b"two\t4\t5\t1.00\n"
                                         b"three\t0\t4\t1.50\n" b"three\t4\t8\t1073741827.75\n" b"three\t8\t12\t1.00\n")
    # a window longer than every record: a line per record
    assert ds.window_file(t, ref, 100) == b"one\t0\t9\t4.11\n" b"two\t0\t5\t3.40\n" b"three\t0\t12\t357913943.41\n"
    assert ds.summary_lines(t, ref, 1) == (b"> Depth of one: 9 positions, 7 covered (77.77 %), mean depth 4.11\n"
                                           b"> Depth of two: 5 positions, 5 covered (100.00 %), mean depth 3.40\n"
                                           b"> Depth of three: 12 positions, 7 covered (58.33 %), mean depth 357913943.41\n")
    assert ds.summary_lines(t, ref, 4).count(b" 3 covered ") == 1


@pytest.mark.parametrize("chunk", [1 << 24, 11, 7, 3, 1])
def test_host_formatters_against_the_spec(chunk):
    """Whatever the ranges: one range, ranges whose borders fall inside a run (chunk 11: inside the run of depth 7 of record two
    and inside that of depth 3 of record three), ranges of a single row."""
    ref, t = three_records()
    for levels in ((), (1, 4), (1,), (7,), (8,)):
        got, summary = front_end(t, ref, levels, chunk=chunk)
        assert got == ds.bedgraph_file(t, ref, levels) and summary == ds.summary_lines(t, ref, 1)
    for window in (1, 2, 4, 5, 9, 12, 13, 100):
        got, summary = front_end(t, ref, window=window, min_depth=4, chunk=chunk)
        assert got == ds.window_file(t, ref, window) and summary == ds.summary_lines(t, ref, 4)


def test_host_formatters_on_random_records():
    rng = np.random.default_rng(197)
    for _ in range(30):
        sizes = rng.integers(1, 40, size=int(rng.integers(1, 5)))
        ref = FakeRef([b"A" * int(s) for s in sizes], [b"r%d x" % i for i in range(len(sizes))])
        n = len(ref.chars)
        t = np.repeat(rng.integers(0, 3, size=(n, 6)), rng.integers(1, 6, size=n), axis=0)[:n]
        chunk = int(rng.integers(1, n + 2))
        levels = tuple(sorted(set(int(x) for x in rng.integers(1, 9, size=int(rng.integers(0, 3))))))
        assert front_end(t, ref, levels, chunk=chunk) == [ds.bedgraph_file(t, ref, levels), ds.summary_lines(t, ref, 1)]
        w = int(rng.integers(1, 50))
        assert front_end(t, ref, window=w, min_depth=3, chunk=chunk) == [ds.window_file(t, ref, w), ds.summary_lines(t, ref, 3)]


def test_host_formatters_large_numbers_and_names():
    L = host()
    b, pend = hostlib.Buffer(), Pending()
    runs = (Run * 2)(Run(5_000_000_000, 5 * (2 ** 32 - 1)), Run(5_000_000_100, 0))
    assert L.slh_format_depth_runs(C.byref(b), b"chr 1\tx", 4_000_000_000, 5_000_000_050, 5_000_000_200, runs, 2, C.byref(pend)) == 0
    assert L.slh_format_depth_flush(C.byref(b), b"chr 1\tx", C.byref(pend)) == 0
    assert L.slh_format_depth_flush(C.byref(b), b"chr 1\tx", C.byref(pend)) == 0  # (nothing open: nothing written)
    cum = np.array([[2 ** 63, 1], [2 ** 63 + 1999, 2]], dtype=np.uint64)
    assert L.slh_format_depth_windows(C.byref(b), b"chr 1\tx", 2 ** 33 + 1000, 2 ** 32, 1, 5, cum.ctypes.data, 2) == 0
    assert L.slh_format_depth_summary(C.byref(b), b"chr 1\tx", 0, 0, 0) == 0
    assert C.string_at(b.data, b.len) == (b"chr\t1000000050\t1000000100\t21474836475\n" b"chr\t1000000100\t1000000200\t0\n"
                                          b"chr\t4294967296\t8589934592\t%s\n" b"chr\t8589934592\t8589935592\t1.99\n"
                                          b"> Depth of chr: 0 positions, 0 covered (0.00 %%), mean depth 0.00\n"
                                          % ds.hundredths(100 * (2 ** 63 - 5) // 2 ** 32))
    L.slh_buffer_free(C.byref(b))


# ---- the options ---------------------------------------------------------------------------------------------------------------

def depth_params(args):
    L = hostlib.lib()
    L.slh_parse_depth_params.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    argv = (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)
    lv, k, w = (C.c_uint32 * 16)(), C.c_int(), C.c_uint64()
    rc = L.slh_parse_depth_params(len(args), argv, lv, C.byref(k), C.byref(w))
    return rc, list(lv[:k.value]), w.value


def test_options_of_the_parser():
    o = hostlib.parse_options(["slaMEM", "-depth", "-lev", "1,4,30", "-win", "100", "ref.fa", "reads.fa"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"] and o["min_mem_len"] == 20 and o["hidden_clean"] == 0
    o = hostlib.parse_options(["slaMEM", "ref.fa", "-WIN", "7", "-mdep", "3", "reads.fa", "-DEPTH", "-b", "-l", "14"])
    assert o["match_type"] == 8 and o["files"] == ["ref.fa", "reads.fa"] and o["both_strands"] == 1 and o["min_mem_len"] == 14
    for other in ("-mam", "-mum", "-smem", "-chain", "-ext", "-aln", "-paf", "-pile", "-sites", "-vcf", "-cons"):
        assert hostlib.parse_options(["slaMEM", "ref.fa", other, "reads.fa", "-depth"])["match_type"] == -1
    # the other modes are what they were
    assert hostlib.parse_options(["slaMEM", "-cons", "ref.fa", "reads.fa"])["match_type"] == 8
    assert hostlib.parse_options(["slaMEM", "-chain", "ref.fa", "reads.fa"])["match_type"] == 4
    assert hostlib.parse_options(["slaMEM", "ref.fa", "reads.fa"])["match_type"] == 0
    assert depth_params(["x", "-depth", "a", "b"]) == (0, [], 0)
    assert depth_params(["x", "-lev", "1,4,30", "-depth"]) == (1, [1, 4, 30], 0)
    assert depth_params(["x", "-LEV", "7"]) == (1, [7], 0)
    assert depth_params(["x", "-win", "100"]) == (2, [], 100)
    assert depth_params(["x", "-win", "1", "-lev", "1,4294967295"]) == (3, [1, 4294967295], 1)
    assert depth_params(["x", "-lev", ",".join(str(k) for k in range(1, 17))])[1] == list(range(1, 17))
    # -l alone is the minimum match length, and its value is no list
    assert depth_params(["x", "-l", "1,2", "-b"]) == (0, [], 0)
    for bad in (["-lev"], ["-lev", ""], ["-lev", "0"], ["-lev", "3,3"], ["-lev", "4,1"], ["-lev", "1,"], ["-lev", ",1"], ["-lev", "1;2"],
                ["-lev", "x"], ["-lev", "-1"], ["-lev", "4294967296"], ["-lev", ",".join(str(k) for k in range(1, 18))]):
        assert depth_params(["x"] + bad)[0] == -1, bad
    for bad in (["-win"], ["-win", "0"], ["-win", "x"], ["-win", "-3"], ["-win", "5x"], ["-win", "1.5"]):
        assert depth_params(["x"] + bad)[0] == -2, bad


def test_usage_lists_the_options():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    line = next(l for l in r.stdout.split(b"\n") if l.startswith(b"\t-depth\t"))
    for word in (b"-mdep", b"-lev", b"-win", b"bedGraph"):
        assert word in line
    for opt in (b"\t-cons\t", b"\t-vcf\t", b"\t-sites\t", b"\t-pile\t"):
        assert opt in r.stdout


def write_fasta(path, records):
    with open(path, "wb") as f:
        for name, letters in records:
            f.write(b">" + name + b"\n" + bytes(letters) + b"\n")


DEPTH_EXCLUDES = b"Option -depth excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites, -vcf and -cons"
REFUSALS = [
    (["-depth", "-cons"], DEPTH_EXCLUDES),
    (["-cons", "-depth"], DEPTH_EXCLUDES),
    (["-vcf", "-depth"], DEPTH_EXCLUDES),
    (["-depth", "-sites"], DEPTH_EXCLUDES),
    (["-pile", "-depth"], DEPTH_EXCLUDES),
    (["-depth", "-paf"], DEPTH_EXCLUDES),
    (["-aln", "-depth"], DEPTH_EXCLUDES),
    (["-depth", "-ext"], DEPTH_EXCLUDES),
    (["-chain", "-depth"], DEPTH_EXCLUDES),
    (["-depth", "-smem"], DEPTH_EXCLUDES),
    (["-mum", "-depth"], DEPTH_EXCLUDES),
    (["-depth", "-mam"], DEPTH_EXCLUDES),
    (["-depth", "-cons", "-vcf"], DEPTH_EXCLUDES),
    (["-depth", "-mpct", "20"], b"Option -mpct has no meaning with -depth"),
    (["-mdep", "3", "-mpct", "0", "-depth"], b"Option -mpct has no meaning with -depth"),
    (["-depth", "-mdep", "0"], b"Option -mdep needs a whole number of at least 1"),
    (["-depth", "-mpct", "101"], b"Option -mpct needs a whole number from 0 to 100"),
    (["-depth", "-lev", "1,4", "-win", "100"], b"Options -lev and -win exclude each other"),
    (["-win", "100", "-depth", "-lev", "3"], b"Options -lev and -win exclude each other"),
    (["-lev", "1,4"], b"Options -lev and -win need -depth"),
    (["-pile", "-win", "100"], b"Options -lev and -win need -depth"),
    (["-cons", "-lev", "1", "-win", "5"], b"Options -lev and -win need -depth"),
    (["-depth", "-lev", "4,1"], b"Option -lev needs 1 to 16 whole numbers of at least 1, ascending, separated by commas"),
    (["-depth", "-lev", "0"], b"Option -lev needs 1 to 16 whole numbers"),
    (["-depth", "-win", "0"], b"Option -win needs a whole number of at least 1"),
    (["-depth", "-minq", "61"], b"Option -minq needs a whole number from 0 to 60"),
    (["-depth", "-evs", "1024"], b"Option -evs needs -vcf"),
    (["-depth", "-occ", "3"], b"Option -occ needs -smem"),
    # the wording of the earlier refusals stands
    (["-cons", "-vcf"], b"Option -cons excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -pile, -sites and -vcf"),
    (["-cons", "-mpct", "20"], b"Option -mpct has no meaning with -cons"),
    (["-pile", "-sites"], b"Option -sites excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf and -pile"),
    (["-paf", "-mdep", "3"], b"Options -mdep and -mpct need -sites"),
    (["-mdep", "3"], b"Options -mdep and -mpct need -sites"),
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


# ---- the known answer of test_gpu_depth.py -------------------------------------------------------------------------------------

def cover_sample(seed: int, n: int = 12000, read_len: int = 150, step: int = 5):
    """A random reference over A,C,G,T and error-free reads of read_len letters that start at every `step`-th position,
    alternating strands.  Returns (reference, reads, offsets)."""
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    reads = []
    for k, a in enumerate(range(0, n - read_len + 1, step)):
        r = ref[a:a + read_len]
        reads.append(ext_spec.revcomp(r) if k % 2 else r.copy())
    off = np.arange(len(reads) + 1, dtype=np.uint64) * np.uint64(read_len)
    return ref, np.concatenate(reads), off


def cover_depth(n: int = 12000, read_len: int = 150, step: int = 5):
    """d(p) = the number of k with step k <= p < step k + read_len and step k + read_len <= n, without a table: the reads that
    start at or in front of p less those that end at or in front of it."""
    p = np.arange(n, dtype=np.int64)
    last = (n - read_len) // step  # the last read's k
    started = np.minimum(p // step, last) + 1
    ended = np.where(p >= read_len, np.minimum((p - read_len) // step, last) + 1, 0)
    return started - ended


def cover_answer(levels=(), n: int = 12000, read_len: int = 150, step: int = 5):
    """The runs in closed form.  Exact: the depth rises by one every `step` rows up to read_len / step, stays, and falls by one
    every `step` rows from n - read_len + step on (the last read starts at a multiple of step: n, read_len are multiples here)."""
    assert n % step == 0 and read_len % step == 0 and n >= 2 * read_len
    top = read_len // step
    if not levels:
        up = [(step * k, k + 1) for k in range(top)]
        down = [(n - read_len + step * k, top - k) for k in range(1, top)]
        return up + down
    out = [(0, sum(1 for t in levels if t <= 1))]
    for t in levels:  # reached at the t-th read's start, lost where only t - 1 reads are left
        if 1 < t <= top:
            out.append((step * (t - 1), sum(1 for u in levels if u <= t)))
    for t in sorted(levels, reverse=True):
        if 1 < t <= top:
            out.append((n - step * (t - 1), sum(1 for u in levels if u <= t - 1)))
    return out


def test_cover_closed_form_is_the_spec_of_its_depth():
    d = cover_depth()
    assert d[0] == 1 and d[149] == 30 and d[150] == 30 and d[6000] == 30 and d[11850] == 30 and d[11855] == 29 and d[11999] == 1
    brute = np.zeros(12000, dtype=np.int64)
    for a in range(0, 12000 - 150 + 1, 5):
        brute[a:a + 150] += 1
    assert np.array_equal(d, brute)
    t = table_of(d)
    assert pairs(ds.runs(t)) == cover_answer() and len(cover_answer()) == 59
    assert pairs(ds.runs(t, (1, 30))) == cover_answer((1, 30)) == [(0, 1), (145, 2), (11855, 1)]
    assert pairs(ds.runs(t, (2, 5, 31))) == cover_answer((2, 5, 31)) == [(0, 0), (5, 1), (20, 2), (11980, 1), (11995, 0)]


def test_cover_sample_answer_holds_on_the_definition():
    """The known answer of test_gpu_depth.py, on the CPU: map_spec.filter_reads over the oracle's MEM list, piled by pile_spec:
    every read of the fixed seed maps where it was taken from, so the table's depth is the closed form."""
    import map_spec
    import pile_spec
    from oracle import pyoracle as po
    ref, q, off = cover_sample(COVER_SEED)
    mem, counts = po.OracleIndex(bytes(ref)).match_batch(q, off, 20, True)
    boff = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    res = map_spec.filter_reads(mem, boff, ref, q, off, True)
    assert all(r[0] == 1 + k % 2 for k, r in enumerate(res))
    table = pile_spec.pile(res, q, off, len(ref))
    assert ds.depth(table) == [int(x) for x in cover_depth()]
    assert pairs(ds.runs(table)) == cover_answer() and pairs(ds.runs(table, (1, 30))) == cover_answer((1, 30))
