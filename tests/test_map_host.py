"""-paf on the CPU: the definition (tests/map_spec.py) held to what a mapping must satisfy -- the quality's
range and its two ends, the primary block's segments equal to -aln's, every PAF line replayed letter by letter on the read as
given and the record -- on random pairs (both strands, several records, N) and on the golden -mem files; a worked example; the
two known-answer constructions of the GPU test on the definition alone; the command line; the front end's writer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aln_spec
import chain_spec
import ext_spec
import hostlib
import map_spec
import test_aln_host as tah
from golden_cases import CASES, MANIFEST
from oracle import pyoracle as po

MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
UNIQUE_SEED = 4150  # (fixed: test_unique_reads_spec_meets_the_cap confirms the cap on the definition alone)


class FakeRef:
    """What map_spec.paf_lines reads of a hostlib.Loaded, for a text built in the test: records joined by one N."""

    class _S:
        pass

    def __init__(self, recs, names):
        self.names, self.sizes = list(names), [len(r) for r in recs]
        self.merged_start = list(np.concatenate([[0], np.cumsum([len(r) + 1 for r in recs])[:-1]]).astype(int))
        self.s = self._S()
        self.s.num = len(recs)
        self.chars = b"N".join(bytes(r) for r in recs)


def _rows(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


def check_read(result, blocks, read: bytes, T: bytes, G, P, X, E):
    """The invariants of one read's result, from chain_spec and aln_spec."""
    strand, mapq, s1, s2, segl = result
    scores = [chain_spec.block_chain(b, G, windowed=len(b) > 200)[1] for b in blocks]
    assert 0 <= mapq <= 60 and 0 <= s2 <= s1 and s1 == max(scores)
    assert (mapq == 60) == (s2 == 0 and s1 > 0) and (s1 == 0 or (mapq == 0) == (60 * (s1 - s2) < s1))
    if s1 == 0:
        assert (strand, mapq, s2, segl) == (0, 0, 0, []) and all(len(b) == 0 for b in blocks)
        return
    assert strand - 1 == scores.index(s1)  # the first block that reaches the maximum
    rec = np.frombuffer(read, dtype=np.uint8)
    Q = bytes(ext_spec.revcomp(rec)) if strand == 2 else read
    assert segl == aln_spec.block_aln(blocks[strand - 1], Q, T, G, P, X, E) and len(segl) > 0
    if len(blocks) == 2:
        assert s2 >= scores[2 - strand]


def replay_paf(data: bytes, names, reads, ref, results):
    """Every PAF line on the read as given (reverse-complemented for '-') and the record's letters: independent of the spec's
    arithmetic.  names: cut read names in order; reads: their letters; results: the read_map tuples (for mapq, s1, s2)."""
    lines = data.split(b"\n")[:-1]
    by_name = {map_spec.cut_name(n): k for k, n in enumerate(names)}
    rec_of = {map_spec.cut_name(n): k for k, n in enumerate(ref.names)}
    seen = {}
    for line in lines:
        f = line.split(b"\t")
        assert len(f) == 16 and not line.startswith(b">")
        k = by_name[f[0]]
        n, qs, qe = int(f[1]), int(f[2]), int(f[3])
        r = rec_of[f[5]]
        rlen, ts, te, eq, alen, mapq = (int(x) for x in f[6:12])
        assert n == len(reads[k]) and rlen == ref.sizes[r] and 0 <= qs < qe <= n and 0 <= ts < te
        assert f[12].startswith(b"NM:i:") and f[13].startswith(b"s1:i:") and f[14].startswith(b"s2:i:") and f[15].startswith(b"cg:Z:")
        assert (mapq, int(f[13][5:]), int(f[14][5:])) == results[k][1:4] and f[4] == (b"+", b"-")[results[k][0] - 1]
        rec = np.frombuffer(reads[k], dtype=np.uint8)
        Q = bytes(ext_spec.revcomp(rec)) if f[4] == b"-" else bytes(rec)
        x = qs if f[4] == b"+" else n - qe  # where the piece starts in the scanned strand
        start = ref.merged_start[r] if ref.s.num > 1 else 0
        R = ref.chars[start:]  # (the record's letters, and what follows it in the merged text: see `rlen` below)
        y, cost, neq, total, num = ts, 0, 0, 0, b""
        passed = False  # an anchor that holds the separator has taken the segment into the next record
        for ch in f[15][5:]:
            if chr(ch).isdigit():
                num += bytes([ch])
                continue
            c, cnt, num = chr(ch), int(num), b""
            assert cnt > 0
            if c in "=X":
                for t in range(cnt):
                    assert ((Q[x + t] & 0xDF) == (R[y + t] & 0xDF)) == (c == "=")
                    # the one way past the record's end (4.15): an anchor that itself holds the separator
                    passed = passed or (y + t == rlen and c == "=" and Q[x + t] in b"Nn")
                    assert y + t < rlen or passed
                x, y = x + cnt, y + cnt
            elif c == "I":
                x += cnt
            else:
                assert c == "D" and (y + cnt <= rlen or passed)
                y += cnt
            cost += cnt if c != "=" else 0
            neq += cnt if c == "=" else 0
            total += cnt
        x0 = qs if f[4] == b"+" else n - qe
        assert (x - x0, y - ts) == (qe - qs, te - ts) and ts < rlen
        assert (cost, neq, total) == (int(f[12][5:]), eq, alen)
        seen[k] = seen.get(k, 0) + 1
    for k, res in enumerate(results):
        assert seen.get(k, 0) == len(res[4])
    return len(lines)


@pytest.mark.parametrize("seed", range(3))
def test_definition_on_random_pairs(seed):
    rng = np.random.default_rng(4150 + seed)
    mapped = unmapped = rev = low = lines = 0
    for _ in range(30):
        alpha = np.frombuffer(b"ACGT"[: int(rng.integers(3, 5))], dtype=np.uint8)
        recs = [rng.choice(alpha, size=int(rng.integers(80, 300))).tobytes() for _ in range(int(rng.integers(1, 4)))]
        ref = FakeRef(recs, [b"rec%d some words" % k for k in range(len(recs))])
        text = ref.chars
        o = po.OracleIndex(text)
        min_len = int(rng.integers(5, 10))
        reads, names = [], []
        for k in range(4):
            if k == 3:
                q = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=12).tobytes() if alpha.size == 3 else b"NNNNNNNNNNNN"
            else:
                a = int(rng.integers(0, len(text) - 60))
                q = tah.mutate(rng, text[a:a + int(rng.integers(60, 250))], alpha)
                if k == 1:
                    q = bytes(ext_spec.revcomp(np.frombuffer(q, dtype=np.uint8)))
            reads.append(q)
            names.append(b"read%d\tcomment" % k)
        for both in (True, False):
            for G, P, X, E in ((5000, 4, 20, 31), (40, 1, 5, 2)):
                results = []
                for q in reads:
                    strands = [q, bytes(ext_spec.revcomp(np.frombuffer(q, dtype=np.uint8)))][: 2 if both else 1]
                    blocks = [_rows(o.get_matches(s, min_len)) for s in strands]
                    res = map_spec.read_map(blocks, q, text, G, P, X, E)
                    check_read(res, blocks, q, text, G, P, X, E)
                    results.append(res)
                    mapped += res[0] != 0
                    unmapped += res[0] == 0
                    rev += res[0] == 2
                    low += res[0] != 0 and res[1] < 60
                data = map_spec.paf_file(results, names, [len(q) for q in reads], ref)
                # (some reads hold an N and match the separator: replay_paf allows the record's end to be passed that way only)
                lines += replay_paf(data, names, reads, ref, results)
    assert mapped > 200 and unmapped > 20 and rev > 40 and low > 40 and lines > 200


@pytest.mark.parametrize("case", MEM_CASES)
def test_definition_on_golden_files(case):
    for G, P, X, E in ((5000, 4, 20, 31), (200, 1, 5, 3)):
        results, rows, ref, qs, opts = map_spec.golden_map(case, G, P, X, E)
        chars, T = qs.chars, ext_spec._letters(ref.chars)
        reads = [chars[qs.offsets[i]:qs.offsets[i + 1]] for i in range(qs.n)]
        for res, bl, q in zip(results, rows, reads):
            check_read(res, bl, q, T, G, P, X, E)
        data = map_spec.paf_file(results, qs.names, qs.sizes, ref)
        assert data == map_spec.golden_paf_file(case, G, P, X, E)
        if len({map_spec.cut_name(n) for n in qs.names}) == qs.n and len({map_spec.cut_name(n) for n in ref.names}) == ref.s.num:
            replay_paf(data, qs.names, reads, ref, results)


def test_worked_example():
    #  the read of aln_spec's worked example, given reverse-complemented, against a text that also holds a shorter exact piece
    #  T: ACGTACGTACAGGATCCATCTTGACA N GGATCCAT
    T = b"ACGTACGTACAGGATCCATCTTGACA" + b"N" + b"GGATCCAT"
    Qr = b"ACGTACGTACTGGATCCATTTGACA"  # the reverse strand of the read as given
    read = bytes(ext_spec.revcomp(np.frombuffer(Qr, dtype=np.uint8)))
    fwd = np.zeros((0, 3), np.int64)
    # reverse block, q descending: the three rows of the example and the second copy of GGATCCAT
    rev = np.array([(20, 19, 6), (11, 11, 8), (27, 11, 8), (0, 0, 10)])
    strand, mapq, s1, s2, segl = map_spec.read_map([fwd, rev], read, T)
    # the chain (0,0,10) -> (11,11,8) -> (20,19,6): 10 + 8 + (6 - 1) = 23; the rows left: (27,11,8) alone, 8
    assert (strand, s1, s2, mapq) == (2, 23, 8, (60 * 15) // 23) and mapq == 39
    assert segl == [(0, 0, 26, 25, 2, [("=", 10), ("X", 1), ("=", 8), ("D", 1), ("=", 6)])]
    ref = FakeRef([T[:26], T[27:]], [b"chrA first", b"chrB"])
    assert map_spec.paf_lines(b"r1 a read", 25, (strand, mapq, s1, s2, segl), ref) == \
        b"r1\t25\t0\t25\t-\tchrA\t26\t0\t26\t24\t26\t39\tNM:i:2\ts1:i:23\ts2:i:8\tcg:Z:10=1X8=1D6=\n"
    # forward rows as good as the reverse ones: the tie goes to the forward block, and the competitor is the other block
    strand, mapq, s1, s2, _ = map_spec.read_map([rev[[0, 1, 3]], rev[[0, 1, 3]]], Qr, T)
    assert (strand, mapq, s1, s2) == (1, 0, 23, 23)
    # a piece of the reverse strand at qs: 4 letters from query_pos 3 of 25 lie at [18, 22) of the read as given
    line = map_spec.paf_lines(b"r", 25, (2, 60, 4, 0, [(5, 3, 4, 4, 0, [("=", 4)])]), ref)
    assert line.split(b"\t")[2:4] == [b"18", b"22"]
    assert map_spec.read_map([fwd, fwd], read, T) == (0, 0, 0, 0, []) and map_spec.paf_lines(b"r", 25, (0, 0, 0, 0, []), ref) == b""
    segs, roff, ops, ooff, recs = map_spec.pack([(0, 0, 0, 0, []), (2, 39, 23, 8, segl)])
    assert list(roff) == [0, 0, 1] and recs.tolist() == [[0, 0, 0, 0], [2, 39, 23, 8]] and list(ooff) == [0, 5]


def test_unique_reads_spec_meets_the_cap():
    """The GPU test's first known answer on the definition alone, with the oracle's rows at -l 20: the chosen seed meets the
    95 % cap, every read maps to its origin on its strand."""
    ref, q, off, truth = map_spec.unique_reads(UNIQUE_SEED)
    T = ref.tobytes()
    o = po.OracleIndex(T)
    top = 0
    for k, (a, strand) in enumerate(truth):
        read = q[int(off[k]):int(off[k + 1])].tobytes()
        blocks = [_rows(o.get_matches(s, 20)) for s in (read, bytes(ext_spec.revcomp(np.frombuffer(read, dtype=np.uint8))))]
        res = map_spec.read_map(blocks, read, T)
        assert res[0] == strand and len(res[4]) >= 1
        for s in res[4]:
            assert a - 200 <= s[0] and s[0] + s[2] <= a + 200 + 200
        top += res[1] == 60
    assert len(truth) == 200 and top >= 0.95 * len(truth)


def test_duplicated_reads_spec_gives_quality_0():
    ref, q, off = map_spec.duplicated_reads(7)
    T = ref.tobytes()
    o = po.OracleIndex(T)
    for k in range(len(off) - 1):
        read = q[int(off[k]):int(off[k + 1])].tobytes()
        blocks = [_rows(o.get_matches(s, 20)) for s in (read, bytes(ext_spec.revcomp(np.frombuffer(read, dtype=np.uint8))))]
        strand, mapq, s1, s2, segl = map_spec.read_map(blocks, read, T)
        assert strand == 1 and s1 == s2 == 150 and mapq == 0 and len(segl) == 1


# ---- the command line ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [["-paf", "ref.fa", "q.fa"], ["ref.fa", "-paf", "q.fa"], ["ref.fa", "q.fa", "-PAF"],
                                  ["-paf", "-maxed", "5", "-mgap", "100", "-pen", "2", "-xdrop", "3", "-b", "ref.fa", "q.fa"]])
def test_paf_sets_match_type_7_anywhere(args):
    o = hostlib.parse_options(["slaMEM"] + args)
    assert o["match_type"] == 7 and o["num_files"] == 2 and o["files"] == ["ref.fa", "q.fa"]


@pytest.mark.parametrize("other", ["-mam", "-mum", "-smem", "-chain", "-ext", "-aln"])
def test_paf_with_another_mode_is_match_type_minus_1(other):
    assert hostlib.parse_options(["slaMEM", "-paf", other, "ref.fa", "q.fa"])["match_type"] == -1
    assert hostlib.parse_options(["slaMEM", other, "ref.fa", "-paf", "q.fa"])["match_type"] == -1


def test_other_options_unchanged():
    for tail, mt in (([], 0), (["-mam"], 1), (["-mum"], 2), (["-smem"], 3), (["-chain"], 4), (["-ext"], 5), (["-aln"], 6),
                     (["-pen", "3", "-ext"], 5)):
        assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa"] + tail)["match_type"] == mt


@pytest.mark.parametrize("args,message", [
    (["-paf", "-aln"], b"> ERROR: Option -paf excludes -mam, -mum, -smem, -chain, -ext and -aln"),
    (["-chain", "-paf"], b"> ERROR: Option -paf excludes -mam, -mum, -smem, -chain, -ext and -aln"),
    (["-paf", "-maxed", "200"], b"> ERROR: Option -maxed needs a whole number from 0 to 127"),
    (["-paf", "-mgap", "0"], b"> ERROR: Option -mgap needs a whole number of at least 1"),
    (["-paf", "-pen", "0"], b"> ERROR: Option -pen needs a whole number of at least 1, option -xdrop one of at least 0"),
    (["-paf", "-occ", "3"], None)])
def test_refused_combinations_exit_255_before_any_work(args, message, tmp_path):
    exe = os.path.join(hostlib.HOST_DIR, "slaMEM-hip")
    out = tmp_path / "out.paf"
    r = subprocess.run([exe] + args + ["-o", str(out), "ref.fa", "q.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and not out.exists()
    assert b"> ERROR: " in r.stdout and (message is None or message in r.stdout)


# ---- the writer ----------------------------------------------------------------------------------------------------------------

def _c_paf(L, name, n, res, ref_recs, merged_start, num):
    strand, mapq, s1, s2, segl = res
    segs, _, ops, ooff = aln_spec.pack([segl])
    segs32 = np.ascontiguousarray(segs, dtype=np.uint32)
    oo = np.ascontiguousarray(ooff, dtype=np.uint64)
    buf, s = hostlib.Buffer(), C.c_uint64()
    assert L.slh_format_read_paf(C.byref(buf), name, n, strand, mapq, s1, s2, segs32.ctypes.data if len(segl) else None,
                                 ops.ctypes.data if len(ops) else None, oo.ctypes.data, len(segl), ref_recs, merged_start, num,
                                 C.byref(s)) == 0
    out = C.string_at(buf.data, buf.len) if buf.len else b""
    L.slh_buffer_free(C.byref(buf))
    assert s.value == sum(x[3] for x in segl)
    return out


def _paf_lib():
    L = hostlib.lib()
    L.slh_format_read_paf.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(hostlib.Record),
                                      C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]
    return L


@pytest.mark.parametrize("case", MEM_CASES)
def test_front_end_writer_equals_the_spec_writer(case):
    """slh_format_read_paf on the spec's results gives map_spec.paf_lines' bytes (what the GPU test compares the executable's
    file with)."""
    L = _paf_lib()
    results, _, ref, qs, _ = map_spec.golden_map(case)
    got = [_c_paf(L, qs.names[i], qs.sizes[i], res, ref.s.recs, ref.s.merged_start, ref.s.num) for i, res in enumerate(results)]
    assert b"".join(got) == map_spec.golden_paf_file(case)
    assert b"".join(got).count(b"\n") == sum(len(r[4]) for r in results)


def test_front_end_writer_cuts_names_and_turns_the_reverse_strand():
    L = _paf_lib()
    recs = (hostlib.Record * 2)(hostlib.Record(b"chrA first", 26), hostlib.Record(b"chrB\tx", 8))
    starts = (C.c_uint32 * 2)(0, 27)
    fake = FakeRef([b"A" * 26, b"C" * 8], [b"chrA first", b"chrB\tx"])
    for res in ((2, 39, 23, 8, [(0, 0, 26, 25, 2, [("=", 10), ("X", 1), ("=", 8), ("D", 1), ("=", 6)])]),
                (1, 60, 8, 0, [(29, 14, 5, 5, 0, [("=", 5)]), (27, 3, 4, 5, 1, [("=", 2), ("I", 1), ("=", 2)])]),
                (2, 0, 4, 4, [(5, 3, 4, 4, 0, [("=", 4)])]), (0, 0, 0, 0, [])):
        assert _c_paf(L, b"r1 a read", 25, res, recs, starts, 2) == map_spec.paf_lines(b"r1 a read", 25, res, fake)
    assert _c_paf(L, b"r1", 25, (2, 0, 4, 4, [(5, 3, 4, 4, 0, [("=", 4)])]), recs, starts, 2).split(b"\t")[2:9] == \
        [b"18", b"22", b"-", b"chrA", b"26", b"5", b"9"]
