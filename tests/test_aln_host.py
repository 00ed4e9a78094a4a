"""-aln on the CPU: the definition (tests/aln_spec.py) held to what an alignment must satisfy -- every CIGAR
replays over the two sequences, counts and lengths agree, segments of a block do not overlap, every closed gap costs its edit
distance by a second routine, every broken gap is over the limit or holds a letter that is not A,C,G,T -- the wavefront
traceback the kernel uses against the matrix traceback on every gap, and a constructed known answer; on random pairs with
substitutions and indels (both strands, N in read and text, several records), on the golden -mem files, and on the designed gaps
of tests/aln_gap_cases.py at edit limits from 31 to 127."""
import functools

import numpy as np
import pytest

import aln_gap_cases
import aln_spec
import ext_spec
import mum_spec
from golden_cases import CASES, MANIFEST
from oracle import pyoracle as po

MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]


@functools.lru_cache(maxsize=4096)  # (the designed gaps come back at every edit limit)
def levenshtein(a: bytes, b: bytes) -> int:
    """Two rows, letter by letter, case folded: independent of aln_spec.edit_matrix."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + ((a[i - 1] & 0xDF) != (b[j - 1] & 0xDF)))
        prev = cur
    return prev[len(b)]


def replay(seg, Q: bytes, T: bytes):
    """A segment's CIGAR over the two sequences: every letter under = is equal, under X unequal; lengths and edits agree."""
    p, q, rlen, qlen, edits, rl = seg
    x, y, cost = q, p, 0
    assert all(n > 0 for _, n in rl) and all(rl[i][0] != rl[i + 1][0] for i in range(len(rl) - 1))
    for op, n in rl:
        if op in "=X":
            for t in range(n):
                assert ((Q[x + t] & 0xDF) == (T[y + t] & 0xDF)) == (op == "=")
            x, y = x + n, y + n
        elif op == "I":
            x += n
        else:
            assert op == "D"
            y += n
        cost += n if op != "=" else 0
    assert (x - q, y - p, cost) == (qlen, rlen, edits)
    assert 0 <= q and x <= len(Q) and 0 <= p and y <= len(T)


def check_blocks(blocks, seqs, gaps, E):
    n_closed = n_broken = 0
    for segl, (Q, T) in zip(blocks, seqs):
        for s in segl:
            replay(s, Q, T)
        for hi, lo in zip(segl, segl[1:]):  # q descending; no overlap in the query
            assert lo[1] + lo[3] <= hi[1]
    for A, B, g in gaps:
        w = aln_spec.wavefront_ops(A, B, E)
        assert (w is None) == (g is None)
        if g is None:
            n_broken += 1
            assert not aln_spec.all_acgt(A) or not aln_spec.all_acgt(B) or levenshtein(A, B) > E
        else:
            n_closed += 1
            ops, d = g
            assert d == levenshtein(A, B) <= E and d == sum(c != "=" for c in ops)
            assert ops.count("=") + ops.count("X") + ops.count("I") == len(A)
            assert ops.count("=") + ops.count("X") + ops.count("D") == len(B)
            assert not (len(A) and len(B)) or ops[0] != "="  # (an anchor is right-maximal)
            assert w == (ops, d)  # the furthest-reaching points alone give the same traceback
    return n_closed, n_broken


def mutate(rng, piece: bytes, alpha) -> bytes:
    out = bytearray()
    for ch in piece:
        r = rng.integers(0, 40)
        if r == 0:
            out.append(int(rng.choice(alpha)))          # substitution (or the same letter)
        elif r == 1:
            out += bytes([ch, int(rng.choice(alpha))])  # insertion
        elif r == 2:
            continue                                    # deletion
        elif r == 3 and rng.integers(0, 4) == 0:
            out.append(ord("N"))
        else:
            out.append(ch)
    return bytes(out)


def _rows(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


@pytest.mark.parametrize("seed", range(4))
def test_definition_on_random_pairs(seed):
    rng = np.random.default_rng(9100 + seed)
    closed = broken = multi = 0
    for _ in range(40):
        alpha = np.frombuffer(b"ACGT"[: int(rng.integers(3, 5))], dtype=np.uint8)
        recs = [rng.choice(alpha, size=int(rng.integers(80, 300))) for _ in range(int(rng.integers(1, 4)))]
        text = bytearray(b"N".join(r.tobytes() for r in recs))
        if rng.integers(0, 2):
            text[int(rng.integers(0, len(text)))] = ord("N")
        text = bytes(text)
        a = int(rng.integers(0, len(text) - 60))
        q = mutate(rng, text[a:a + int(rng.integers(60, 250))], alpha)
        o = po.OracleIndex(text)
        min_len = int(rng.integers(4, 10))
        for strand in (q, bytes(ext_spec.revcomp(np.frombuffer(q, dtype=np.uint8)))):
            rows = _rows(o.get_matches(strand, min_len))
            for G, P, X, E in ((5000, 4, 20, 31), (40, 1, 5, 2), (5000, 4, 20, 0)):
                gaps = []
                segl = aln_spec.block_aln(rows, strand, text, G, P, X, E, gaps)
                c, b = check_blocks([segl], [(strand, text)], gaps, E)
                closed, broken, multi = closed + c, broken + b, multi + (len(segl) > 1)
                assert (len(segl) == 0) == (len(rows) == 0)
    assert closed > 200 and broken > 100 and multi > 50


@pytest.mark.parametrize("case", MEM_CASES)
def test_definition_on_golden_files(case):
    for G, P, X, E in ((5000, 4, 20, 31), (200, 1, 5, 3)):
        gaps = []
        blocks, seqs, _, _, _ = aln_spec.golden_aln(case, G, P, X, E, gaps)
        big = [(A, B, g) for A, B, g in gaps if len(A) * len(B) > 250_000]  # (the letter-wise second routine is quadratic)
        check_blocks(blocks, seqs, [t for t in gaps if len(t[0]) * len(t[1]) <= 250_000], E)
        for A, B, g in big:
            assert aln_spec.wavefront_ops(A, B, E) == g


def test_wavefront_traceback_on_short_random_gaps():
    """Every kind of gap the chain does not produce as well: equal first letters, empty pieces, |a - b| at the limit."""
    rng = np.random.default_rng(77)
    alpha = np.frombuffer(b"AC", dtype=np.uint8)
    closed = 0
    for _ in range(3000):
        A = rng.choice(alpha, size=int(rng.integers(0, 9))).tobytes()
        B = rng.choice(alpha, size=int(rng.integers(0, 9))).tobytes()
        for E in (0, 1, 3, 8):
            D = aln_spec.edit_matrix(A, B)
            assert D[len(A)][len(B)] == levenshtein(A, B)
            want = (aln_spec.traceback(A, B, D), int(D[len(A)][len(B)])) if D[len(A)][len(B)] <= E else None
            assert aln_spec.gap_ops(A, B, E) == want
            assert aln_spec.wavefront_ops(A, B, E) == want
            closed += want is not None
    assert closed > 3000


# ---- designed gaps above 31 edits --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def designed_mems():
    ref, q, off, _ = aln_gap_cases.catalogue()
    mem, counts = po.OracleIndex(ref.tobytes()).match_batch(q, off, aln_gap_cases.MIN_LEN, True)
    return ref, q, off, mem, np.concatenate([[0], np.cumsum(counts.astype(np.int64))])


@pytest.mark.parametrize("E", aln_gap_cases.EDITS)
def test_designed_gaps_above_31_edits(E):
    """The catalogue with the oracle's -mem rows: every CIGAR replays, every gap's distance by the letter-wise routine, the
    wavefront traceback equal to the matrix traceback on every gap -- and the gaps are the ones the catalogue is there for."""
    ref, q, off, mem, boff = designed_mems()
    gaps = []
    blocks = aln_spec.filter_blocks(mem, boff, ref, q, off, True, E=E, gaps_out=gaps)
    T = ref.tobytes()
    seqs = []
    for b in range(len(blocks)):
        rec = q[int(off[b // 2]):int(off[b // 2 + 1])]
        seqs.append((bytes(ext_spec.revcomp(rec)) if b % 2 else rec.tobytes(), T))
    closed, broken = check_blocks(blocks, seqs, gaps, E)
    assert closed + broken == len(gaps) >= len(off) - 1 and sum(len(s) > 0 for s in blocks) == len(off) - 1
    aln_gap_cases.assert_coverage(gaps, E)


def test_bulk_batch_lists_more_gaps_than_workgroups():
    ref, q, off, labels = aln_gap_cases.bulk()
    mem, counts = po.OracleIndex(ref.tobytes()).match_batch(q, off, aln_gap_cases.MIN_LEN, True)
    gaps = []
    aln_spec.filter_blocks(mem, np.concatenate([[0], np.cumsum(counts.astype(np.int64))]), ref, q, off, True, E=127, gaps_out=gaps)
    assert len(labels) >= 1100 + 40 and aln_gap_cases.listed_and_closed(gaps) > 1100
    for A, B, g in gaps[::7]:
        assert aln_spec.wavefront_ops(A, B, 127) == g


def test_wavefront_traceback_on_designed_pieces():
    """The pieces as designed, before any anchor trims them (so with equal first letters, and with an empty side): the wavefront
    form against the traceback of the full matrix at every edit limit up to 127, and the banded matrix against the full one."""
    closed = {E: 0 for E in aln_gap_cases.EDITS}
    for label, A, B in aln_gap_cases.pieces():
        if not aln_spec.all_acgt(A) or not aln_spec.all_acgt(B):
            assert aln_spec.gap_ops(A, B, 127) is None and aln_spec.wavefront_ops(A, B, 127) is None
            continue
        D = aln_spec.edit_matrix(A, B)
        d = int(D[len(A)][len(B)])
        full = (aln_spec.traceback(A, B, D), d)
        for E in aln_gap_cases.EDITS:
            want = full if d <= E else None
            assert aln_spec.gap_ops(A, B, E) == want, (label, E)
            assert aln_spec.wavefront_ops(A, B, E) == want, (label, E)
            closed[E] += want is not None
    assert closed[31] > 10 and closed[127] > 100 and closed[127] > closed[96] > closed[65] > closed[31]


def test_worked_example():
    #    Q: ACGTACGTAC T GGATCCAT  -  TTGACA     one substitution, then one text letter without a query letter
    T = b"ACGTACGTACAGGATCCATCTTGACA"
    Q = b"ACGTACGTACTGGATCCATTTGACA"
    rows = np.array([(20, 19, 6), (11, 11, 8), (0, 0, 10)])  # q descending
    segl = aln_spec.block_aln(rows, Q, T, 5000, 4, 20, 31)
    assert segl == [(0, 0, 26, 25, 2, [("=", 10), ("X", 1), ("=", 8), ("D", 1), ("=", 6)])]
    assert aln_spec.cigar_string(segl[0][5]) == "10=1X8=1D6="
    segl = aln_spec.block_aln(rows, Q, T, 5000, 4, 20, 0)  # no edit allowed: three segments, outer ends only
    assert [s[:5] for s in segl] == [(20, 19, 6, 6, 0), (11, 11, 8, 8, 0), (0, 0, 10, 10, 0)]
    ops = aln_spec.pack([segl])
    assert list(ops[2]) == [(6 << 4) | 7, (8 << 4) | 7, (10 << 4) | 7] and list(ops[3]) == [0, 1, 2, 3] and list(ops[1]) == [0, 3]


def test_constructed_reads_known_answer_holds_for_the_spec():
    """The GPU test's construction on the definition, with the oracle's -mem rows at -l 20: the CIGAR written down from the
    construction for every read."""
    ref, q, off, truth = aln_spec.constructed_reads(11)
    T = ref.tobytes()
    o = po.OracleIndex(T)
    kinds = set()
    for k, (b, seg, rl) in enumerate(truth):
        rec = q[int(off[k]):int(off[k + 1])]
        Q = bytes(ext_spec.revcomp(rec)) if b % 2 else rec.tobytes()
        rows = _rows(o.get_matches(Q, 20))
        segl = aln_spec.block_aln(rows, Q, T)
        assert segl == [seg + (rl,)], (k, segl, seg, rl)
        kinds.add(tuple(c for c, _ in rl if c != "="))
    assert len(truth) == 240 and {("I",), ("D",), ("X",)} <= kinds


# ---- the command line ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [["-aln", "ref.fa", "q.fa"], ["ref.fa", "-aln", "q.fa"], ["ref.fa", "q.fa", "-ALN"],
                                  ["-aln", "-maxed", "5", "-mgap", "100", "-pen", "2", "-xdrop", "3", "ref.fa", "q.fa"]])
def test_aln_sets_match_type_6_anywhere(args):
    import hostlib
    o = hostlib.parse_options(["slaMEM"] + args)
    assert o["match_type"] == 6 and o["num_files"] == 2


@pytest.mark.parametrize("args", [["-aln", "-mam"], ["-aln", "-mum"], ["-smem", "-aln"], ["-chain", "-aln"], ["-aln", "-ext"]])
def test_aln_with_another_mode_is_match_type_minus_1(args):
    import hostlib
    assert hostlib.parse_options(["slaMEM"] + args + ["ref.fa", "q.fa"])["match_type"] == -1


def test_maxed_is_not_mam_and_other_options_unchanged():
    import ctypes as C
    import hostlib
    assert hostlib.parse_options(["slaMEM", "-maxed", "5", "ref.fa", "q.fa"])["match_type"] == 0
    for tail, mt in (([], 0), (["-mam"], 1), (["-mum"], 2), (["-smem"], 3), (["-chain"], 4), (["-ext"], 5)):
        assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa"] + tail)["match_type"] == mt
    L = hostlib.lib()
    L.slh_parse_max_edits.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int)]

    def parse(args):
        argv = (C.c_char_p * (len(args) + 1))(b"slaMEM", *[a.encode() for a in args])
        out = C.c_int()
        return L.slh_parse_max_edits(len(args) + 1, argv, C.byref(out)), out.value
    assert parse(["-aln", "a", "b"]) == (0, -1)
    assert parse(["-aln", "-maxed", "0", "a", "b"]) == (1, 0) and parse(["-MAXED", "127", "a"]) == (1, 127)
    for bad in (["-maxed"], ["-maxed", "128"], ["-maxed", "-1"], ["-maxed", "3x"], ["-maxed", "few"]):
        assert parse(bad)[0] == -1


@pytest.mark.parametrize("args,message", [(["-maxed", "3"], b"> ERROR: Option -maxed needs -aln"),
                                          (["-aln", "-chain"], b"> ERROR: Option -aln excludes -mam, -mum, -smem, -chain and -ext"),
                                          (["-aln", "-maxed", "200"], b"> ERROR: Option -maxed needs a whole number from 0 to 127")])
def test_refused_combinations_exit_255_before_any_work(args, message, tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slamem_amd", "host", "slaMEM-hip")
    out = tmp_path / "out.txt"
    r = subprocess.run([exe] + args + ["-o", str(out), "ref.fa", "q.fa"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and message in r.stdout and not out.exists()


@pytest.mark.parametrize("case", MEM_CASES)
def test_front_end_writer_equals_the_spec_writer(case):
    """slh_format_block_aln on the spec's segments gives aln_spec.format_block's bytes (what the GPU test compares the
    executable's file with)."""
    import ctypes as C
    import hostlib
    L = hostlib.lib()
    L.slh_format_block_aln.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.POINTER(hostlib.Record), C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]
    blocks, _, ref, qs, opts = aln_spec.golden_aln(case)
    strands = 2 if "-b" in opts else 1
    segs, boff, ops, ooff = aln_spec.pack(blocks)
    segs32 = np.ascontiguousarray(segs, dtype=np.uint32)
    oo = np.ascontiguousarray(ooff, dtype=np.uint64)
    got, lines = [], 0
    for b, segl in enumerate(blocks):
        buf, s = hostlib.Buffer(), C.c_uint64()
        at = int(boff[b])
        assert L.slh_format_block_aln(C.byref(buf), qs.names[b // strands], b % strands, segs32[at:].ctypes.data if len(segl) else None,
                                      ops.ctypes.data, oo[at:].ctypes.data, len(segl), ref.s.recs, ref.s.merged_start, ref.s.num,
                                      C.byref(s)) == 0
        got.append(C.string_at(buf.data, buf.len))
        L.slh_buffer_free(C.byref(buf))
        assert s.value == sum(x[3] for x in segl)
        lines += len(segl)
    assert b"".join(got) == aln_spec.golden_aln_file(case)
    assert b"".join(got).count(b"\n") == lines + len(blocks)
