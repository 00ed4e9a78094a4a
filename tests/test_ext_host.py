"""-ext without a GPU: the option and its parameters as the front end parses them, the refused combinations, the four-column
writer, and the definition the GPU tests check against (tests/ext_spec.py) -- the per-letter rule against an exhaustive check
of every reachable prefix, against a second implementation that walks the set bits of a mismatch mask (the equivalence the
kernel relies on), and the one-row-per-segment rule -- on random text/query pairs of both strands with N and several reference
records, on the golden -mem files the real reference wrote, and on the planted reads of the GPU test's known answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ext_spec
import hostlib
import mum_spec
from golden_cases import CASES, MANIFEST, case_paths
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
ACGT = frozenset(b"ACGT")


# ---- options ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [
    ["-ext", "ref.fa", "q.fa"],
    ["-b", "-ext", "-l", "20", "ref.fa", "q.fa"],
    ["-l", "20", "ref.fa", "q.fa", "-ext"],
    ["ref.fa", "-ext", "q.fa"],
    ["-EXT", "ref.fa", "q.fa"],
    ["-ext", "-pen", "3", "ref.fa", "-xdrop", "0", "q.fa"],
], ids=["first", "middle", "last", "between-files", "upper-case", "with-values"])
def test_ext_sets_match_type_5_anywhere(args):
    o = hostlib.parse_options(["slaMEM"] + args)
    assert o["match_type"] == 5
    assert o["files"] == ["ref.fa", "q.fa"]  # never taken as a file; the values of -pen and -xdrop neither


@pytest.mark.parametrize("args", [
    ["-ext", "-mam", "x", "ref.fa", "q.fa"],
    ["-mum", "x", "-ext", "ref.fa", "q.fa"],
    ["-ext", "ref.fa", "q.fa", "-smem"],
    ["-chain", "-ext", "ref.fa", "q.fa"],
])
def test_ext_with_another_mode_is_match_type_minus_1(args):
    assert hostlib.parse_options(["slaMEM"] + args)["match_type"] == -1


def test_other_options_unchanged():
    for tail, mt in (([], 0), (["-mam"], 1), (["-mum"], 2), (["-smem"], 3), (["-chain"], 4)):
        assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa"] + tail)["match_type"] == mt
    o = hostlib.parse_options(["slaMEM", "-ext", "-pen", "2", "-m", "50", "-b", "-o", "out.txt", "ref.fa", "q.fa"])
    assert (o["match_type"], o["min_seq_len"], o["both_strands"], o["files"], o["out_arg"]) == (5, 50, 1, ["ref.fa", "q.fa"], 8)


def parse_ext_params(args):
    L = hostlib.lib()
    L.slh_parse_ext_params.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    argv = (C.c_char_p * (len(args) + 2))(b"slaMEM", *[a.encode() for a in args], None)
    pen, xd = C.c_int(-7), C.c_int(-7)
    rc = L.slh_parse_ext_params(len(args) + 1, argv, C.byref(pen), C.byref(xd))
    return rc, pen.value, xd.value


@pytest.mark.parametrize("args,expect", [
    (["-ext", "ref.fa", "q.fa"], (0, 0, -1)),
    (["-ext", "-pen", "1", "ref.fa", "q.fa"], (1, 1, -1)),
    (["-ext", "ref.fa", "q.fa", "-xdrop", "0"], (1, 0, 0)),
    (["-XDROP", "2147483647", "-PEN", "7", "-ext", "ref.fa", "q.fa"], (1, 7, 2147483647)),
])
def test_pen_and_xdrop_values(args, expect):
    assert parse_ext_params(args) == expect


@pytest.mark.parametrize("args", [
    ["-ext", "-pen", "0"], ["-ext", "-pen", "-2"], ["-ext", "-pen", "four"], ["-ext", "-pen", "4x"], ["-ext", "-pen", "2147483648"],
    ["-ext", "-xdrop", "-1"], ["-ext", "-xdrop", "wide"], ["-ext", "ref.fa", "q.fa", "-xdrop"], ["-ext", "ref.fa", "-pen"],
])
def test_pen_and_xdrop_errors(args):
    assert parse_ext_params(args)[0] == -1


@pytest.mark.parametrize("args,message", [
    (["-ext", "-chain"], b"> ERROR: Option -ext excludes -mam, -mum, -smem and -chain"),
    (["-ext", "-mam", "x"], b"> ERROR: Option -ext excludes -mam, -mum, -smem and -chain"),
    (["-smem", "-ext"], b"> ERROR: Option -ext excludes -mam, -mum, -smem and -chain"),
    (["-pen", "3"], b"> ERROR: Options -pen and -xdrop need -ext"),
    (["-chain", "-xdrop", "3"], b"> ERROR: Options -pen and -xdrop need -ext"),
    (["-ext", "-pen", "0"], b"> ERROR: Option -pen needs a whole number of at least 1"),
    (["-ext", "-pen", "four"], b"> ERROR: Option -pen needs a whole number of at least 1"),
    (["-ext", "-xdrop", "-1"], b"option -xdrop one of at least 0"),
])
def test_refused_combinations_exit_255_before_any_work(args, message, tmp_path):
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + args + ["-o", str(out), ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60)
    assert r.returncode == 255
    assert message in r.stdout
    assert not out.exists()


def test_usage_lists_ext_pen_and_xdrop():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"\t-ext\t" in r.stdout and b"\t-pen\t" in r.stdout and b"\t-xdrop\t" in r.stdout


# ---- the writer -------------------------------------------------------------------------------------------------------------

def c_format_block_ext(name, reverse, rows, mms, ref):
    L = hostlib.lib()
    L.slh_format_block_ext.argtypes = [C.POINTER(hostlib.Buffer), C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.POINTER(hostlib.Record), C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]
    m = np.ascontiguousarray(rows, dtype=np.uint32)
    x = np.ascontiguousarray(mms, dtype=np.uint32)
    b, s = hostlib.Buffer(), C.c_uint64()
    assert L.slh_format_block_ext(C.byref(b), name, reverse, m.ctypes.data, x.ctypes.data, m.shape[0], ref.s.recs,
                                  ref.s.merged_start, ref.s.num, C.byref(s)) == 0
    out = C.string_at(b.data, b.len)
    L.slh_buffer_free(C.byref(b))
    return out, s.value


def _check_writer(case):
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    data = open(exp_mems, "rb").read()
    blocks = mum_spec.parse_mems_file(data, ref)
    strands = 2 if "-b" in opts else 1
    plain, four_py, four_c = [], [], []
    for b, (_, rows) in enumerate(blocks):
        name, s = qs.names[b // strands], b % strands
        mms = (np.arange(len(rows)) * 7 + b) % 1000
        plain.append(ext_spec.format_block(name, s, rows, None, ref))
        four_py.append(ext_spec.format_block(name, s, rows, mms, ref))
        got, total = c_format_block_ext(name, s, rows, mms, ref)
        four_c.append(got)
        assert total == int(np.asarray(rows, dtype=np.int64).reshape(-1, 3)[:, 2].sum())
    assert b"".join(plain) == data  # the Python writer reproduces the reference's file ...
    assert b"".join(four_c) == b"".join(four_py)  # ... and the front end's writer agrees with it on the fourth column
    lines = [ln for ln in b"".join(four_c).split(b"\n") if ln and not ln.startswith(b">")]
    assert all(len(ln.split(b"\t")) == (5 if ref.s.num > 1 else 4) for ln in lines)
    return ref.s.num > 1


def test_four_column_writer_on_every_golden_case():
    multi = 0
    for case in MEM_CASES:
        multi += _check_writer(case)
    assert multi >= 1  # (lines that name their reference record are covered)


# ---- the definition ---------------------------------------------------------------------------------------------------------

def test_worked_example():
    """One side to the right of a seed that ends in front of Q[0] / T[8]:

        Q  A C G T A C G T A C G T
        T  A C G A A C G T A C C T N        (mismatches at t = 3 and t = 10)

    P = 4: s = 1 2 3 -1 0 1 2 3 4 5 1 2, then Q ends: best 5 at ext 10, the prefix in front of the second mismatch, one mismatch
    inside.  X = 20 and X = 5 give the same (the drop is 4); X = 3 and X = 0 end at the first mismatch: best 3, ext 3.
    P = 1: s = 1 2 3 2 3 4 5 6 7 8 7 8: the last letter brings s back to 8, equal to the best, not more: ext stays 10."""
    Q = b"ACGTACGTACGT"
    T = b"GGGGGGGG" + b"ACGAACGTACCT" + b"NACGT"
    assert ext_spec.extend_side(Q, T, 0, 8, 1, 4, 20) == (10, 5, 1)
    assert ext_spec.extend_side(Q, T, 0, 8, 1, 4, 5) == (10, 5, 1)
    assert ext_spec.extend_side(Q, T, 0, 8, 1, 4, 3) == (3, 3, 0)
    assert ext_spec.extend_side(Q, T, 0, 8, 1, 4, 0) == (3, 3, 0)
    assert ext_spec.extend_side(Q, T, 0, 8, 1, 1, 20) == (10, 8, 1)
    # the mirror image gives the mirrored answer
    assert ext_spec.extend_side(Q[::-1], T[::-1], len(Q) - 1, len(T) - 9, -1, 4, 20) == (10, 5, 1)
    # a row: the seed Q[4:8] = T[12:16].  P = 4: to the right A C match, then G/C costs more than the T behind it gives back:
    # extR = 2; to the left the first letter is the mismatch T/A and the three letters behind it cannot pay for it: extL = 0
    assert ext_spec.extend_row(Q, T, (12, 4, 4), 4, 20) == ((12, 4, 6), 0)
    # P = 1: to the left s = -1 0 1 2: extL = 4 with one mismatch; to the right 1 2 1 2: extR = 2
    assert ext_spec.extend_row(Q, T, (12, 4, 4), 1, 20) == ((8, 0, 10), 1)
    # the seed Q[0:3] = T[8:11] of the same diagonal grows into the same segment (s = -1 0 1 2 3 4 5 4 5: extR = 7) and is
    # dropped; the row on another diagonal between them stays as it is
    rows = np.array([(12, 4, 4), (0, 2, 1), (8, 0, 3)])
    k, m, keep = ext_spec.block_ext(rows, Q, T, 1, 20)
    assert list(keep) == [True, True, False]
    assert [tuple(int(v) for v in r) for r in k] == [(8, 0, 10), (0, 2, 1)] and list(m) == [1, 0]
    # with P = 4 the second seed still crosses the mismatch behind it (s = -4 -3 -2 -1 0 1 2 -2 -1: extR = 7) but the first does
    # not reach back over it: two segments of one diagonal that overlap but differ, both reported
    k, m, keep = ext_spec.block_ext(rows, Q, T, 4, 20)
    assert [tuple(int(v) for v in r) for r in k] == [(12, 4, 6), (0, 2, 1), (8, 0, 10)] and list(m) == [0, 0, 1]


def side_letters(Q, T, qi, ti, step):
    """The pairs of letters a side may look at, in order, up to the first step that the stop rule forbids."""
    out = []
    a, b = qi, ti
    while 0 <= a < len(Q) and 0 <= b < len(T) and (Q[a] & 0xDF) in ACGT and (T[b] & 0xDF) in ACGT:
        out.append((Q[a] & 0xDF) == (T[b] & 0xDF))
        a += step
        b += step
    return np.array(out, dtype=bool)


def exhaustive_side(eq: np.ndarray, P: int, X: int):
    """(ext, best) by looking at every prefix: score(e) over the first e letters, e reachable when no shorter prefix had
    fallen more than X below the best before it; the best score, its shortest prefix."""
    score = np.concatenate([[0], np.cumsum(np.where(eq, 1, -P))])
    drop = np.maximum.accumulate(score) - score
    over = np.nonzero(drop > X)[0]
    last = int(over[0]) if len(over) else len(eq)  # the step that ends the side is taken, nothing behind it
    reach = score[:last + 1]
    best = int(reach.max())
    return int(np.argmax(reach)), best


def mask_walk_side(eq: np.ndarray, P: int, X: int):
    """The same by walking the set bits of the mismatch mask (a Python integer): per mismatch the run of matches in front of
    it is added, the maximum taken, P subtracted, the drop tested; the run behind the last mismatch is added at the end."""
    n = len(eq)
    mask = 0
    for t in np.nonzero(~eq)[0]:
        mask |= 1 << int(t)
    s = best = ext = pos = mm = mm_best = 0
    while mask:
        at = (mask & -mask).bit_length() - 1
        mask &= mask - 1
        s += at - pos
        if s > best:
            best, ext, mm_best = s, at, mm
        s -= P
        mm += 1
        pos = at + 1
        if best - s > X:
            return ext, best, mm_best
    s += n - pos
    if s > best:
        best, ext, mm_best = s, n, mm
    return ext, best, mm_best


def check_row(Q, T, row, P, X):
    """Everything the definition promises about one row; returns (extended by, mismatches)."""
    p, q, ln = (int(v) for v in row)
    ext = {}
    for name, qi, ti, step in (("right", q + ln, p + ln, 1), ("left", q - 1, p - 1, -1)):
        got = ext_spec.extend_side(Q, T, qi, ti, step, P, X)
        for chunk in (5, 4096):  # the chunked numpy form the large GPU cases use
            assert ext_spec.extend_side_np(np.frombuffer(Q, dtype=np.uint8), np.frombuffer(T, dtype=np.uint8), qi, ti, step, P, X,
                                           chunk) == got, (name, row, P, X, chunk)
        eq = side_letters(Q, T, qi, ti, step)
        e, best = exhaustive_side(eq, P, X)
        assert got[:2] == (e, best), (name, row, P, X)
        assert got[2] == int((~eq[:e]).sum())
        assert mask_walk_side(eq, P, X) == got, (name, row, P, X)
        assert e == 0 or eq[e - 1]  # a side ends on a match
        # no prefix scores more, no shorter one the same (stated once more, on the reachable prefixes themselves)
        ext[name] = got
    (p2, q2, l2), mm = ext_spec.extend_row(Q, T, row, P, X)
    assert (p2, q2, l2) == (p - ext["left"][0], q - ext["left"][0], ext["left"][0] + ln + ext["right"][0])
    assert p2 <= p and q2 <= q and p2 + l2 >= p + ln and q2 >= 0 and p2 >= 0 and q2 + l2 <= len(Q) and p2 + l2 <= len(T)
    a = np.frombuffer(Q[q2:q2 + l2], dtype=np.uint8) & 0xDF
    b = np.frombuffer(T[p2:p2 + l2], dtype=np.uint8) & 0xDF
    # the Hamming count of the two slices (outside the seed every letter is one of A,C,G,T; inside it N = N stays a match)
    assert mm == int((a != b).sum())
    assert not (a != b)[q - q2:q - q2 + ln].any()
    assert l2 - (P + 1) * mm >= ln
    assert l2 - (P + 1) * mm == ln + ext["left"][1] + ext["right"][1]
    return l2 - ln, mm


def _rows(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


def check_block(rows, Q, T, P, X):
    """Kept rows are pairwise different and every dropped row has an earlier twin."""
    k, m, keep = ext_spec.block_ext(rows, Q, T, P, X)
    segs = [ext_spec.extend_row(Q, T, r, P, X)[0] for r in rows]
    kept = [s for s, f in zip(segs, keep) if f]
    assert len(set(kept)) == len(kept) == len(k) and [tuple(int(v) for v in r) for r in k] == kept
    for i, f in enumerate(keep):
        assert f == (segs[i] not in segs[:i])
    return int((~keep).sum())


@pytest.mark.parametrize("seed", range(4))
def test_definition_on_random_pairs(seed):
    rng = np.random.default_rng(8100 + seed)
    grown = mms = dropped = pairs = 0
    for _ in range(75):
        alpha = np.frombuffer(b"ACGT"[: int(rng.integers(2, 5))], dtype=np.uint8)
        recs = [rng.choice(alpha, size=int(rng.integers(30, 150))) for _ in range(int(rng.integers(1, 4)))]
        text = bytearray(b"N".join(r.tobytes() for r in recs))  # several records, merged with an N between them
        if rng.integers(0, 2):
            text[int(rng.integers(0, len(text)))] = ord("N")
        text = bytes(text)
        a = int(rng.integers(0, len(text) - 20))
        piece = bytearray(text[a:a + int(rng.integers(20, 120))])
        for _ in range(int(rng.integers(0, 5))):  # substitutions, now and then an N in the read
            piece[int(rng.integers(0, len(piece)))] = int(rng.choice(alpha)) if rng.integers(0, 6) else ord("N")
        q = rng.choice(alpha, size=int(rng.integers(0, 6))).tobytes() + bytes(piece) + rng.choice(alpha, size=int(rng.integers(0, 6))).tobytes()
        o = po.OracleIndex(text)
        min_len = int(rng.integers(3, 9))
        for strand in (q, bytes(ext_spec.revcomp(np.frombuffer(q, dtype=np.uint8)))):
            rows = _rows(o.get_matches(strand, min_len))
            pairs += 1
            for P in (1, 4):
                for X in (0, 5, 20):
                    for r in rows:
                        g, m = check_row(strand, text, r, P, X)
                        grown += g > 0
                        mms += m
                        if X == 0:
                            assert m == 0
                    dropped += check_block(rows, strand, text, P, X)
    assert pairs >= 150 and grown > 100 and mms > 100 and dropped > 10


@pytest.mark.parametrize("case", MEM_CASES)
def test_definition_on_golden_files(case):
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    blocks = mum_spec.parse_mems_file(open(exp_mems, "rb").read(), ref)
    strands = 2 if "-b" in opts else 1
    chars = np.frombuffer(qs.chars, dtype=np.uint8)
    budget = 400  # rows checked exhaustively per case (the checks are per letter, in Python)
    for b, (_, rows) in enumerate(blocks):
        rec = chars[qs.offsets[b // strands]:qs.offsets[b // strands + 1]]
        Q = bytes(ext_spec.revcomp(rec)) if b % strands else rec.tobytes()
        take = rows[: max(0, budget)]
        budget -= len(take)
        for P, X in ((4, 20), (1, 5)):
            for r in take:
                check_row(Q, ref.chars, r, P, X)
            if len(rows) <= 300:
                check_block(rows, Q, ref.chars, P, X)


def test_golden_ext_files_differ_from_the_mem_files_and_have_four_columns():
    grew = fewer = 0
    for case in MEM_CASES:
        plain = open(case_paths(case)[2], "rb").read()
        data, kept, mms, ref, _, _ = ext_spec.golden_ext_file(case)
        grew += any(int(m.sum()) > 0 for m in mms)
        fewer += data.count(b"\n") < plain.count(b"\n")
        for ln in data.split(b"\n")[:-1]:
            if not ln.startswith(b">"):
                assert len(ln.split(b"\t")) == (5 if ref.s.num > 1 else 4)
    assert grew >= 5 and fewer >= 3


def test_planted_reads_known_answer_holds_for_the_spec():
    """The GPU test's construction, on the definition: every read gives (a, 0, 200) with the planted number of mismatches, once,
    from every maximal exact run of 20 letters or more on its true diagonal."""
    ref, q, off, truth = ext_spec.planted_reads(5, count=300)
    T = ref.tobytes()
    runs = 0
    for k, (a, rev, planted) in enumerate(truth):
        rec = q[int(off[k]):int(off[k + 1])]
        Q = bytes(ext_spec.revcomp(rec)) if rev else rec.tobytes()
        eq = np.frombuffer(Q, dtype=np.uint8) == ref[a:a + 200]
        assert int((~eq).sum()) == planted
        edges = np.flatnonzero(np.diff(np.concatenate([[0], eq.astype(np.int8), [0]])))
        rows = [(a + s, s, e - s) for s, e in zip(edges[::2], edges[1::2]) if e - s >= 20]
        assert rows
        runs += len(rows)
        k2, m2, keep = ext_spec.block_ext(np.array(rows[::-1]), Q, T)  # (q descending, as the engine emits them)
        assert [tuple(int(v) for v in r) for r in k2] == [(a, 0, 200)] and list(m2) == [planted]
        assert list(keep) == [True] + [False] * (len(rows) - 1)
    assert runs > 500
