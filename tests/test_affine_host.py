"""-affine on the CPU: the three forms of the definition held to each other -- the Gotoh matrices of
tests/affine_spec.py, the Python model of what k_aln_wave_affine stores and reads, and an enumeration of every alignment of short
pieces -- the two facts the design rests on (costs 1,0,1 are unit cost byte for byte; the inline tier of k_aln_geom), the
motivating case written out, the word that carries the costs and the command line's option row."""
import ctypes as C
import functools

import numpy as np
import pytest

import affine_spec
import aln_gap_cases
import aln_spec
import ext_spec
import hostlib
from golden_cases import CASES, MANIFEST
from oracle import pyoracle as po

COSTS = [(4, 6, 2), (1, 0, 1), (5, 10, 1), (2, 0, 3), (31, 63, 31)]
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]


def _rows(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


def check_gap(A, B, E, costs):
    """Matrix form against wavefront form on one gap, and what any alignment must satisfy.  Returns the matrix form's result."""
    g = affine_spec.gap_ops(A, B, E, costs)
    w = affine_spec.wavefront_ops(A, B, E, costs)
    assert w == g, (A, B, E, costs, g, w)
    if g is not None:
        ops, edits, cost = g
        assert cost == affine_spec.cost_of(ops, *costs) <= affine_spec.bound(E, costs)
        assert edits == sum(c != "=" for c in ops)
        assert ops.count("=") + ops.count("X") + ops.count("I") == len(A) and ops.count("=") + ops.count("X") + ops.count("D") == len(B)
    return g


@functools.lru_cache(maxsize=None)
def chain_gaps():
    """(A, B) of every gap of the constructed reads and of the golden cases, as the chain leaves them."""
    gaps = []
    ref, q, off, truth = aln_spec.constructed_reads(11)
    T = ref.tobytes()
    o = po.OracleIndex(T)
    for k, (b, _, _) in enumerate(truth):
        rec = q[int(off[k]):int(off[k + 1])]
        Q = bytes(ext_spec.revcomp(rec)) if b % 2 else rec.tobytes()
        aln_spec.block_aln(_rows(o.get_matches(Q, 20)), Q, T, gaps_out=gaps)
    for case in MEM_CASES:
        aln_spec.golden_aln(case, gaps_out=gaps)
    seen = {(bytes(A), bytes(B)) for A, B, _ in gaps}
    return sorted(seen)


@pytest.mark.parametrize("costs", COSTS)
def test_matrix_against_wavefront_on_chain_gaps(costs):
    closed = 0
    for A, B in chain_gaps():
        if len(A) * len(B) > 40_000:  # (the model is letter-wise Python)
            continue
        for E in (31, 3) if costs != (31, 63, 31) else (14, 3):
            closed += check_gap(A, B, E, costs) is not None
    assert closed >= 50  # (the distinct gaps of 240 reads with one to three edits and of the golden cases)


@pytest.mark.parametrize("costs,E", [((4, 6, 2), 127), ((4, 6, 2), 64), ((4, 6, 2), 31), ((1, 0, 1), 127), ((5, 10, 1), 127), ((2, 0, 3), 40),
                                     ((31, 63, 31), 14)])
def test_matrix_against_wavefront_on_designed_gaps(costs, E):
    """The pieces of aln_gap_cases as designed (equal first letters and empty sides among them)."""
    closed = broken = 0
    for label, A, B in aln_gap_cases.pieces():
        if len(A) * len(B) > 50_000 and (costs, E) != ((4, 6, 2), 127):
            continue
        g = check_gap(A, B, E, costs)
        closed, broken = closed + (g is not None), broken + (g is None)
    assert closed >= 8 and broken >= 3  # (broken: at least the pieces with an N)


def test_matrix_against_wavefront_on_short_random_pieces_and_both_sides_of_the_bound():
    rng = np.random.default_rng(429)
    alpha = np.frombuffer(b"AC", dtype=np.uint8)
    at_bound, excess, closed = set(), {c: set() for c in COSTS}, 0
    for _ in range(3000):
        A = rng.choice(alpha, size=int(rng.integers(0, 9))).tobytes()
        B = rng.choice(alpha, size=int(rng.integers(0, 9))).tobytes()
        for costs in COSTS:
            x, o, e = costs
            H = affine_spec.gotoh(A, B, x, o, e)[0]
            for E in (0, 1, 3, 8):
                g = check_gap(A, B, E, costs)
                h, bound = int(H[len(A)][len(B)]), affine_spec.bound(E, costs)
                assert (g is not None) == (h <= bound and abs(len(A) - len(B)) <= E)
                closed += g is not None
                if g is not None and h == bound:
                    at_bound.add(costs)
                if g is None and abs(len(A) - len(B)) <= E:
                    excess[costs].add(h - bound)
    assert closed > 15_000
    # Costs of exactly C (closing) and of the next cost above it (breaking) are met.  That is C + 1 where the costs can form it.  With
    # 4,6,2 every cost and C = 6 + 2 E are even: C + 2.  With 31,63,31 a cost is 31 (i + k) + 63 j for i mismatches, j gaps and k gap
    # letters, so above C = 63 + 31 E by 31 m - 63 without a gap (30 for m = 3) and by 31 m with one; 1 needs two gaps.
    assert at_bound == set(COSTS)
    for costs, least in (((1, 0, 1), 1), ((5, 10, 1), 1), ((2, 0, 3), 1), ((4, 6, 2), 2), ((31, 63, 31), 30)):
        assert min(excess[costs]) == least, costs


@functools.lru_cache(maxsize=None)
def _paths(a: int, b: int):
    """Every alignment of a and b letters as a string over M (a letter of both), I, D."""
    if a == 0 and b == 0:
        return ("",)
    out = []
    if a and b:
        out += [p + "M" for p in _paths(a - 1, b - 1)]
    if a:
        out += [p + "I" for p in _paths(a - 1, b)]
    if b:
        out += [p + "D" for p in _paths(a, b - 1)]
    return tuple(out)


def brute_force(A: bytes, B: bytes, x: int, o: int, e: int) -> int:
    best = None
    for p in _paths(len(A), len(B)):
        i = j = c = 0
        last = ""
        for ch in p:
            if ch == "M":
                c += x if A[i] != B[j] else 0
                i, j = i + 1, j + 1
            else:
                c += e + (o if ch != last else 0)
                i, j = i + (ch == "I"), j + (ch == "D")
            last = ch
        best = c if best is None or c < best else best
    return best


def test_matrix_cost_against_every_alignment_of_short_pieces():
    rng = np.random.default_rng(430)
    alpha = np.frombuffer(b"ACG", dtype=np.uint8)
    for t in range(80):
        A = rng.choice(alpha, size=int(rng.integers(0, 7 if t < 12 else 6))).tobytes()
        B = rng.choice(alpha, size=int(rng.integers(0, 7 if t < 12 else 6))).tobytes()
        for x, o, e in COSTS:
            H = affine_spec.gotoh(A, B, x, o, e)[0]
            assert int(H[len(A)][len(B)]) == brute_force(A, B, x, o, e), (A, B, x, o, e)


# ---- fact (a): costs 1, 0, 1 are unit cost -----------------------------------------------------------------------------------

def test_unit_costs_reproduce_aln_spec_operation_for_operation():
    rng = np.random.default_rng(431)
    alpha = np.frombuffer(b"AC", dtype=np.uint8)
    pieces = [(A, B) for A, B in chain_gaps() if len(A) * len(B) <= 40_000]
    pieces += [(A, B) for _, A, B in aln_gap_cases.pieces()]
    pieces += [(rng.choice(alpha, size=int(rng.integers(0, 9))).tobytes(), rng.choice(alpha, size=int(rng.integers(0, 9))).tobytes())
               for _ in range(3000)]
    closed = 0
    for A, B in pieces:
        for E in (0, 1, 3, 31, 127):
            if E == 127 and len(A) * len(B) > 50_000:
                continue
            want = aln_spec.gap_ops(A, B, E)
            got = affine_spec.gap_ops(A, B, E, (1, 0, 1))
            assert (got is None) == (want is None)
            if want is not None:
                assert got == (want[0], want[1], want[1])  # operations, edits = distance = cost
                closed += 1
    assert closed > 5000


# ---- fact (b): the inline tier -----------------------------------------------------------------------------------------------

def _pieces_of_mask(rng, m: int, n: int):
    B = rng.choice(aln_gap_cases.ACGT, size=n)
    A = B.copy()
    for t in range(n):
        if (m >> t) & 1:
            A[t] = rng.choice(aln_gap_cases.ACGT[aln_gap_cases.ACGT != B[t]])
    return A.tobytes(), B.tobytes()


@pytest.mark.parametrize("costs", COSTS)
def test_inline_rule_of_the_geometry_kernel(costs):
    """Pieces of one length n <= 64 whose differing letters are the bits of a mask: with d x <= 2 (o + e) the matrix form stays on
    the diagonal -- closed iff d x <= C, the runs those of the mask.  Every mask for n <= 7, sampled ones up to 64 letters, and
    d x == 2 (o + e) exactly wherever x divides it."""
    x, o, e = costs
    rng = np.random.default_rng(432)
    dmax = 2 * (o + e) // x
    masks = [(m, n) for n in range(1, 8) for m in range(1 << n) if bin(m).count("1") <= dmax]
    for n in (8, 20, 33, 63, 64):
        for d in sorted({0, 1, 2, max(0, dmax - 1), dmax}):
            if d > n:
                continue
            for _ in range(12):
                places = rng.choice(n, size=d, replace=False)
                masks.append((sum(1 << int(p) for p in places), n))
            masks.append(((1 << d) - 1, n))             # the first letters
            masks.append((((1 << d) - 1) << (n - d), n))  # the last letters
    exact = closed = broken = 0
    for m, n in masks:
        A, B = _pieces_of_mask(rng, m, n)
        d = bin(m).count("1")
        for E in (31, 3, 0):
            rule = affine_spec.inline_rule(m, n, E, costs)
            g = affine_spec.gap_ops(A, B, E, costs)
            assert rule[0] != "listed"
            if rule[0] == "closed":
                assert g == (rule[1], d, d * x), (m, n, E, costs)
                closed += 1
            else:
                assert g is None
                broken += 1
            exact += d * x == 2 * (o + e)
    assert closed > 500 and (broken > 0 or x * dmax <= o) and (exact > 0 or (2 * (o + e)) % x)
    # one more differing letter is not decided inline
    assert affine_spec.inline_rule((1 << (dmax + 1)) - 1, 64, 31, costs) == ("listed",) or dmax + 1 > 64


def test_default_costs_take_four_letters_inline_where_unit_cost_takes_two():
    assert affine_spec.inline_rule(0b1111, 8, 31, (4, 6, 2))[0] == "closed" and affine_spec.inline_rule(0b11111, 8, 31, (4, 6, 2)) == ("listed",)
    assert affine_spec.inline_rule(0b11, 8, 31, (1, 0, 1))[0] == "closed" and affine_spec.inline_rule(0b111, 8, 31, (1, 0, 1)) == ("listed",)


# ---- the motivating case -----------------------------------------------------------------------------------------------------

def three_substitutions():
    """Two anchors of 160 letters around 12 letters of which three differ, five letters apart: (reference, read)."""
    rng = np.random.default_rng(433)
    left, right = rng.choice(aln_gap_cases.ACGT, size=160), rng.choice(aln_gap_cases.ACGT, size=160)
    left[-1], right[0] = ord("A"), ord("C")  # (the anchors end where the design says)
    B = np.frombuffer(b"CTTTTTGGGGGA", dtype=np.uint8)
    A = np.frombuffer(b"TTTTTGGGGGAA", dtype=np.uint8)
    pad = rng.choice(aln_gap_cases.ACGT, size=100)
    return np.concatenate([pad, left, B, right, pad]).astype(np.uint8), np.concatenate([left, A, right]).astype(np.uint8)


def test_three_clustered_substitutions_are_an_indel_pair_at_unit_cost_and_three_x_at_affine_cost():
    ref, read = three_substitutions()
    T, Q = ref.tobytes(), read.tobytes()
    rows = _rows(po.OracleIndex(T).get_matches(Q, 20))
    unit = affine_spec.block_aln(rows, Q, T, costs=None)
    aff = affine_spec.block_aln(rows, Q, T, costs=(4, 6, 2))
    assert len(unit) == len(aff) == 1
    assert aln_spec.cigar_string(unit[0][5]) == "160=1D10=1I161=" and unit[0][4] == 2
    assert aln_spec.cigar_string(aff[0][5]) == "160=1X4=1X4=1X161=" and aff[0][4] == 3
    assert unit[0][:4] == aff[0][:4] == (100, 0, 332, 332)


# ---- the word and the option ---------------------------------------------------------------------------------------------------

def _decode(word):
    L = hostlib.lib()
    L.slh_aln_word_decode.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    f, aff = (C.c_uint32 * 4)(), C.c_int()
    rc = L.slh_aln_word_decode(word, f, C.byref(aff))
    return rc, tuple(f), aff.value


def test_word_packing_and_every_refusal_of_the_decoder():
    L = hostlib.lib()
    L.slh_aln_word.restype = C.c_uint32
    L.slh_aln_word.argtypes = [C.c_int] * 5
    assert L.slh_aln_word(-1, 0, 0, 0, 0) == 0xFFFFFFFF and L.slh_aln_word(40, 0, 9, 9, 9) == 40  # without -affine: as before
    assert L.slh_aln_word(-1, 1, 4, 6, 2) == affine_spec.aln_word(31, (4, 6, 2)) == 31 | 4 << 8 | 6 << 16 | 2 << 24
    assert L.slh_aln_word(127, 1, 31, 63, 31) == affine_spec.aln_word(127, (31, 63, 31)) == 0x1F3F1F7F
    assert _decode(0xFFFFFFFF) == (0, (31, 1, 0, 1), 0)          # the default: unit cost, 31
    assert _decode(0) == (0, (0, 1, 0, 1), 0) and _decode(127) == (0, (127, 1, 0, 1), 0)  # upper bits zero: unit cost
    assert _decode(128)[0] == 1 and _decode(255)[0] == 1
    assert _decode(affine_spec.aln_word(31, (4, 6, 2))) == (0, (31, 4, 6, 2), 1)
    assert _decode(affine_spec.aln_word(127, (1, 0, 1))) == (0, (127, 1, 0, 1), 1)  # costs 1,0,1 given: through the affine kernel
    assert _decode(affine_spec.aln_word(14, (31, 63, 31))) == (0, (14, 31, 63, 31), 1)
    assert _decode(affine_spec.aln_word(128, (4, 6, 2)))[0] == 1
    assert _decode(31 | 0 << 8 | 6 << 16 | 2 << 24)[0] == 2 and _decode(affine_spec.aln_word(31, (32, 6, 2)))[0] == 2
    assert _decode(affine_spec.aln_word(31, (4, 64, 2)))[0] == 3
    assert _decode(31 | 4 << 8 | 6 << 16)[0] == 4 and _decode(affine_spec.aln_word(3, (4, 6, 32)))[0] == 4
    assert _decode(affine_spec.aln_word(127, (4, 6, 4)))[0] == 5 and _decode(affine_spec.aln_word(15, (31, 63, 31)))[0] == 5
    assert _decode(affine_spec.aln_word(126, (4, 8, 4)))[0] == 0  # 8 + 4 * 126 = 512 exactly


def test_engine_word_is_the_same_packing():
    from slamem_amd import engine
    assert engine.aln_word(None, None) is None and engine.aln_word(40, None) == 40  # gap_costs=None: the word passed before
    assert engine.aln_word(None, (4, 6, 2)) == affine_spec.aln_word(31, (4, 6, 2))
    assert engine.aln_word(0, (1, 0, 1)) == 1 << 8 | 1 << 24
    for E, costs in ((31, (0, 6, 2)), (31, (32, 6, 2)), (31, (4, 64, 2)), (31, (4, 6, 0)), (31, (4, 6, 32)), (128, (4, 6, 2)), (127, (4, 6, 4))):
        with pytest.raises(ValueError):
            engine.aln_word(E, costs)


def _affine(args):
    L = hostlib.lib()
    L.slh_parse_affine.argtypes = [C.c_int, C.POINTER(C.c_char_p)] + [C.POINTER(C.c_int)] * 3
    v = [C.c_int() for _ in range(3)]
    return (L.slh_parse_affine(len(args), hostlib.c_argv(args), *[C.byref(t) for t in v]),) + tuple(t.value for t in v)


REFUSAL = "Option -affine needs three whole numbers X,O,E: "


def test_option_row_value_parser_and_refusals():
    assert ("affine", True) in hostlib.option_rows()
    assert _affine(["x", "-aln", "a", "b"]) == (0, 0, 0, 0)
    assert _affine(["x", "-aln", "-affine", "4,6,2", "a", "b"]) == (1, 4, 6, 2) and _affine(["x", "-AFFINE", "31,63,31"]) == (1, 31, 63, 31)
    assert _affine(["x", "-af", "1,0,1", "a"]) == (1, 1, 0, 1)  # the first two letters decide
    for bad in ("", "4", "4,6", "4,6,2,1", "4,6,", ",6,2", "0,6,2", "32,6,2", "4,64,2", "4,6,0", "4,6,32", "4;6;2", "4,6,2x", "-4,6,2", "4, 6,2",
                "a,b,c", "4,,2"):
        assert _affine(["x", "-aln", "-affine", bad, "a", "b"])[0] == -1, bad
    assert _affine(["x", "-aln", "a", "-affine"])[0] == -1  # nothing behind it
    # the value is not a file; the files stay the files
    o = hostlib.parse_options(["slaMEM", "-aln", "-affine", "4,6,2", "ref.fa", "reads.fa"])
    assert o["match_type"] == 6 and o["files"] == ["ref.fa", "reads.fa"]
    for mode in ("-aln", "-paf", "-sam", "-stats", "-pile", "-sites", "-vcf", "-cons", "-depth"):
        rc, refusal, _ = hostlib.parse_run(["slaMEM", mode, "-affine", "4,6,2", "ref.fa", "reads.fa"])
        assert (rc, refusal) == (0, None), mode
    rc, refusal, v = hostlib.parse_run(["slaMEM", "-vcf", "-gt", "-affine", "5,10,1", "-maxed", "127", "ref.fa", "reads.fa"])
    assert (rc, refusal, v["max_edits"]) == (0, None, 127)
    for mode in ([], ["-mam"], ["-mum"], ["-smem"], ["-chain"], ["-ext"]):
        rc, refusal, _ = hostlib.parse_run(["slaMEM"] + mode + ["-affine", "4,6,2", "ref.fa", "reads.fa"])
        assert (rc, refusal) == (-1, "Option -affine needs -aln"), mode
    for bad in ("4,6", "0,6,2", "4,64,2", "x"):
        rc, refusal, _ = hostlib.parse_run(["slaMEM", "-aln", "-affine", bad, "ref.fa", "reads.fa"])
        assert rc == -1 and refusal.startswith(REFUSAL), bad
    # o + e E above the cap: 6 + 4 * 127 = 514, and 63 + 31 * 31 with the default 31
    for args in (["-affine", "4,6,4", "-maxed", "127"], ["-affine", "31,63,31"]):
        rc, refusal, _ = hostlib.parse_run(["slaMEM", "-aln"] + args + ["ref.fa", "reads.fa"])
        assert rc == -1 and "at most 512" in refusal and refusal.startswith("Option -affine"), args
    assert hostlib.parse_run(["slaMEM", "-aln", "-affine", "4,8,4", "-maxed", "126", "ref.fa", "reads.fa"])[:2] == (0, None)
    assert hostlib.parse_run(["slaMEM", "-aln", "-affine", "31,63,31", "-maxed", "14", "ref.fa", "reads.fa"])[:2] == (0, None)
