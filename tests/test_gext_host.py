"""-gext without a GPU: the two forms of tests/gext_spec.py held to each other (fact b) and to a brute-force
enumeration, the attempt on the diagonal k = 0 alone held to 4.13's walk (fact a), fact (c) and 2S = x + y - p on every designed
end, the motivating case written out, and the command line's option row."""
import ctypes as C
import itertools

import numpy as np
import pytest

import affine_spec
import aln_spec
import ext_spec
import gext_end_cases as cases
import gext_spec
import hostlib

DEFAULT = (4, 6, 2)
ALL_COSTS = [DEFAULT, (5, 10, 1), (1, 0, 1)]


def random_pair(rng, longest=40):
    """A piece and a mutated copy of it with a few letters behind, now and then over two letters only."""
    letters = b"ACGT" if rng.random() < 0.7 else b"AC"
    A = bytes(rng.choice(np.frombuffer(letters, dtype=np.uint8), size=int(rng.integers(0, longest + 1))))
    B = bytearray()
    for c in A:
        r = rng.random()
        if r < 0.06:
            B.append(int(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8))))
        elif r < 0.10:
            continue
        elif r < 0.14:
            B += bytes([c, int(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8)))])
        else:
            B.append(c)
    B += bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(rng.integers(0, 6))))
    return A, bytes(B)


@pytest.mark.parametrize("costs", ALL_COSTS)
def test_wavefront_form_equals_matrix_form_when_nothing_is_pruned(costs):
    """Fact (b), on 1,000 random pairs of up to 40 letters per cost triple (3,000 in all)."""
    rng = np.random.default_rng(430 + costs[1])
    gapped = 0
    for _ in range(1000):
        A, B = random_pair(rng)
        Z, P = int(rng.choice([0, 1, 3, 8, 31])), int(rng.choice([1, 4, 6]))
        B = B[:len(A) + Z]
        w = gext_spec.attempt(A, B, Z, P, None, costs)
        assert w == gext_spec.matrix_attempt(A, B, Z, P, costs), (A, B, Z, P)
        assert 2 * w[3] == w[0] + w[1] - w[4] and w[3] == gext_spec.score_of(w[2], P, costs)  # 2S = x + y - p
        gapped += "I" in w[2] or "D" in w[2]
    assert gapped > 100


def alignments(a, b, Z):
    """Every path from (0, 0) inside the band over pieces of a and b letters, as (x, y, steps): M a diagonal step, I a strand
    letter, D a text letter."""
    out = []

    def go(x, y, ops):
        out.append((x, y, ops))
        if x < a and y < b:
            go(x + 1, y + 1, ops + "M")
        if x < a and abs(y - x - 1) <= Z:
            go(x + 1, y, ops + "I")
        if y < b and abs(y + 1 - x) <= Z:
            go(x, y + 1, ops + "D")
    go(0, 0, "")
    return out


@pytest.mark.parametrize("costs", ALL_COSTS)
def test_matrix_form_against_every_alignment_of_short_pieces(costs):
    """No alignment of any prefix pair scores more than the attempt's result, for pieces of up to 6 letters."""
    rng = np.random.default_rng(7)
    P = 4
    for a, b in itertools.product(range(0, 7, 2), range(0, 7, 3)):
        for _ in range(2):
            A = bytes(rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=a))
            B = bytes(rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=b))
            for Z in (0, 1, 3):
                Bz = B[:a + Z]
                best = 0
                for x, y, ops in alignments(a, len(Bz), Z):
                    i = j = 0
                    s = ""
                    for c in ops:
                        if c == "M":
                            s += "=" if A[i] == Bz[j] else "X"
                            i, j = i + 1, j + 1
                        else:
                            s += c
                            i, j = i + (c == "I"), j + (c == "D")
                    best = max(best, gext_spec.score_of(s, P, costs))
                assert gext_spec.matrix_attempt(A, Bz, Z, P, costs)[3] == best, (A, Bz, Z)


@pytest.mark.parametrize("X", [0, 5, 20])
def test_the_diagonal_alone_is_the_ungapped_walk(X):
    """Fact (a): Z = 0 against ext_spec.extend_side on random pairs with N and sequence ends, both directions."""
    rng = np.random.default_rng(413 + X)
    acgt, acgtn = np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(b"ACGTN", dtype=np.uint8)
    nonempty = 0
    for _ in range(1500):
        Q = rng.choice(acgt, size=int(rng.integers(0, 61)))
        T = np.concatenate([Q, rng.choice(acgt, size=5)])
        hit = rng.random(len(T)) < 0.15
        T[hit] = rng.choice(acgtn, size=int(hit.sum()))
        T = T[:int(rng.integers(0, 66))]
        if len(Q) and rng.random() < 0.3:
            Q[len(Q) // 2] = ord("N")
        Qb, Tb = bytes(Q), bytes(T)
        for step in (1, -1):
            qi, ti = (0, 0) if step > 0 else (len(Qb) - 1, len(Tb) - 1)
            ext, best, mm = ext_spec.extend_side(Qb, Tb, qi, ti, step, 4, X)
            A, B = gext_spec.pieces(Qb, Tb, qi, ti, step, 0)
            x, y, ops, S, s = gext_spec.attempt(A, B, 0, 4, X, DEFAULT)
            assert (x, y, S, ops.count("X")) == (ext, ext, best, mm) and set(ops) <= {"=", "X"}
            nonempty += ext > 0
    assert nonempty > 500


def designed_ends(Z):
    """The ends of the catalogue on its own MEMs (the -mem list of the CPU oracle)."""
    from oracle import pyoracle as po
    ref, q, off, labels = cases.catalogue(8)
    mem, counts = po.OracleIndex(ref.tobytes()).match_batch(q, off, cases.MIN_LEN, True)
    boff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ends = []
    blocks = gext_spec.filter_blocks(mem, boff, ref, q, off, True, costs=DEFAULT, Z=Z, ends_out=ends)
    return blocks, ends, (mem, boff, ref, q, off)


@pytest.mark.parametrize("Z", [1, 8, 31])
def test_fact_c_and_the_score_identity_on_every_designed_end(Z):
    blocks, ends, _ = designed_ends(Z)
    replaced = [e for e in ends if e["replaced"]]
    assert len(replaced) >= 10
    for e in ends:
        if e["replaced"]:  # it holds a gap, scores at most a - (o + e), and its end was listed
            assert ("I" in e["ops"] or "D" in e["ops"]) and e["gapped"] <= e["a"] - 8 and e["listed"] and e["gapped"] > e["ungapped"]
            assert e["gapped"] == gext_spec.score_of(e["ops"], 4, DEFAULT) and e["ops"][0] != "="
        elif "listed" in e and not e["listed"]:  # kept without an attempt: the attempt would not have won
            assert e["gapped"] <= e["ungapped"]


def test_band_0_is_the_affine_spec():
    blocks, ends, (mem, boff, ref, q, off) = designed_ends(0)
    assert blocks == affine_spec.filter_blocks(mem, boff, ref, q, off, True, costs=DEFAULT) and not any(e["replaced"] for e in ends)


def test_a_deleted_letter_12_letters_from_the_read_end():
    """The motivating case: a read of 200 letters that lacks the reference letter 12 letters in front of its end is 188= 1D 12=
    with the band (188 + 12 = 200 letters); without it the alignment ends at the deletion and the tail is clipped."""
    rng = np.random.default_rng(12)
    ref = rng.choice(cases.ACGT, size=1000)
    ref[488] = cases.ACGT[(list(cases.ACGT).index(ref[489]) + 1) % 4]  # (the MEM ends at the deleted letter)
    read = np.concatenate([ref[300:488], ref[489:501]])
    assert len(read) == 200
    rows = [(300, 0, 188)]
    Q, T = bytes(read), bytes(ref)
    (seg,) = gext_spec.block_aln(rows, Q, T, Z=8)
    assert aln_spec.cigar_string(seg[5]) == "188=1D12=" and seg[:5] == (300, 0, 201, 200, 1)
    (seg,) = gext_spec.block_aln(rows, Q, T, Z=0)
    assert aln_spec.cigar_string(seg[5]).startswith("188=") and seg[3] < 200 and "D" not in aln_spec.cigar_string(seg[5])


def test_option_row_and_refusals():
    assert ("gext", True) in hostlib.option_rows()
    firsts = [n[:2] for n, _ in hostlib.option_rows() if len(n) > 1]
    assert firsts.count("ge") == 1 and "gt" in firsts  # -gext and -gt differ in the second letter, which the table compares
    ok = ["slaMEM", "-aln", "-affine", "4,6,2", "-gext", "8", "ref.fa", "reads.fa"]
    assert hostlib.parse_run(ok)[:2] == (0, None)
    for mode in (["-paf"], ["-sam"], ["-pile"], ["-vcf", "-gt"], ["-stats"]):
        assert hostlib.parse_run(["slaMEM"] + mode + ["-affine", "4,6,2", "-gext", "31", "ref.fa", "reads.fa"])[:2] == (0, None)
    rc, refusal, _ = hostlib.parse_run(["slaMEM", "-aln", "-gext", "8", "ref.fa", "reads.fa"])
    assert rc != 0 and refusal == "Option -gext needs -affine"
    for bad in ("0", "32", "-1", "x", "8x"):
        rc, refusal, _ = hostlib.parse_run(["slaMEM", "-aln", "-affine", "4,6,2", "-gext", bad, "ref.fa", "reads.fa"])
        assert rc != 0 and refusal == "Option -gext needs a whole number from 1 to 31", bad
    for mode in ([], ["-mum"], ["-chain"], ["-ext"]):
        rc, refusal, _ = hostlib.parse_run(["slaMEM"] + mode + ["-gext", "8", "ref.fa", "reads.fa"])
        assert rc != 0 and refusal == "Option -gext needs -aln"
    L = hostlib.lib()
    v = C.c_int(-5)
    argv = hostlib.c_argv(ok)
    assert L.slh_parse_gext(len(ok), argv, C.byref(v)) == 1 and v.value == 8
