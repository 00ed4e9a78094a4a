"""The designed reads of -sv: one family per edge of the definition in tests/sv_spec.py, each on both strands, and
a random batch with planted long indels.  Seeded; numpy alone.  tests/test_sv_host.py proves from the oracle and the specs that every
read maps into the designed segments and yields exactly its designed junction or skip; tests/test_gpu_sv.py runs the same reads
through the engine.

The reference is 40,000 random letters in two records of 20,000 (the merged text: a separator N at 20000), with two plants: four
copies of a 40-letter unit from 3000 (other letters in front and behind), and an N at 26100.  Reads are 250 letters, searched at
-l 20, -maxed 31 -- but for the 300-letter deletions and the 120-letter insertion, whose reads are longer: the chain of 4.12 pays
|difference of the diagonals| for a link, so two anchors across an indel of L letters are one chain, and that chain the block's best, only when
the letters in front of the break and those behind it each score more than L.  Those reads carry L + 30 letters on either side of the
break; the random batch's reads carry a tenth more, for their substitutions.

A deletion of L rows at d is *clean* when T[d-1] != T[d+L-1] and T[d] != T[d+L]: neither anchor runs into the other's letters, the
break lies at d exactly and nothing normalises.  A mutated letter differs from the text on both diagonals."""
import numpy as np

import events_spec as es
import ext_spec

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
READ_LEN, MIN_LEN, MAXED = 250, 20, 31
SLOPPY = 60  # rows of the deletions whose break is blurred by mismatches: fewer than the 85 letters that stay in front of the slop
SEPARATOR, PLANTED_N = 20000, 26100
REPEAT, UNIT, COPIES = 3000, 40, 4


def reference() -> np.ndarray:
    rng = np.random.default_rng(4031)
    t = rng.choice(ACGT, size=40001)
    unit = rng.choice(ACGT, size=UNIT)
    t[REPEAT:REPEAT + UNIT * COPIES] = np.tile(unit, COPIES)
    t[REPEAT - 1] = ACGT[(int(np.nonzero(ACGT == unit[-1])[0][0]) + 1) % 4]   # (the repeat starts at REPEAT ...)
    t[REPEAT + UNIT * COPIES] = ACGT[(int(np.nonzero(ACGT == unit[0])[0][0]) + 1) % 4]  # (... and ends behind its fourth copy)
    t[SEPARATOR] = t[PLANTED_N] = ord("N")
    return t


def clean(T, d: int, L: int) -> bool:
    return T[d - 1] != T[d + L - 1] and T[d] != T[d + L]


def find_clean(T, start: int, L: int) -> int:
    d = start
    while not clean(T, d, L):
        d += 1
    return d


def other_letter(*avoid) -> int:
    """The first of A,C,G,T that is none of the given letters."""
    return next(int(c) for c in ACGT if all(int(c) != (int(a) & 0xDF) for a in avoid))


def del_read(T, d: int, L: int, left: int = 125, right: int = 125) -> np.ndarray:
    return np.concatenate([T[d - left:d], T[d + L:d + L + right]])


def mutated(T, d: int, L: int, a_side=(), b_side=(), letter=None, left: int = 125) -> np.ndarray:
    """del_read with the k-th letter in front of the break (a_side) or behind it (b_side) changed."""
    r = del_read(T, d, L, left).copy()
    for k in a_side:   # read letter left - k lies on a's diagonal at row d - k, on b's at row d + L - k
        r[left - k] = other_letter(T[d - k], T[d + L - k]) if letter is None else letter
    for k in b_side:   # read letter left + k - 1 lies on b's diagonal at row d + L + k - 1, on a's at row d + k - 1
        r[left + k - 1] = other_letter(T[d + L + k - 1], T[d + k - 1]) if letter is None else letter
    return r


def catalogue():
    """(reference, cases): a case is a dict of name, read (forward, uint8), segments (how many the read maps into), expect (the
    classified junctions in ascending order of the scanned strand at max_mis 3) and expect4 (at max_mis 4)."""
    T = reference()
    rng = np.random.default_rng(4032)
    cases = []

    def case(name, read, segments, expect, expect4=None, length=READ_LEN):
        assert len(read) == length, (name, len(read))
        cases.append(dict(name=name, read=np.asarray(read, dtype=np.uint8), segments=segments, expect=expect,
                          expect4=expect if expect4 is None else expect4))

    def key(pos, kind, L):
        return ("key", int(pos), kind, L)

    def norm_del(d, L):
        return es.normalise(bytes(T), d, 0, L)[0]

    # a 300-letter deletion, nothing shared: m = 0
    d = find_clean(T, 1000, 300)
    case("del300", del_read(T, d, 300, 330, 330), 2, [key(d, 0, 300)], length=660)
    # one copy of the tandem repeat is missing: the anchors meet behind the third copy, normalisation walks to the first
    last = REPEAT + UNIT * (COPIES - 1)
    case("tandem", np.concatenate([T[REPEAT - 65:REPEAT], T[REPEAT:last], T[last + UNIT:last + UNIT + 65]]), 2, [key(REPEAT, 0, UNIT)])
    # maxed + 1 letters do not close, maxed letters do
    d = find_clean(T, 5000, MAXED + 1)
    case("del_maxed_plus_1", del_read(T, d, MAXED + 1), 2, [key(d, 0, MAXED + 1)])
    d = find_clean(T, 6000, MAXED)
    case("del_maxed", del_read(T, d, MAXED), 1, [])
    # a mismatch k letters from the break: on a's side at k = 1 the split ties between t = 0 and t = 1 and takes t = 0 (the deletion
    # moves one row to the left); on b's side at k = 1 it ties as well and t = 0 is the break itself
    for i, (side, k) in enumerate([("a", 1), ("a", 3), ("a", 20), ("b", 1), ("b", 3), ("b", 20)]):
        d = find_clean(T, 7000 + 500 * i, SLOPPY)
        read = mutated(T, d, SLOPPY, a_side=(k,)) if side == "a" else mutated(T, d, SLOPPY, b_side=(k,))
        case("mis_%s%d" % (side, k), read, 2, [key(norm_del(d - 1, SLOPPY) if (side, k) == ("a", 1) else d, 0, SLOPPY)])
    # the slop: 40 letters on a's side and 24 / 25 on b's (runs of at most 19 between the mutated letters: no anchor among them)
    d = find_clean(T, 10500, SLOPPY)
    case("slop64", mutated(T, d, SLOPPY, a_side=(40, 20), b_side=(20, 24)), 2, [("skip", 3)], [key(d, 0, SLOPPY)])
    d = find_clean(T, 11000, SLOPPY)
    case("slop65", mutated(T, d, SLOPPY, a_side=(40, 20), b_side=(20, 25)), 2, [("skip", 3)])
    # max_mis mismatches in the slop are stored (slop64 has max_mis + 1)
    d = find_clean(T, 11500, SLOPPY)
    case("mis3", mutated(T, d, SLOPPY, a_side=(40, 20), b_side=(20,)), 2, [key(d, 0, SLOPPY)])
    # an N in the slop, an N in the deleted rows, a break across the separator
    d = find_clean(T, 12000, SLOPPY)
    case("n_in_slop", mutated(T, d, SLOPPY, a_side=(3,), letter=ord("N")), 2, [("skip", 2)])
    d = find_clean(T, PLANTED_N - 150, 300)
    assert d < PLANTED_N < d + 300
    case("n_in_rows", del_read(T, d, 300, 330, 330), 2, [("skip", 2)], length=660)
    case("separator", np.concatenate([T[SEPARATOR - 125:SEPARATOR], T[SEPARATOR + 100:SEPARATOR + 225]]), 2, [("skip", 2)])
    # an insertion of 120 letters that neither anchor runs into
    d = 12600
    ins = rng.choice(ACGT, size=120)
    ins[0], ins[-1] = other_letter(T[d]), other_letter(T[d - 1])
    case("ins120", np.concatenate([T[d - 150:d], ins, T[d:d + 150]]), 2, [key(d, 1, 120)], length=420)
    # an insertion that repeats the 40 letters in front of it: normalisation walks past all of them
    d = 13000
    p = es.normalise(bytes(T), d, 1, 40, es.fold(bytes(T[d - 40:d])))[0]
    assert p <= d - 40
    case("dup40", np.concatenate([T[d - 105:d], T[d - 40:d], T[d:d + 105]]), 2, [key(p, 1, 40)])
    # an insertion with an N among its letters: they are not compared and not part of the key, so the junction is stored
    d = 13500
    ins = rng.choice(ACGT, size=40)
    ins[0], ins[20], ins[-1] = other_letter(T[d]), ord("N"), other_letter(T[d - 1])
    case("ins_with_n", np.concatenate([T[d - 105:d], ins, T[d:d + 105]]), 2, [key(d, 1, 40)])
    # a divergent stretch of 100 letters: balanced, whatever its slop
    d = 14000
    div = np.array([other_letter(c) for c in T[d:d + 100]], dtype=np.uint8)
    case("balanced", np.concatenate([T[d - 75:d], div, T[d + 100:d + 175]]), 2, [("skip", 0)])
    # three segments: deletions of 40 and of 50 rows, 85 letters apart
    d = 15000
    while not (clean(T, d, 40) and clean(T, d + 125, 50)):
        d += 1
    case("three", np.concatenate([T[d - 80:d], T[d + 40:d + 125], T[d + 175:d + 260]]), 3, [key(d, 0, 40), key(d + 125, 0, 50)])
    return T, cases


def batch(cases):
    """The catalogue's reads as a batch: read 2c is case c as designed (strand 1), read 2c + 1 its reverse complement (strand 2)."""
    reads = []
    for c in cases:
        reads += [c["read"], ext_spec.revcomp(c["read"])]
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return np.concatenate(reads), off


def expected_table(cases, which: str = "expect"):
    """(junctions, skipped) the catalogue's batch gives: every designed key once from each strand."""
    keys, skipped = {}, [0, 0, 0, 0]
    for c in cases:
        for j in c[which]:
            if j[0] == "skip":
                skipped[j[1]] += 2
            else:
                k = keys.setdefault(j[1:], [0, 0])
                k[0] += 1
                k[1] += 1
    return sorted(k + tuple(v) for k, v in keys.items()), skipped


# ---- a random batch with planted long indels -------------------------------------------------------------------------------------

ROOMY = [(2400, 15600), (28500, 35600)]  # breaks around which a deletion of 2,000 rows and both flanks stay clear of the two N


def random_batch(seed: int = 4033, count: int = 400, sub_rate: float = 0.01):
    """(reference, reads, offsets, plants): read r holds one planted deletion or insertion of L = 130 to 2,000 letters between two
    flanks of L + 60 + L // 10 letters, with substitutions at sub_rate, on a random strand.  plants[r] = (kind, row, length)."""
    T = reference()
    rng = np.random.default_rng(seed)
    reads, plants = [], []
    for _ in range(count):
        kind, L = int(rng.integers(0, 2)), int(rng.integers(130, 2001))
        lo, hi = ROOMY[int(rng.integers(0, len(ROOMY)))]
        d = int(rng.integers(lo, hi))
        f = L + 60 + L // 10  # (a flank's chain loses a few points per substitution)
        r = del_read(T, d, L, f, f) if kind == 0 else np.concatenate([T[d - f:d], rng.choice(ACGT, size=L), T[d:d + f]])
        r = r.copy()
        hit = np.nonzero(rng.random(len(r)) < sub_rate)[0]
        r[hit] = ACGT[(np.searchsorted(ACGT, r[hit] & 0xDF) + rng.integers(1, 4, size=len(hit))) % 4]
        reads.append(ext_spec.revcomp(r) if rng.integers(0, 2) else r)
        plants.append((kind, d, L))
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return T, np.concatenate(reads), off, plants
