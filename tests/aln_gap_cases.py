"""Designed gaps for -aln, -paf and -pile above 31 edits per gap: a deterministic builder of reads whose one gap
has a shape chosen for what k_aln_wave does there, and the assertions that such gaps are really met -- computed from the gaps a
run of aln_spec saw (its gaps_out), not from the labels, and shared by the CPU and the GPU tests.

A case is a random A,C,G,T reference of 50 kbp with a few planted places (a run of 150 A, (AC) x 100, (ACG) x 70, three N) and
reads of the form 160 exact letters, a designed middle, 160 exact letters, to be searched with -l 20 on both strands (the
chain's link of 4.12 subtracts the shift between two anchors' diagonals, so an anchor has to be longer than the largest indel, 128
letters, for the chain to take both; the cheap reads of bulk() make do with 80).  The middle
pairs a piece B of the reference with a piece A of the read; no exact match of 20 letters survives inside it (substitutions are at
most 15 letters apart, inserted letters are random), and wherever both pieces have letters their first and their last letters are
substituted, so the anchors end where the design says and the gap is (A, B) itself.  Every third read is reverse-complemented.

  catalogue()   the smallest shapes at which the paths of the kernel above 31 edits are reached: pure deletions and insertions
                around 32, 64, 96 and 128 letters, equal-length pieces of 130, 200 and 400 letters with a set number of
                substitutions, an indel with scattered substitutions, a replaced stretch (|a - b| small, the distance large),
                pieces of 63..65 and 127..129 letters on either side, deletions inside the three tandem repeats (many optimal
                alignments: the rule "diagonal, then D, then I" decides), an N beyond the first 64 letters of either piece
  bulk()        1,150 cheap reads -- a deletion or an insertion of 33..60 letters and one substitution nine letters on, each one
                listed gap -- mixed with 40 expensive reads of the catalogue: more listed gaps than k_aln_wave has workgroups at
                127 edits (514), every one of which then closes a second gap in the same LDS and slab

Both return (reference, reads, offsets, labels)."""
import functools

import numpy as np

import aln_spec
import ext_spec

EDITS = (31, 32, 63, 64, 65, 96, 127)  # the edit limits the designed gaps are compared at
MIN_LEN = 20
FLANK = 160
BULK_FLANK = 80
REF_LEN = 50_000
BULK_READS = 1150
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_FREE = 4000  # the planted places lie in front of this row; reads at random places behind it
HOMOPOLYMER, AC_REPEAT, ACG_REPEAT = (400, 550), (900, 1100), (1500, 1710)
TEXT_N = (2200, 2600, 3100)


@functools.lru_cache(maxsize=None)
def _reference() -> bytes:
    rng = np.random.default_rng(4140)
    ref = rng.choice(ACGT, size=REF_LEN)
    for (s, e), unit in ((HOMOPOLYMER, b"A"), (AC_REPEAT, b"AC"), (ACG_REPEAT, b"ACG")):
        ref[s:e] = np.frombuffer(unit * ((e - s) // len(unit)), dtype=np.uint8)
        ref[s - 1] = ref[e] = ord("T")
    for p in TEXT_N:
        ref[p] = ord("N")
    return ref.tobytes()


def reference() -> np.ndarray:
    return np.frombuffer(_reference(), dtype=np.uint8).copy()


def _other(rng, c: int) -> int:
    return int(rng.choice(ACGT[ACGT != (c & 0xDF)]))


def _spread(length: int, d: int):
    """d distinct places in [0, length), evenly spread, the first and the last letter among them."""
    assert 2 <= d <= length
    return [int(np.floor(t * (length - 1) / (d - 1) + 0.5)) for t in range(d)]


def _middle(rng, B: np.ndarray, nsub: int = 0, dele: int = 0, ins: int = 0) -> np.ndarray:
    """The read's piece: B with `dele` letters cut out of its middle, nsub substitutions spread over the rest (its first and last
    letter among them), and `ins` random letters put where the cut is."""
    x = (len(B) - dele) // 2
    kept = np.concatenate([B[:x], B[x + dele:]]).astype(np.uint8)
    if nsub:
        for p in _spread(len(kept), nsub):
            kept[p] = _other(rng, int(kept[p])) if (int(kept[p]) & 0xDF) in b"ACGT" else kept[p]
    return np.concatenate([kept[:x], rng.choice(ACGT, size=ins), kept[x:]]).astype(np.uint8)


def _few(length: int) -> int:
    """Substitutions for a piece so that they are at most 13 letters apart."""
    return max(2, -(-(length - 1) // 13) + 1)


def _designs(rng):
    """[(label, start of B in the reference or None for a random place, len(B), function B -> A)]"""
    out = []
    for k in (31, 32, 33, 63, 64, 65, 66, 96, 97, 126, 127, 128):
        out.append(("del:%d" % k, None, k, lambda B, k=k: _middle(rng, B, 0, dele=k)))
        out.append(("ins:%d" % k, None, 0, lambda B, k=k: _middle(rng, B, 0, ins=k)))
    for length in (130, 200, 400):
        for d in (32, 33, 63, 64, 65, 96, 127, 128):
            out.append(("sub:%d/%d" % (d, length), None, length, lambda B, d=d: _middle(rng, B, d)))
    for d in (66, 97, 110, 115, 120, 125):  # (from 110 on: above 200 runs, the edits two letters apart and more)
        out.append(("sub:%d/400" % d, None, 400, lambda B, d=d: _middle(rng, B, d)))
    # an indel with scattered substitutions: 60 + 40, 100 + 27, 110 + 17, 110 + 18, and k - 6 letters + 6 substitutions for the limits and one more
    for k, nsub, rest in ((60, 40, 320), (100, 27, 324), (110, 17, 204), (110, 18, 216)):
        out.append(("del:%d+sub:%d" % (k, nsub), None, rest + k, lambda B, k=k, nsub=nsub: _middle(rng, B, nsub, dele=k)))
        out.append(("ins:%d+sub:%d" % (k, nsub), None, rest, lambda B, k=k, nsub=nsub: _middle(rng, B, nsub, ins=k)))
    for dist in (31, 32, 33, 63, 64, 65, 66, 96, 97, 127, 128):
        out.append(("del:%d+sub:6" % (dist - 6), None, dist - 6 + 61, lambda B, k=dist - 6: _middle(rng, B, 6, dele=k)))
        out.append(("ins:%d+sub:6" % (dist - 6), None, 61, lambda B, k=dist - 6: _middle(rng, B, 6, ins=k)))
    # a stretch replaced by random letters of nearly its length
    for dele, ins in ((50, 48), (100, 104), (140, 137)):
        out.append(("del:%d+ins:%d" % (dele, ins), None, dele + 40, lambda B, dele=dele, ins=ins: _middle(rng, B, 4, dele=dele, ins=ins)))
    # pieces at the borders of the 64-letter windows
    sizes = (63, 64, 65, 127, 128, 129)
    for a in sizes:
        for b in sizes:
            n = _few(min(a, b))
            out.append(("window:%d/%d" % (a, b), None, b, lambda B, a=a, b=b, n=n: _middle(rng, B, n, dele=max(0, b - a), ins=max(0, a - b))))
    # deletions inside the tandem repeats, as they stand and with substitutions in what the read keeps
    for name, (s, e) in (("A", HOMOPOLYMER), ("AC", AC_REPEAT), ("ACG", ACG_REPEAT)):
        for k in (40, 100):
            if name != "ACG":
                out.append(("repeat:%s-%d" % (name, k), s, e - s, lambda B, k=k: _middle(rng, B, 0, dele=k)))
            out.append(("repeat:%s-%d+sub" % (name, k), s, e - s, lambda B, k=k: _middle(rng, B, _few(len(B) - k), dele=k)))
    # a letter that is not A,C,G,T beyond the first 64 letters: of the read's piece, of the text's piece
    for length, at in ((150, 100), (300, 70), (300, 200)):
        def with_n(B, at=at):
            A = _middle(rng, B, _few(len(B)))
            A[at] = ord("N")
            return A
        out.append(("read-N:%d/%d" % (at, length), None, length, with_n))
    for p, at, length in zip(TEXT_N, (70, 130, 200), (150, 200, 300)):
        out.append(("text-N:%d/%d" % (at, length), p - at, length, lambda B: _middle(rng, B, _few(len(B)))))
    return out


_DEAR = set()  # labels of the catalogue (bulk() keeps their flanks)


def _assemble(ref: np.ndarray, rng, designs, flank: int = FLANK):
    reads, labels, pieces = [], [], []
    for label, start, blen, make in designs:
        if start is None:
            start = int(rng.integers(_FREE + FLANK, REF_LEN - FLANK - 500))
        f = FLANK if label in _DEAR else flank
        B = ref[start:start + blen]
        A = make(B)
        r = np.concatenate([ref[start - f:start], A, ref[start + blen:start + blen + f]]).astype(np.uint8)
        reads.append(ext_spec.revcomp(r) if len(reads) % 3 == 2 else r)
        labels.append(label)
        pieces.append((label, A.tobytes(), B.tobytes()))
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return q, off, labels, pieces


@functools.lru_cache(maxsize=None)
def _catalogue():
    rng = np.random.default_rng(4141)
    ref = reference()
    return (ref,) + _assemble(ref, rng, _designs(rng))


def catalogue():
    ref, q, off, labels, _ = _catalogue()
    return ref.copy(), q.copy(), off.copy(), list(labels)


def pieces():
    """[(label, A, B)] of the catalogue as designed, before any anchor is found."""
    return list(_catalogue()[4])


@functools.lru_cache(maxsize=None)
def _bulk():
    rng = np.random.default_rng(4142)
    ref = reference()
    designs = []
    for i in range(BULK_READS):
        k = 33 + int(rng.integers(0, 28))

        def one_more(B, k=k, dele=i % 2 == 0):
            A = np.concatenate([B[k:k + 8], [_other(rng, int(B[-1]))]]) if dele else \
                np.concatenate([rng.choice(ACGT, size=k), B[:8], [_other(rng, int(B[-1]))]])
            return A.astype(np.uint8)
        designs.append((("del:%d+sub:1" if i % 2 == 0 else "ins:%d+sub:1") % k, None, k + 9 if i % 2 == 0 else 9, one_more))
    rng_c = np.random.default_rng(4141)
    cat = _designs(rng_c)
    dear = [d for d in cat if d[0].startswith(("sub:", "del:100+", "ins:100+", "del:60+", "ins:60+", "window:129", "repeat:ACG"))][:40]
    step = len(designs) // len(dear)
    for j, d in enumerate(dear):  # spread through the batch
        designs.insert(j * (step + 1), d)
    _DEAR.update(d[0] for d in dear)
    return (ref,) + _assemble(ref, rng, designs, BULK_FLANK)


def bulk():
    ref, q, off, labels, _ = _bulk()
    return ref.copy(), q.copy(), off.copy(), list(labels)


# ---- what a run must have met ------------------------------------------------------------------------------------------------

def distance_within(A, B, limit: int):
    """The edit distance of two A,C,G,T pieces when it is at most limit, else None."""
    if not aln_spec.all_acgt(A) or not aln_spec.all_acgt(B) or abs(len(A) - len(B)) > limit:
        return None
    d = int(aln_spec.edit_matrix(A, B, band=limit)[len(A)][len(B)])
    return d if d <= limit else None


def _bad_beyond_64(x) -> bool:
    return not aln_spec.all_acgt(x[65:])


def assert_coverage(gaps, E: int) -> None:
    """gaps: aln_spec's gaps_out, (A, B, result of gap_ops), of the catalogue at the edit limit E."""
    closed = [(len(A), len(B), g) for A, B, g in gaps if g is not None]
    broken = [(A, B) for A, B, g in gaps if g is None]
    assert sum(g[1] == E for _, _, g in closed) >= 3
    assert sum(distance_within(A, B, E + 1) == E + 1 for A, B in broken) >= 3
    assert sum(_bad_beyond_64(A) or _bad_beyond_64(B) for A, B in broken) >= 2
    if E < 127:
        return
    for lo, hi in ((32, 63), (64, 95), (96, 127)):
        assert sum(lo <= g[1] <= hi for _, _, g in closed) >= 8, (lo, hi)
    assert sum(abs(a - b) >= 100 for a, b, _ in closed) >= 4
    assert sum(min(a, b) >= 300 for a, b, _ in closed) >= 4
    assert sum(a == 0 for a, b, _ in closed) >= 2 and sum(b == 0 for a, b, _ in closed) >= 2
    assert sum(len(aln_spec.runs(g[0])) > 200 for _, _, g in closed) >= 4


def listed_and_closed(gaps) -> int:
    """Closed gaps that k_aln_geom hands to k_aln_wave: |a - b| > 0 or more than two edits."""
    return sum(g is not None and (len(A) != len(B) or g[1] > 2) for A, B, g in gaps)
