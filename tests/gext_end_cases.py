"""Designed outer ends for -gext: a reference of 40 kb with planted features and reads of 200 letters whose
first or last letters hold what the end rule has to decide.  Every read is one label; tests/test_gpu_gext.py asserts from the
spec that the edges named here are really met."""
import numpy as np

import ext_spec

MIN_LEN = 20
READ = 200
REF_LEN = 40000
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
HOMO_AT, AC_AT, N_AT = 5000, 9000, 20000  # a run of 12 A, (AC) x 12, and one N (what a record border is in the merged text)


def reference(seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed)
    ref = rng.choice(ACGT, size=REF_LEN)
    ref[HOMO_AT:HOMO_AT + 12] = ord("A")
    ref[HOMO_AT - 1], ref[HOMO_AT + 12] = ord("C"), ord("G")
    ref[AC_AT:AC_AT + 24] = np.frombuffer(b"AC" * 12, dtype=np.uint8)
    ref[AC_AT - 1], ref[AC_AT + 24] = ord("G"), ord("T")
    ref[N_AT] = ord("N")
    return ref


def other(rng, c):
    return rng.choice(ACGT[ACGT != c])


def right_end(w, d: int, kind: str, L: int, rng, n: int = READ):
    """A read of n letters from the window w (at least n + L letters): an indel of L letters d letters in front of its end."""
    if kind == "D":
        return np.concatenate([w[:n - d], w[n - d + L:n + L]])
    ins = np.array([other(rng, w[n - d - L])] + [rng.choice(ACGT) for _ in range(L - 1)], dtype=np.uint8)
    return np.concatenate([w[:n - d - L], ins, w[n - d - L:n - L]])


def catalogue(Z: int = 8, seed: int = 5):
    """(reference, reads, offsets, labels).  Sizes Z and Z + 1 follow the band."""
    rng = np.random.default_rng(seed + 1)
    ref = reference(seed)
    reads, labels = [], []

    def add(label, r):
        assert len(r) > 0
        reads.append(np.asarray(r, dtype=np.uint8))
        labels.append(label)

    def window(at, n=READ + 40):
        return ref[at:at + n].copy()
    at = 100
    for kind in "ID":
        for L in (1, 2, Z, Z + 1):
            for d in (1, 5, 12, 19, 25):
                if kind == "I" and d + L > READ - 40:
                    continue
                at += 211
                w = window(at)
                add(f"right:{kind}{L}@{d}", right_end(w, d, kind, L, rng))
                at += 211
                w = window(at)[::-1].copy()  # the mirror image: the indel d letters behind the read's start
                add(f"left:{kind}{L}@{d}", right_end(w, d, kind, L, rng)[::-1])
    # a deleted A inside the run of A, a deleted AC inside (AC)n.  Inside a repeat the diagonal behind the deletion matches back to
    # the repeat's start, so a substitution keeps that stretch under 20 letters (no second MEM): the end is X or =, the D, the tail
    for label, pos, L, d, sub in (("homopolymer", HOMO_AT + 6, 1, 25, 12), ("repeat:AC", AC_AT + 6, 2, 28, 10)):
        start = pos + d - READ
        r = right_end(ref[start:start + READ + 40].copy(), d, "D", L, rng)
        r[READ - d + sub] = other(rng, r[READ - d + sub])
        add(label + ":D", r)
        w = ref[pos + L - d - 40:pos + L - d + READ][::-1].copy()
        r = right_end(w, d, "D", L, rng)
        r[READ - d + sub] = other(rng, r[READ - d + sub])
        add(label + ":D:left", r[::-1])
    # an indel and a mismatch; an N in the read's tail
    r = right_end(window(30000), 19, "D", 1, rng)
    r[READ - 8] = other(rng, r[READ - 8])
    add("D1@19+sub@8", r)
    r = right_end(window(30300), 25, "I", 2, rng)
    r[READ - 6] = other(rng, r[READ - 6])
    add("I2@25+sub@6", r)
    r = right_end(window(30600), 23, "D", 1, rng)
    r[READ - 5] = ord("N")
    add("D1@23+N@5", r)
    # the text's first and last letter and the N between records clamp B
    add("text-start", right_end(np.concatenate([ref[:READ - 2][::-1], ACGT[:2], ACGT[:40]]), 12, "I", 2, rng)[::-1])
    add("text-end", right_end(np.concatenate([ref[REF_LEN - READ + 2:], ACGT[:2], ACGT[:40]]), 12, "I", 2, rng))
    add("record-border", right_end(np.concatenate([ref[N_AT - READ + 2:N_AT], ACGT[:2], ACGT[:40]]), 12, "I", 2, rng))
    add("record-border:left", right_end(np.concatenate([ref[N_AT + 1:N_AT + READ - 1][::-1], ACGT[:2], ACGT[:40]]), 12, "I", 2, rng)[::-1])
    # an inserted letter 8 from the end: the gapped end scores 8 - (o + e) = 0 at costs 4,6,2, as the empty ungapped side does
    for k in range(4):
        add(f"tie:{k}", right_end(window(31000 + 300 * k), 8, "I", 1, rng))
    # tails without a MEM of 20 letters: a deleted letter, then a substitution every 15 letters
    for n in (63, 64, 65, 127, 128, 129):
        r = right_end(window(33000 + 250 * (n % 7) + n), n, "D", 1, rng)
        for x in range(READ - n + 14, READ - 5, 15):  # (the last one has five letters behind it: the tail runs to the read's end)
            r[x] = other(rng, r[x])
        add(f"tail:{n}", r)
    # indels of Z and Z + 1 letters in front of a tail of 70 letters with a substitution every 15: found when the drop and the costs
    # allow a gap of Z letters (they do not at the defaults), the band refuses Z + 1
    for kind in "DI":
        for L in (Z, Z + 1):
            r = right_end(window(36000 + 300 * len(reads) % 3000, READ + 80), 70, kind, L, rng)
            for x in range(READ - 70 + 14, READ - 5, 15):
                r[x] = other(rng, r[x])
            add(f"tail70:{kind}{L}", r)
    # one long record whose end passes Cp: a deleted letter, then a substitution every 20 letters for 2,900 letters
    w = ref[35000:35000 + 3040].copy()
    r = right_end(w, 2900, "D", 1, rng, n=3000)
    for x in range(3000 - 2900 + 19, 3000, 20):
        r[x] = other(rng, r[x])
    add("long:past-Cp", r)
    # every third read from the other strand
    for i in range(0, len(reads), 3):
        reads[i] = ext_spec.revcomp(reads[i])
        labels[i] += ":rc"
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return ref, np.concatenate(reads), off, labels


def bulk(n: int = 400, seed: int = 9):
    """n reads with a deleted letter 12 letters in front of the end: a listed end each."""
    rng = np.random.default_rng(seed)
    ref = reference()
    reads = []
    for _ in range(n):
        at = int(rng.integers(0, N_AT - READ - 50))
        if HOMO_AT - READ - 50 < at < AC_AT + 50:
            at = AC_AT + 100 + at % 1000
        reads.append(right_end(ref[at:at + READ + 40].copy(), 12, "D", 1, rng))
    off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(READ))
    return ref, np.concatenate(reads), off
