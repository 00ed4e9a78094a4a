"""K8s (k_seed_mems) on designed reads: one compare per (read, strand, diagonal) reports every MEM on the diagonal, and the first
round looks up only a few windows of a read.  Every case asks one thing: the rows of the seed path equal the rows of the
index walk (SLAMEM_SEED_SEARCH=0), row for row, in order, block counts included -- and the oracle's.  The texts are random
letters, 270 k of them: the smallest for which the index takes seeds of 12 letters (2^18 < n <= 2^19).
The inputs are built so that the things the kernel could lose are there: runs of l - 1, l and l + 1 letters that hold no
first-round window, reads none of whose first-round windows is free of errors, copies of a locus (next to each other too),
diagonals that start before the text and end behind it, palindromic windows, one strand asked for, lists that run over, the
last wave partly filled, every plane-word count."""
import numpy as np
import pytest

from test_gpu_seed import ACGT, eng, mutate, normalised, pack, rc, seed_stats  # noqa: F401  (eng: the module's fixture)

pytestmark = pytest.mark.gpu

K = 12  # seed letters for these texts (asserted against the index)
STEPS = ("1", "2", "3", "4", "6", "")


def other_letter(c):
    return ACGT[(int(np.where(ACGT == c)[0][0]) + 1) % 4]


def cut(t, x, length, agree):
    """The `length` text letters from x on, every letter outside the intervals `agree` (read offsets [a, b)) substituted."""
    r = t[x:x + length].copy()
    keep = np.zeros(length, dtype=bool)
    for a, b in agree:
        assert 0 <= a < b <= length
        keep[a:b] = True
    for i in np.where(~keep)[0]:
        r[i] = other_letter(r[i])
    return r


def codes(a, k):
    """The k-mers of a as integers (2 bits a letter)."""
    c = np.searchsorted(ACGT, a).astype(np.int64)
    out = np.zeros(len(a) - k + 1, dtype=np.int64)
    for i in range(k):
        out = out * 4 + c[i:len(a) - k + 1 + i]
    return out


_sorted = {}  # the sorted k-mers of the text looked at last


def diagonals_with_a_kmer(t, r, k):
    """(strand, diagonal) of every k letters that the read (either strand) shares with the text: brute force."""
    if _sorted.get("text") is not t:
        tc = codes(t, k)
        order = np.argsort(tc, kind="stable")
        _sorted.update(text=t, order=order, ts=tc[order])
    order, ts = _sorted["order"], _sorted["ts"]
    out = set()
    for st, x in ((0, r), (1, rc(r))):
        xc = codes(x, k)
        lo, hi = np.searchsorted(ts, xc, "left"), np.searchsorted(ts, xc, "right")
        for o in np.where(hi > lo)[0]:
            for p in order[lo[o]:hi[o]]:
                out.add((st, int(p) - int(o)))
    return out


def rows(g, q, off, l, both):
    gm, goff = g.find_mems(q, off, l, both)
    return gm, np.diff(goff.astype(np.int64))


def agree(eng, t, qs, l, both=True, oracle=True, steps=("",), monkeypatch=None):
    """The seed path's rows == the walk's == the oracle's, for every first-round stride asked for; the counters per stride
    (and under "rows" the rows themselves with their block counts, a block per strand)."""
    from conftest import search_path
    text = t.tobytes()
    q, off = pack(qs)
    g = eng.Index.build(text)
    out = {}
    try:
        assert int(g.info.seed_k) == K and l >= K + 2
        with search_path("walk"):
            wm, wbc = rows(g, q, off, l, both)
        if oracle:
            from oracle import pyoracle as po
            om, obc = po.OracleIndex(text).match_batch(pack([normalised(x) for x in qs])[0], off, l, both)
            assert np.array_equal(wbc, obc.astype(np.int64))
            for f in ("ref_pos", "query_pos", "length"):
                assert np.array_equal(wm[f], om[f]), f
        for step in steps:
            if monkeypatch is not None:
                if step:
                    monkeypatch.setenv("SLAMEM_SEED_STEP", step)
                else:
                    monkeypatch.delenv("SLAMEM_SEED_STEP", raising=False)
            with search_path("seed"):
                sm, sbc = rows(g, q, off, l, both)
                assert np.array_equal(sbc, wbc), step
                for f in ("ref_pos", "query_pos", "length"):
                    assert np.array_equal(sm[f], wm[f]), (step, f)
                st = seed_stats(eng, g, q, off, l, both)
            assert st["seed_reads"] == len(qs) and st["mems"] == len(wm), step
            out[step] = st
        out["rows"] = (wm, wbc)
    finally:
        if monkeypatch is not None:
            monkeypatch.delenv("SLAMEM_SEED_STEP", raising=False)
        g.close()
    return out


def lone_windows(l, length):
    """Window numbers that no first round looks up, whatever its stride (2 .. 9, and the default, which is larger)."""
    s = l - K + 1
    nwin = (length - K) // s + 1
    return [w for w in range(1, nwin - 2) if all(w % m for m in range(2, 10))]


def threshold_reads(rng, t, l, count, length=150):
    """Reads of one locus each: two short runs (l - 1, l, l + 1, k .. l - 1 letters) that hold exactly one window, a window no
    first round looks up, and one long run; every other letter substituted."""
    s = l - K + 1
    lone = lone_windows(l, length)
    kinds = [l - 1, l, l + 1] + list(range(K, l))
    qs, n_mems = [], 0
    for i in range(count):
        w1, w2 = lone[0], lone[-1]
        r1, r2 = kinds[i % len(kinds)], kinds[(i // len(kinds) + i + 1) % len(kinds)]
        iv = []
        for w, r in ((w1, r1), (w2, r2)):
            a = w * s - (1 if r > K else 0)  # the run holds the window at w * s and no other
            assert a >= 0 and a + r <= length and (a + r - K) // s == w and (a + s - 1) // s == w
            iv.append((a, a + r))
        assert iv[0][1] + 2 + 2 * l < iv[1][0]
        iv.append((iv[0][1] + 1, iv[1][0] - 1))  # the long run between them
        for _ in range(3000):  # (most of the time a 12-mer of the read lies somewhere else in the text too)
            x = int(rng.integers(0, len(t) - length))
            r = cut(t, x, length, iv)
            if len(diagonals_with_a_kmer(t, r, K)) == 1:
                break
        n_mems += sum(1 for a, b in iv if b - a >= l)
        qs.append(rc(r) if i % 2 else r)
    return qs, n_mems


def random_text(seed, n=270_000):
    rng = np.random.default_rng(seed)
    return rng, rng.choice(ACGT, size=n)


@pytest.mark.parametrize("l", [K + 3, 20])
def test_runs_beside_the_threshold_on_one_diagonal(eng, l):
    rng, t = random_text(700 + l)
    qs, n_mems = threshold_reads(rng, t, l, 64)
    for r in qs:  # (no GPU yet) one diagonal with k letters in common, on one strand
        assert len(diagonals_with_a_kmer(t, r, K)) == 1
    st = agree(eng, t, qs, l)[""]
    assert st["mems"] == n_mems
    assert st["seed_compares"] == st["seed_reads"] == len(qs), st
    assert st["seed_strands_left"] == 0, st["seed_left_why"]


def test_no_first_round_window_survives(eng, monkeypatch):
    """A read per stride m: a substitution in every window whose number is a multiple of m, so that with that stride (and its
    multiples: the default for 150 letters is 6 windows at l = 20, 12 at l = k + 3) no first-round window of the read is
    free of errors.  l = 20 (windows 9 letters apart, letters 3 .. 8 of a window lie in no other): the substitutions leave runs
    of 22 letters (m = 2: at letter 3 and letter 8 of the windows in turn) or more; l = k + 3: of 15 letters and more from m = 4."""
    rng, t = random_text(811)
    length = 150
    qs = []
    s = 20 - K + 1
    nwin = (length - K) // s + 1
    for m in (2, 3, 4, 6):
        for _ in range(9):
            x = int(rng.integers(0, len(t) - length))
            r = t[x:x + length].copy()
            for w in range(0, nwin, m):
                at = w * s + (4 if m > 2 else 3 if (w // 2) % 2 == 0 else 8)
                r[at] = other_letter(r[at])
            qs.append(r if len(qs) % 2 else rc(r))
    st = agree(eng, t, qs, 20, steps=STEPS, monkeypatch=monkeypatch)
    assert st[""]["mems"] >= len(qs)
    l = K + 3
    s = l - K + 1
    nwin = (length - K) // s + 1
    qs = []
    for m in (2, 3, 4, 6, 12):  # (12: the default stride for 35 windows, three probes)
        for _ in range(9):
            x = int(rng.integers(0, len(t) - length))
            r = t[x:x + length].copy()
            for w in range(0, nwin, m):
                r[w * s] = other_letter(r[w * s])
            qs.append(r if len(qs) % 2 else rc(r))
    st = agree(eng, t, qs, l, steps=STEPS, monkeypatch=monkeypatch)
    assert st[""]["mems"] > 0


def copies_text(seed):
    """Two and three copies of a locus, exact and 1 % diverged, and a locus repeated 130 letters behind itself."""
    rng, t = random_text(seed)
    loci = []
    for copies, div, at in [(2, 0.0, 2_000), (3, 0.0, 8_000), (2, 0.01, 16_000), (3, 0.01, 22_000)]:
        seg = t[at:at + 400].copy()
        spots = [at]
        for c in range(1, copies):
            y = at + 1_500 * c
            t[y:y + 400] = mutate(rng, seg, div) if div else seg
            spots.append(y)
        loci += spots
    seg = t[40_000:40_100].copy()  # neighbouring diagonals: the copies lie 130 and 260 letters apart
    t[40_130:40_230] = seg
    t[40_260:40_360] = mutate(rng, seg, 0.01)
    return rng, t, loci


def copies_reads(rng, t, loci):
    qs = []
    for y in loci:
        for o in (0, 37, 250):
            r = mutate(rng, t[y + o:y + o + 150], 0.02)
            qs += [r, rc(t[y + o:y + o + 150])]
    for o in range(39_960, 40_240, 20):
        qs += [t[o:o + 150].copy(), rc(mutate(rng, t[o:o + 150], 0.02))]
    return qs


@pytest.mark.parametrize("l", [K + 3, 20])
def test_two_and_three_copies_of_the_locus(eng, l):
    rng, t, loci = copies_text(900 + l)
    qs = copies_reads(rng, t, loci)
    out = agree(eng, t, qs, l)
    assert out[""]["seed_mems"] > 0
    # every diagonal once: an unchanged read of an exact locus has one full-length row per copy (the five exact spots come
    # first in `loci`: two of one locus, three of another; three reads a spot, the unchanged one second of each pair)
    wm, wbc = out["rows"]
    ends = np.cumsum(wbc)
    for spot in range(5):
        for o in range(3):
            i = (spot * 3 + o) * 2 + 1
            mine = wm["length"][ends[2 * i] - wbc[2 * i]:ends[2 * i + 1]]
            assert int((mine == 150).sum()) == (2 if spot < 2 else 3), (spot, o)


@pytest.mark.parametrize("l", [K + 3, 20])
def test_diagonals_at_the_ends_of_the_text(eng, l):
    rng, t = random_text(1000 + l)
    n = len(t)
    qs = []
    for over in (1, 7, l - 1, 40, 150 - l, 150 - l + 1):
        junk = rng.choice(ACGT, size=over)
        head = np.concatenate([junk, t[:150 - over]])            # d = -over
        tail = np.concatenate([t[n - (150 - over):], junk])      # d + 150 = n + over
        qs += [head, rc(head), tail, rc(tail), mutate(rng, head, 0.03), rc(mutate(rng, tail, 0.03))]
    agree(eng, t, qs, l)


@pytest.mark.parametrize("both", [True, False])
def test_reverse_strand_reads_and_palindromic_windows(eng, both):
    rng, t = random_text(1100)
    spots = [int(x) for x in rng.integers(500, len(t) - 500, size=24)]
    for i, x in enumerate(spots):  # eight palindromes of 12 letters, three copies each
        half = np.random.default_rng(300 + i // 3).choice(ACGT, size=6)
        t[x:x + 12] = np.concatenate([half, rc(half)])
    for l in (K + 3, 20):
        s = l - K + 1
        qs = []
        for x in spots:
            for w in (0, 1, 6):  # the palindrome on a window of the read, looked up in the first round or not
                r = t[x - s * w:x - s * w + 150].copy()
                qs += [r, rc(mutate(rng, r, 0.02))]
        for i in range(60):  # half the reads from the other strand
            x = int(rng.integers(0, len(t) - 150))
            r = mutate(rng, t[x:x + 150], 0.02)
            qs.append(rc(r) if i % 2 else r)
        st = agree(eng, t, qs, l, both=both)[""]
        assert st["seed_left_why"][2] > 0 or not both, st  # (palindromic windows were compared on both strands)


@pytest.mark.parametrize("l", [K + 3, 20])
def test_strides_agree_and_look_up_less(eng, l, monkeypatch):
    rng, t, loci = copies_text(1200 + l)
    qs = copies_reads(rng, t, loci) + threshold_reads(rng, t, l, 40)[0]
    st = agree(eng, t, qs, l, steps=STEPS, monkeypatch=monkeypatch)
    for step in ("2", "3", "4", "6", ""):
        assert st[step]["seed_windows"] < st["1"]["seed_windows"], (step, st[step]["seed_windows"], st["1"]["seed_windows"])


def test_lists_that_run_over_leave_their_reads_to_the_walk(eng):
    rng, t = random_text(1300)
    seg = t[1_000:1_200].copy()
    for c in range(1, 12):  # a family of twelve exact copies
        t[1_000 + 4_000 * c:1_200 + 4_000 * c] = seg
    qs = [(t[1_000 + 4_000 * (i % 12) + i:1_150 + 4_000 * (i % 12) + i]).copy() for i in range(21)]  # the first wave
    for i in range(63):
        x = int(rng.integers(49_000, len(t) - 150))
        r = mutate(rng, t[x:x + 150], 0.02)
        qs.append(rc(r) if i % 2 else r)
    st = agree(eng, t, qs, 20)[""]
    why = st["seed_left_why"]
    assert why[3] > 0 or why[5] > 0, why
    assert 0 < st["seed_strands_left"] <= 2 * 21, st  # (the other waves' reads stay)


@pytest.mark.parametrize("l", [K + 3, 20])
@pytest.mark.parametrize("count", [20, 21, 22, 43])
def test_wave_edges(eng, count, l):
    rng, t = random_text(1400 + count)
    lengths = [l, 63, 64, 65, 127, 128, 129, 191, 192, 150]
    qs = []
    for i in range(count):
        n = lengths[i % len(lengths)]
        x = int(rng.integers(0, len(t) - n))
        r = mutate(rng, t[x:x + n], 0.02 if n > l else 0.0)
        qs.append(rc(r) if i % 3 == 0 else r)
    agree(eng, t, qs, l)


@pytest.mark.parametrize("length,l", [(250, 20), (250, K + 3), (380, 20), (380, 30)])
def test_four_and_six_plane_words(eng, length, l):
    rng, t = random_text(1500 + length + l)
    qs = []
    for i in range(40):
        x = int(rng.integers(0, len(t) - length))
        r = mutate(rng, t[x:x + length], 0.02)
        qs.append(rc(r) if i % 2 else r)
    head = np.concatenate([rng.choice(ACGT, size=30), t[:length - 30]])
    qs += [head, rc(head)]
    agree(eng, t, qs, l)


def test_a_read_with_an_n_on_a_text_without_one(eng):
    rng, t = random_text(1600)
    qs = []
    for i in range(43):
        x = int(rng.integers(0, len(t) - 150))
        r = mutate(rng, t[x:x + 150], 0.02)
        if i % 4 == 0:
            r[[5, 77, 149][i % 3]] = ord("N")
        if i % 8 == 0:
            r[60:63] = ord("n")
        qs.append(rc(r) if i % 2 else r)
    for l in (K + 3, 20):
        st = agree(eng, t, qs, l)[""]
        assert st["seed_strands_left"] == 0 and st["seed_left_why"][0] == 0, st["seed_left_why"]
