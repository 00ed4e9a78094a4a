"""-chain without a GPU: the option and its maximum gap as the front end parses them, the refused combinations, and the
definition the GPU tests check against (tests/chain_spec.py) -- the dynamic programme against exhaustive enumeration of every
valid chain, the bounds and monotonicity DESIGN.md 4.12 states, on random blocks, on random text/query pairs of both strands
and on the golden -mem files the real reference wrote."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chain_spec
import hostlib
import mum_spec
from golden_cases import CASES, MANIFEST, case_paths
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]


# ---- options ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [
    ["-chain", "ref.fa", "q.fa"],
    ["-b", "-chain", "-l", "20", "ref.fa", "q.fa"],
    ["-l", "20", "ref.fa", "q.fa", "-chain"],
    ["ref.fa", "-chain", "q.fa"],
    ["-CHAIN", "ref.fa", "q.fa"],
], ids=["first", "middle", "last", "between-files", "upper-case"])
def test_chain_sets_match_type_4_anywhere(args):
    o = hostlib.parse_options(["slaMEM"] + args)
    assert o["match_type"] == 4
    assert o["files"] == ["ref.fa", "q.fa"]  # never taken as a file, and it takes no value
    assert not o["hidden_clean"]             # only the exact -c is the clean tool


@pytest.mark.parametrize("args", [
    ["-chain", "-mam", "x", "ref.fa", "q.fa"],
    ["-mum", "x", "-chain", "ref.fa", "q.fa"],
    ["-chain", "ref.fa", "q.fa", "-smem"],
    ["-smem", "-chain", "ref.fa", "q.fa"],
])
def test_chain_with_another_mode_is_match_type_minus_1(args):
    assert hostlib.parse_options(["slaMEM"] + args)["match_type"] == -1


def test_other_options_unchanged():
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa"])["match_type"] == 0
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa", "-mam"])["match_type"] == 1
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa", "-mum"])["match_type"] == 2
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa", "-smem"])["match_type"] == 3
    o = hostlib.parse_options(["slaMEM", "-m", "50", "ref.fa", "q.fa"])
    assert (o["match_type"], o["min_seq_len"], o["files"]) == (0, 50, ["ref.fa", "q.fa"])
    o = hostlib.parse_options(["slaMEM", "-chain", "-mgap", "70", "-m", "50", "-b", "-o", "out.txt", "ref.fa", "q.fa"])
    assert (o["match_type"], o["min_seq_len"], o["both_strands"], o["files"]) == (4, 50, 1, ["ref.fa", "q.fa"])
    assert o["out_arg"] == 8
    assert hostlib.parse_options(["slaMEM", "-c", "x.fa"])["hidden_clean"]


def parse_max_gap(args):
    L = hostlib.lib()
    L.slh_parse_max_gap.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
    argv = (C.c_char_p * (len(args) + 2))(b"slaMEM", *[a.encode() for a in args], None)
    out = C.c_int(-7)
    rc = L.slh_parse_max_gap(len(args) + 1, argv, C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("args,expect", [
    (["-chain", "ref.fa", "q.fa"], (0, 0)),
    (["-chain", "-mgap", "50", "ref.fa", "q.fa"], (1, 50)),
    (["-chain", "ref.fa", "q.fa", "-mgap", "1"], (1, 1)),
    (["-MGAP", "2147483647", "-chain", "ref.fa", "q.fa"], (1, 2147483647)),
    (["-chain", "-mgap", "2147483648", "ref.fa", "q.fa"], (-1, 0)),
    (["-chain", "-mgap", "0", "ref.fa", "q.fa"], (-1, 0)),
    (["-chain", "-mgap", "-3", "ref.fa", "q.fa"], (-1, 0)),
    (["-chain", "-mgap", "wide", "ref.fa", "q.fa"], (-1, 0)),
    (["-chain", "-mgap", "3x", "ref.fa", "q.fa"], (-1, 0)),
    (["-chain", "ref.fa", "q.fa", "-mgap"], (-1, 0)),
    (["-chain", "-m", "50", "-mam", "ref.fa", "q.fa"], (0, 0)),
])
def test_mgap_values_and_errors(args, expect):
    assert parse_max_gap(args) == expect


def test_mgap_value_is_not_a_file():
    o = hostlib.parse_options(["slaMEM", "-chain", "-mgap", "40", "ref.fa", "q.fa"])
    assert o["files"] == ["ref.fa", "q.fa"] and o["match_type"] == 4 and o["min_seq_len"] == 0


@pytest.mark.parametrize("args,message", [
    (["-mgap", "3"], b"> ERROR: Option -mgap needs -chain"),
    (["-smem", "-mgap", "3"], b"> ERROR: Option -mgap needs -chain"),
    (["-chain", "-mgap", "0"], b"> ERROR: Option -mgap needs a whole number of at least 1"),
    (["-chain", "-mgap", "wide"], b"> ERROR: Option -mgap needs a whole number of at least 1"),
    (["-chain", "-mam", "x"], b"> ERROR: Option -chain excludes -mam, -mum and -smem"),
    (["-mum", "x", "-chain"], b"> ERROR: Option -chain excludes -mam, -mum and -smem"),
    (["-smem", "-chain"], b"> ERROR: Option -chain excludes -mam, -mum and -smem"),
])
def test_refused_combinations_exit_255_before_any_work(args, message, tmp_path):
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + args + ["-o", str(out), ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60)
    assert r.returncode == 255
    assert message in r.stdout
    assert not out.exists()


def test_usage_lists_chain_and_mgap():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"\t-chain\t" in r.stdout and b"\t-mgap\t" in r.stdout


# ---- the definition ---------------------------------------------------------------------------------------------------------

def test_worked_example():
    """A read of 100 letters against a reference with one deleted letter, G = 50.  Rows in the emission order (q descending):

        index  (p,    q,  L)    diagonal p - q
        0      (161,  60, 40)   101     the part behind the indel
        1      (9060, 60, 12)   9000    a repeat copy far away: p differs by more than G from every other row
        2      (130,  30, 30)   100     the part before the indel ...
        3      (100,   0, 30)   100     ... in two pieces (a mismatch at letter 30 would split it so; here they abut)

    3 -> 2: link = min(30, 60 - 30, 160 - 130) - 0 = 30, f(2) = 60.  2 -> 0: min(40, 100 - 60, 201 - 160) - |101 - 100| = 39,
    f(0) = 99.  3 -> 0 directly would give 30 + 39 = 69.  Row 1 has no predecessor and precedes nothing (G): f(1) = 12."""
    rows = np.array([(161, 60, 40), (9060, 60, 12), (130, 30, 30), (100, 0, 30)])
    assert chain_spec.in_emission_order(rows)
    f, pred = chain_spec.chain_dp(rows, 50)
    assert f == [99, 12, 60, 30] and pred == [2, -1, 3, -1]
    keep, score = chain_spec.block_chain(rows, 50)
    assert list(keep) == [True, False, True, True] and score == 99
    assert chain_spec.kept_score(rows[keep], 50) == 99
    # a gap that admits the copy changes nothing: it lies in front in the query but behind in the reference of no row
    assert chain_spec.chain_dp(rows, 10000)[0] == [99, 12, 60, 30]
    # G = 29: no row may precede another (every query start differs by 30 or more): the longest row alone
    keep, score = chain_spec.block_chain(rows, 30 - 1)
    assert chain_spec.chain_dp(rows, 29)[1] == [-1, -1, -1, -1] and score == 40 and list(keep) == [True, False, False, False]
    # a tie: two rows one diagonal step to either side give row 0 the same value -- the smaller index wins; two ends of
    # equal f -- the smaller index
    tie = np.array([(200, 100, 10), (149, 50, 10), (151, 50, 10)])
    f, pred = chain_spec.chain_dp(tie, 100)
    assert f == [19, 10, 10] and pred == [1, -1, -1]
    assert chain_spec.chain_dp(tie[[0, 2, 1]], 100) == ([19, 10, 10], [1, -1, -1])
    ends = np.array([(500, 100, 10), (700, 50, 10)])
    assert list(chain_spec.block_chain(ends, 100)[0]) == [True, False]
    # a predecessor that gives exactly L_i is not taken
    same = np.array([(120, 20, 10), (100, 10, 10)])  # link = 10 - 10 = 0: f = 10 + 0 = L
    assert chain_spec.chain_dp(same, 100) == ([10, 10], [-1, -1])


def _all_chains(rows, gap):
    """Every valid chain as a tuple of indices, by depth-first extension."""
    n = len(rows)
    ok = [[chain_spec.may_precede(rows[j], rows[i], gap) for i in range(n)] for j in range(n)]
    out = []

    def extend(chain):
        out.append(tuple(chain))
        for i in range(n):
            if ok[chain[-1]][i]:
                extend(chain + [i])

    for s in range(n):
        extend([s])
    return out


def _score(rows, chain):
    return int(rows[chain[0]][2]) + sum(chain_spec.link(rows[a], rows[b]) for a, b in zip(chain, chain[1:]))


def _random_block(rng, n):
    """Rows on a few diagonals near each other with small coordinates, so that links, ties and gap limits all occur."""
    base = int(rng.integers(0, 50))
    rows = []
    for _ in range(n):
        q = int(rng.integers(0, 40))
        d = base + int(rng.choice([0, 0, 0, 1, 2, -1, 30]))
        p = max(0, q + d)
        rows.append((p, q, int(rng.integers(1, 12))))
    if n >= 3 and rng.integers(0, 2):  # a planted tie: a copy of a row one diagonal step aside
        p, q, ln = rows[0]
        rows[1] = (p + 1, q, ln)
    rows.sort(key=lambda r: (-r[1], -r[2]))
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


@pytest.mark.parametrize("seed", range(4))
def test_dp_against_exhaustive_enumeration(seed):
    rng = np.random.default_rng(7100 + seed)
    multi = ties = 0
    for _ in range(150):
        n = int(rng.integers(1, 10))
        rows = _random_block(rng, n)
        gap = int(rng.choice([3, 8, 20, 5000]))
        chains = _all_chains(rows, gap)
        f, pred = chain_spec.chain_dp(rows, gap)
        # f(i) is the best score over all chains that end in i
        for i in range(n):
            assert f[i] == max(_score(rows, c) for c in chains if c[-1] == i), (rows, gap, i)
        best = max(_score(rows, c) for c in chains)
        keep, score = chain_spec.block_chain(rows, gap)
        assert score == best, (rows, gap)
        kept = [i for i in range(n) if keep[i]]
        chain = tuple(reversed(kept))  # (the block is q descending; a chain ascends)
        assert chain in chains and _score(rows, chain) == best, (rows, gap)
        # the tie-breaks: the end is the smallest index of the largest f; each predecessor is the smallest index that
        # reaches f, and there is none when no chain beats L_i
        assert chain[-1] == min(i for i in range(n) if f[i] == best)
        for i in range(n):
            cands = [j for j in range(n) if chain_spec.may_precede(rows[j], rows[i], gap)
                     and f[j] + chain_spec.link(rows[j], rows[i]) == f[i]]
            assert pred[i] == (min(cands) if f[i] > rows[i][2] else -1), (rows, gap, i)
            ties += len(cands) > 1 and f[i] > rows[i][2]
        for a, b in zip(chain, chain[1:]):
            assert pred[b] == a
        assert pred[chain[0]] == -1
        multi += len(chain) > 1
        # the windowed evaluation the large cases use gives the same values
        assert chain_spec.chain_dp_windowed(rows, gap) == (f, pred), (rows, gap)
    assert multi > 30 and ties > 0


def _check_block(rows, gap):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    f, pred = chain_spec.chain_dp_windowed(rows, gap) if len(rows) > 200 else chain_spec.chain_dp(rows, gap)
    for (p, q, ln), fi in zip(rows, f):
        assert ln <= fi <= q + ln
    keep, score = chain_spec.block_chain(rows, gap, windowed=len(rows) > 200)
    k = rows[keep][::-1]  # ascending
    if len(rows) == 0:
        assert score == 0
        return 0, 0
    assert len(k) >= 1
    for col in (k[:, 1], k[:, 0], k[:, 1] + k[:, 2], k[:, 0] + k[:, 2]):
        assert np.all(np.diff(col) > 0)
    assert chain_spec.kept_score(rows[keep], gap) == score
    return len(rows) - len(k), int(len(k) > 1)


def _rows(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


@pytest.mark.parametrize("seed", range(3))
def test_properties_on_random_pairs(seed):
    rng = np.random.default_rng(7300 + seed)
    dropped = multi = 0
    for _ in range(60):
        alpha = np.frombuffer(b"ACGT"[: int(rng.integers(2, 5))], dtype=np.uint8)
        text = rng.choice(alpha, size=int(rng.integers(20, 200))).tobytes()
        a = int(rng.integers(0, len(text) - 10))
        piece = bytearray(text[a:a + int(rng.integers(10, 80))])
        if len(piece) > 6:  # an indel and a substitution
            del piece[int(rng.integers(1, len(piece) - 1))]
            piece[int(rng.integers(0, len(piece)))] = int(rng.choice(alpha))
        q = bytes(piece) + rng.choice(alpha, size=int(rng.integers(0, 10))).tobytes()
        o = po.OracleIndex(text)
        min_len = int(rng.integers(1, 6))
        for strand in (q, po.reverse_complement(q)):
            rows = _rows(o.get_matches(strand, min_len))
            assert chain_spec.in_emission_order(rows)
            for gap in (5, 5000):
                d, m = _check_block(rows, gap)
                dropped += d
                multi += m
    assert dropped and multi


@pytest.mark.parametrize("case", MEM_CASES)
def test_properties_on_golden_files(case):
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    blocks = mum_spec.parse_mems_file(open(exp_mems, "rb").read(), ref)
    for _, rows in blocks:
        assert chain_spec.in_emission_order(rows)
        _check_block(rows, chain_spec.DEFAULT_GAP)
        if len(rows) <= 400:
            _check_block(rows, 50)


def test_golden_cases_include_blocks_that_lose_rows_and_chains_of_several_rows():
    lose = multi = 0
    kept_of = {}
    for case in MEM_CASES:
        plain = open(case_paths(case)[2], "rb").read()
        data, kept, scores, _, _, _ = chain_spec.golden_chain_file(case)
        lose += data != plain
        multi += any(len(k) > 1 for k in kept)
        kept_of[case] = sum(len(k) for k in kept)
        assert len(scores) == len(kept)
    assert len(MEM_CASES) == 17
    assert lose >= 10 and multi >= 15
    assert (kept_of["ac_l10_both"], kept_of["acgt_l20_both"], kept_of["long_repeat_l20"], kept_of["acgt_l1_fwd"],
            kept_of["long_single_query"]) == (11, 19, 13, 3, 33)
