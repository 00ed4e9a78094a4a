"""-smem without a GPU: the option and its occurrence cap as the front end parses them, the refused combinations, and the
definition the GPU tests check against (tests/smem_spec.py) -- the emission order every block is in, the super-maximal
filter against claim 1 of DESIGN.md 4.11 and the run lengths against claim 2, both by naive substring search, on random
text/query pairs of both strands and on the golden -mem files the real reference wrote."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostlib
import mum_spec
import smem_spec
from golden_cases import CASES, MANIFEST, case_paths
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]


# ---- options ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [
    ["-smem", "ref.fa", "q.fa"],
    ["-b", "-smem", "-l", "20", "ref.fa", "q.fa"],
    ["-l", "20", "ref.fa", "q.fa", "-smem"],
    ["ref.fa", "-smem", "q.fa"],
    ["-SMEM", "ref.fa", "q.fa"],
], ids=["first", "middle", "last", "between-files", "upper-case"])
def test_smem_sets_match_type_3_anywhere(args):
    o = hostlib.parse_options(["slaMEM"] + args)
    assert o["match_type"] == 3
    assert o["files"] == ["ref.fa", "q.fa"]  # never taken as a file, and it takes no value
    assert not o["hidden_sort"]              # only the exact -s is the sort tool


def test_smem_does_not_disturb_the_other_options():
    o = hostlib.parse_options(["slaMEM", "-smem", "-b", "-l", "31", "-o", "out.txt", "ref.fa", "q1.fa", "q2.fa"])
    assert (o["match_type"], o["both_strands"], o["min_mem_len"], o["files"]) == (3, 1, 31, ["ref.fa", "q1.fa", "q2.fa"])
    assert o["out_arg"] == 6


@pytest.mark.parametrize("args", [
    ["-smem", "-mam", "x", "ref.fa", "q.fa"],
    ["-mam", "x", "-smem", "ref.fa", "q.fa"],
    ["-smem", "ref.fa", "q.fa", "-mum"],
    ["-mam", "x", "-smem", "ref.fa", "q.fa", "-mum"],
])
def test_smem_with_mam_or_mum_is_match_type_minus_1(args):
    assert hostlib.parse_options(["slaMEM"] + args)["match_type"] == -1


def test_existing_match_types_unchanged():
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa"])["match_type"] == 0
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa", "-mam"])["match_type"] == 1
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa", "-mum"])["match_type"] == 2
    assert hostlib.parse_options(["slaMEM", "-mam", "x", "ref.fa", "q.fa", "-mum"])["match_type"] == -1
    o = hostlib.parse_options(["slaMEM", "-s", "mems.txt"])
    assert o["hidden_sort"]


def parse_max_occ(args):
    L = hostlib.lib()
    L.slh_parse_max_occ.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
    argv = (C.c_char_p * (len(args) + 2))(b"slaMEM", *[a.encode() for a in args], None)
    out = C.c_int(-7)
    rc = L.slh_parse_max_occ(len(args) + 1, argv, C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("args,expect", [
    (["-smem", "ref.fa", "q.fa"], (0, 0)),
    (["-smem", "-occ", "5", "ref.fa", "q.fa"], (1, 5)),
    (["-smem", "ref.fa", "q.fa", "-occ", "1"], (1, 1)),
    (["-OCC", "2", "-smem", "ref.fa", "q.fa"], (1, 2)),
    (["-smem", "-occ", "0", "ref.fa", "q.fa"], (-1, 0)),
    (["-smem", "-occ", "-3", "ref.fa", "q.fa"], (-1, 0)),
    (["-smem", "-occ", "two", "ref.fa", "q.fa"], (-1, 0)),
    (["-smem", "-occ", "3x", "ref.fa", "q.fa"], (-1, 0)),
    (["-smem", "ref.fa", "q.fa", "-occ"], (-1, 0)),
    (["-smem", "-o", "out.txt", "ref.fa", "q.fa"], (0, 0)),
])
def test_occ_values_and_errors(args, expect):
    assert parse_max_occ(args) == expect


def test_occ_value_is_not_a_file_and_o_stays_the_output():
    o = hostlib.parse_options(["slaMEM", "-smem", "-occ", "4", "-o", "out.txt", "ref.fa", "q.fa"])
    assert o["files"] == ["ref.fa", "q.fa"]
    assert o["out_arg"] == 5


@pytest.mark.parametrize("args,message", [
    (["-occ", "3"], b"> ERROR: Option -occ needs -smem"),
    (["-mum", "-occ", "3"], b"> ERROR: Option -occ needs -smem"),
    (["-smem", "-occ", "0"], b"> ERROR: Option -occ needs a whole number of at least 1"),
    (["-smem", "-occ", "many"], b"> ERROR: Option -occ needs a whole number of at least 1"),
    (["-smem", "-mam", "x"], b"> ERROR: Option -smem excludes -mam and -mum"),
    (["-mum", "x", "-smem"], b"> ERROR: Option -smem excludes -mam and -mum"),
    (["-mam", "x", "-mum", "x"], b"> ERROR: Options -mam and -mum exclude each other"),
])
def test_refused_combinations_exit_255_before_any_work(args, message, tmp_path):
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    out = tmp_path / "out.txt"
    r = subprocess.run([EXE] + args + ["-o", str(out), ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60)
    assert r.returncode == 255
    assert message in r.stdout
    assert not out.exists()


def test_usage_lists_smem_and_occ():
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"\t-smem\t" in r.stdout and b"\t-occ\t" in r.stdout


# ---- the definition ---------------------------------------------------------------------------------------------------------

def test_worked_example():
    rows = np.array([(500, 10, 20), (900, 10, 20), (100, 5, 30), (40, 0, 22)])
    assert smem_spec.in_emission_order(rows)
    assert list(smem_spec.smem_keep(rows)) == [False, False, True, True]
    rest = rows[[0, 1, 3]]
    assert list(smem_spec.smem_keep(rest)) == [True, True, True]
    assert list(smem_spec.occurrence_counts(rest)) == [2, 2, 1]
    assert list(smem_spec.block_keep(rest, 1)) == [False, False, True]
    assert list(smem_spec.block_keep(rest, 2)) == [True, True, True]


def _random_pair(rng):
    """A small text (records joined by one N) with nested repeats planted in it, and a query taken partly from it."""
    alpha = np.frombuffer(b"ACGT"[: int(rng.integers(1, 5))], dtype=np.uint8)
    recs = [rng.choice(alpha, size=int(rng.integers(1, 60))).tobytes() for _ in range(int(rng.integers(1, 4)))]
    text = bytearray(b"N".join(recs))
    if len(text) > 12 and rng.integers(0, 2):  # a segment copied elsewhere, and a shorter piece of it once more
        a = int(rng.integers(0, len(text) - 6))
        seg = bytes(text[a:a + int(rng.integers(3, 12))])
        at = int(rng.integers(0, len(text)))
        text[at:at] = seg
        at = int(rng.integers(0, len(text)))
        text[at:at] = seg[1:-1]
    text = bytes(text)
    parts = []
    for _ in range(int(rng.integers(1, 4))):
        if rng.integers(0, 3):
            a = int(rng.integers(0, len(text)))
            parts.append(text[a:a + int(rng.integers(1, 30))])
        else:
            parts.append(rng.choice(np.append(alpha, np.uint8(ord("N"))), size=int(rng.integers(1, 20))).tobytes())
    q = b"".join(parts) or b"A"
    return text, q


def _rows(m):
    return np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1).astype(np.int64) if len(m) else np.zeros((0, 3), np.int64)


@pytest.mark.parametrize("seed", range(4))
def test_definition_on_random_pairs(seed):
    """>= 500 pairs over the four seeds, both strands: the emission order (the oracle's, which in-order parity tests tie to the
    engine's), its completeness against brute force, claim 1 and claim 2."""
    rng = np.random.default_rng(4200 + seed)
    kept = dropped = capped = multi = 0
    for _ in range(130):
        text, q = _random_pair(rng)
        min_len = int(rng.integers(1, 7))
        o = po.OracleIndex(text)
        for strand in (q, po.reverse_complement(q)):
            rows = _rows(o.get_matches(strand, min_len))
            brute = _rows(po.brute_force_mems(text, strand, min_len))
            assert np.array_equal(po.sorted_triples(o.get_matches(strand, min_len)),
                                  brute[np.lexsort((brute[:, 2], brute[:, 1], brute[:, 0]))]), (text, strand, min_len)
            assert smem_spec.in_emission_order(rows), (text, strand, min_len, rows)
            assert smem_spec.runs_adjacent(rows), (text, strand, min_len, rows)
            keep = smem_spec.smem_keep(rows)
            assert np.array_equal(keep, smem_spec.claim1_keep(text, strand, rows)), (text, strand, min_len, rows)
            occ = smem_spec.occurrence_counts(rows)
            assert np.array_equal(occ[keep], smem_spec.claim2_counts(text, strand, rows[keep])), (text, strand, min_len)
            kept += int(keep.sum())
            dropped += int((~keep).sum())
            multi += int((occ[keep] > 1).sum())
            capped += int((smem_spec.block_keep(rows, 1) != keep).sum())
    assert kept and dropped and multi and capped


@pytest.mark.parametrize("case", MEM_CASES)
def test_definition_on_golden_files(case):
    """The golden -mem files the real reference wrote, rows mapped to merged coordinates through the front end's loader."""
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    blocks = mum_spec.parse_mems_file(open(exp_mems, "rb").read(), ref)
    strands = 2 if "-b" in opts else 1
    for b, (_, rows) in enumerate(blocks):
        i = b // strands
        strand = qs.chars[qs.offsets[i]:qs.offsets[i + 1]]
        if b % strands:
            strand = po.reverse_complement(strand)
        rows = rows.astype(np.int64)
        assert smem_spec.in_emission_order(rows), (case, b)
        assert smem_spec.runs_adjacent(rows), (case, b)
        keep = smem_spec.smem_keep(rows)
        assert np.array_equal(keep, smem_spec.claim1_keep(ref.chars, strand, rows)), (case, b)
        occ = smem_spec.occurrence_counts(rows)
        assert np.array_equal(occ[keep], smem_spec.claim2_counts(ref.chars, strand, rows[keep])), (case, b)


def test_golden_cases_include_blocks_the_filter_and_the_cap_change():
    changed = capped = 0
    for case in MEM_CASES:
        plain = open(case_paths(case)[2], "rb").read()
        data, _, _, _, _ = smem_spec.golden_smem_file(case)
        data1, _, _, _, _ = smem_spec.golden_smem_file(case, 1)
        changed += data != plain
        capped += data1 != data
    assert len(MEM_CASES) == 17
    assert changed >= 5 and capped >= 3
