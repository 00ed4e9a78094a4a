"""-mum without a GPU: the option as the front end parses it, the refusal of -mam with -mum, and the definition the GPU tests
check against -- the containment filter of a block's -mem rows equals counting the row's string in the merged reference and in
the scanned strand, on random pairs (brute-force MEM lists) and on the golden -mem files the real reference wrote."""
import os
import subprocess

import numpy as np
import pytest

import hostlib
import mum_spec
from golden_cases import CASES, MANIFEST, case_paths
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]


def test_mum_option_sets_match_type_2():
    o = hostlib.parse_options(["slaMEM", "-mum", "x", "ref.fa", "q.fa"])
    assert o["match_type"] == 2
    assert o["files"] == ["ref.fa", "q.fa"]
    # the reference's quirk: every -m... option takes the next argument as its value, so -mum goes last like -mam
    o = hostlib.parse_options(["slaMEM", "-b", "-l", "20", "ref.fa", "q.fa", "-mum"])
    assert (o["match_type"], o["files"], o["both_strands"], o["min_mem_len"]) == (2, ["ref.fa", "q.fa"], 1, 20)
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa", "-mam"])["match_type"] == 1
    assert hostlib.parse_options(["slaMEM", "ref.fa", "q.fa"])["match_type"] == 0


def test_mam_and_mum_together_are_refused(tmp_path):
    assert hostlib.parse_options(["slaMEM", "-mam", "x", "ref.fa", "q.fa", "-mum"])["match_type"] == -1
    exe = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
    ref_fa, q_fa, _, _ = case_paths("acgt_l20_fwd")
    out = tmp_path / "out.txt"
    r = subprocess.run([exe, "-mam", "x", "-o", str(out), ref_fa, q_fa, "-mum"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60)
    assert r.returncode == 255
    assert b"> ERROR: Options -mam and -mum exclude each other" in r.stdout
    assert not out.exists()


def _random_pair(rng):
    alpha = np.frombuffer(b"ACGT"[: int(rng.integers(1, 5))], dtype=np.uint8)
    recs = [rng.choice(alpha, size=int(rng.integers(1, 40))).tobytes() for _ in range(int(rng.integers(1, 4)))]
    text = b"N".join(recs)  # the merged reference: records joined by one N
    q = rng.choice(np.append(alpha, np.uint8(ord("N"))), size=int(rng.integers(1, 50))).tobytes()
    if len(q) > 4 and rng.integers(0, 2):  # a duplicated query segment
        a = int(rng.integers(0, len(q) - 2))
        b = int(rng.integers(a + 1, min(len(q), a + 12) + 1))
        q = q + q[a:b]
    return text, q


@pytest.mark.parametrize("seed", range(4))
def test_containment_filter_equals_occurrence_counting_on_random_pairs(seed):
    rng = np.random.default_rng(1000 + seed)
    kept_some = dropped_some = 0
    for _ in range(150):
        text, q = _random_pair(rng)
        min_len = int(rng.integers(1, 7))
        for strand in (q, po.reverse_complement(q)):
            m = po.brute_force_mems(text, strand, min_len)
            rows = np.stack([m["ref_pos"], m["query_pos"], m["length"]], axis=1) if len(m) else np.zeros((0, 3))
            keep = mum_spec.containment_keep(rows)
            assert np.array_equal(keep, mum_spec.naive_keep(text, strand, rows)), (text, strand, min_len)
            kept_some += int(keep.sum())
            dropped_some += int((~keep).sum())
    assert kept_some and dropped_some


@pytest.mark.parametrize("case", MEM_CASES)
def test_containment_filter_equals_occurrence_counting_on_golden_files(case):
    """The golden -mem files the real reference wrote, rows mapped to merged coordinates through the front end's loader."""
    _, kept, ref, qs, opts = mum_spec.golden_mum_file(case)
    _, _, _, exp_mems = mum_spec.golden_inputs(case)
    blocks = mum_spec.parse_mems_file(open(exp_mems, "rb").read(), ref)
    strands = 2 if "-b" in opts else 1
    for b, (_, rows) in enumerate(blocks):
        i = b // strands
        strand = qs.chars[qs.offsets[i]:qs.offsets[i + 1]]
        if b % strands:
            strand = po.reverse_complement(strand)
        keep = mum_spec.naive_keep(ref.chars, strand, rows)
        assert np.array_equal(rows[keep], kept[b]), (case, b)


def test_golden_cases_include_blocks_the_filter_changes():
    changed = 0
    for case in MEM_CASES:
        data, _, _, _, _ = mum_spec.golden_mum_file(case)
        changed += data != open(case_paths(case)[2], "rb").read()
    assert changed >= 5
    assert len(MEM_CASES) == 17
