"""The read-outs of the pileup take the table from the GPU in ranges of rows (16 Mi by default), and a record that crosses a range
border, or a separator inside a range, takes other branches than a record inside one range does.  No test has a reference of
16 Mi rows, so SLAMEM_READOUT_ROWS=64 makes the ranges small instead: a reference of two records of 150 and 100 letters then
has borders at 64, 128 and 192 inside its records and the separator (row 150) inside a range, and every read-out must write
byte for byte what it writes with one range, and say the same on stderr -- with two logical GPUs, whose tables and events are
added up range by range, as well."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_sites import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
MODES = [["-pile"], ["-sites"], ["-vcf"], ["-vcf", "-gt"], ["-cons"], ["-depth"], ["-depth", "-win", "7"]]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Two records; a sample with an SNV and a deletion of two letters in the first and an insertion and an SNV in the second;
    reads of 60 letters of the sample every third position, every other one reverse-complemented, 120 times over (enough letters
    for two batches of SLAMEM_BATCH_MB=1, so that a second GPU has a table of its own)."""
    rng = np.random.default_rng(64)
    d = tmp_path_factory.mktemp("ranges")
    one, two = (bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)) for n in (150, 100))
    snv = lambda s, x: s[:x] + (b"A" if s[x:x + 1] != b"A" else b"C") + s[x + 1:]
    s_one = snv(one, 128)                            # (row 128: a range's first)
    s_one = s_one[:63] + s_one[65:]                  # the deletion lies across the border at 64
    s_two = snv(two[:41] + b"GT" + two[41:], 70)     # the insertion in front of row 151 + 41 = 192, a border
    reads = []
    for s in (s_one, s_two):
        for k, a in enumerate(range(0, len(s) - 60 + 1, 3)):
            r = s[a:a + 60]
            reads.append(r.translate(COMP)[::-1] if k % 2 else r)
    assert 30 < len(reads) < 100
    ref_fa, q_fa = str(d / "ref.fa"), str(d / "reads.fa")
    write_fasta(ref_fa, [(b"one first", np.frombuffer(one, dtype=np.uint8)), (b"two", np.frombuffer(two, dtype=np.uint8))])
    write_fasta(q_fa, [(b"read%d" % k, np.frombuffer(r, dtype=np.uint8)) for k, r in enumerate(reads * 120)])
    assert 120 * sum(len(r) for r in reads) > 256 << 10  # (the first batch of two GPUs takes a quarter of SLAMEM_BATCH_MB)
    return d, ref_fa, q_fa


def run(inputs, mode, name, **env):
    d, ref_fa, q_fa = inputs
    out = str(d / name)
    r = subprocess.run([EXE, "-b"] + mode + ["-o", out, ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env))
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    said = [l for l in r.stderr.split(b"\n") if l.startswith(b"> ") and b"HBM" not in l]
    return open(out, "rb").read(), said


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "".join(m))
def test_small_ranges_write_what_one_range_writes(inputs, mode):
    whole, said = run(inputs, mode, "whole.txt")
    small, said_small = run(inputs, mode, "small.txt", SLAMEM_READOUT_ROWS="64")
    print(mode, len(whole), "bytes;", said)
    assert whole.count(b"\n") > 3 and b"one" in whole and b"two" in whole
    assert small == whole
    assert said_small == said
    if mode in (["-pile"], ["-vcf", "-gt"], ["-cons"], ["-depth"]):  # the tables and events of two GPUs, added up in small ranges
        two, _ = run(inputs, mode, "two.txt", SLAMEM_READOUT_ROWS="64", SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1")
        assert two == whole


def test_the_sample_is_in_the_calls(inputs):
    """(the data is what the docstring says: the SNVs, the deletion and the insertion are called, next to the borders)"""
    vcf, _ = run(inputs, ["-vcf"], "calls.vcf", SLAMEM_READOUT_ROWS="64")
    rows = [l.split(b"\t") for l in vcf.split(b"\n") if l and not l.startswith(b"#")]
    pos = {(r[0], int(r[1]), len(r[3]), len(r[4])) for r in rows}
    print(sorted(pos))
    assert (b"one", 129, 1, 1) in pos and (b"two", 69, 1, 1) in pos
    assert any(c == b"one" and 50 <= p <= 63 and a == 3 and b == 1 for c, p, a, b in pos)  # (left-normalised: at 63 or in front of it)
    assert any(c == b"two" and 35 <= p <= 41 and a == 1 and b == 3 for c, p, a, b in pos)
