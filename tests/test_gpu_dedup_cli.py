"""slaMEM-hip -dedup on the MI355X: the mixed batch of test_gpu_dedup written as FASTA and as FASTQ, through -vcf and -depth; the
files are what events_spec and depth_spec make of the reads tests/dedup_spec.py keeps, the line on stderr carries its counts; and
the option's refusals, which come before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import dedup_spec as dd
import depth_spec as ds
import events_spec as es
import lowq_spec
import pile_spec
from test_gpu_dedup import MIN_LEN, N, batch, mapped, mixed_batch
from test_gpu_pile import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    import hostlib
    from slamem_amd import engine
    tmp = tmp_path_factory.mktemp("dedup_cli")
    ref, reads, _ = mixed_batch()
    ref_fa, q_fa, q_fq = str(tmp / "ref.fa"), str(tmp / "reads.fa"), str(tmp / "reads.fq")
    write_fasta(ref_fa, [(b"one first", ref[:1500]), (b"two", ref[1501:])])
    write_fasta(q_fa, [(b"read%d x" % k, r) for k, r in enumerate(reads)])
    with open(q_fq, "wb") as f:
        f.write(lowq_spec.write_fastq([(b"read%d x" % k, r, b"I" * len(r)) for k, r in enumerate(reads)]))
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(ref)
    idx = engine.Index.build(ref)
    res = mapped(idx, ref, reads)
    idx.close()
    q, off = batch(reads)
    tables = {}
    for min_mapq in (0, 20):
        flags = dd.flags([(res, off)], min_mapq)[0]
        kept = dd.keep(res, flags)
        cand = sum(dd.is_candidate(r, min_mapq) for r in res)
        tables[min_mapq] = (pile_spec.pile(kept, q, off, N, min_mapq), es.events(kept, q, off, ref, min_mapq)[0], cand, int(flags.sum()),
                            pile_spec.pile(res, q, off, N, min_mapq), es.events(res, q, off, ref, min_mapq)[0])
    return dict(tmp=tmp, ref_fa=ref_fa, queries={"fasta": q_fa, "fastq": q_fq}, loaded=loaded, tables=tables)


def stderr_line(cand, dup):
    return b"> Duplicates: %d candidate reads, %d duplicates (%.2f %%) not counted, 0 without room in the duplicate table\n" % (
        cand, dup, 100.0 * dup / cand)


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_vcf_and_depth_files_are_the_specs_of_the_kept_reads(case, fmt):
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    q_file = case["queries"][fmt]
    # -vcf -dedup -minq 20 (-mdep 1 -mpct 0: at one read per key the depth is a few, and every call is to be seen)
    table, ev, cand, dup, all_table, all_ev = case["tables"][20]
    want = es.vcf_file(table, ev, case["loaded"], 1, 0)
    assert want != es.vcf_file(all_table, all_ev, case["loaded"], 1, 0) and want.count(b";SF=") >= 2 and dup > 60
    out = str(case["tmp"] / (fmt + ".vcf"))
    r = subprocess.run([EXE, "-b", "-l", str(MIN_LEN), "-vcf", "-dedup", "-minq", "20", "-mdep", "1", "-mpct", "0", "-o", out, case["ref_fa"], q_file],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=base, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    assert open(out, "rb").read() == want
    assert stderr_line(cand, dup) in r.stderr and b"WARNING" not in r.stderr
    # -depth -dedup, the option in front and a table of 64 slots: forty keys find room
    table, _, cand, dup, all_table, _ = case["tables"][0]
    want = ds.bedgraph_file(table, case["loaded"])
    assert want != ds.bedgraph_file(all_table, case["loaded"]) and want.count(b"\n") > 40
    out = str(case["tmp"] / (fmt + ".bedgraph"))
    r = subprocess.run([EXE, "-dedup", "-dslots", "64", "-depth", "-b", "-l", str(MIN_LEN), "-o", out, case["ref_fa"], q_file],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=base, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    assert open(out, "rb").read() == want
    assert stderr_line(cand, dup) in r.stderr
    summary = b"".join(l + b"\n" for l in r.stderr.split(b"\n") if l.startswith(b"> Depth of "))
    assert summary == ds.summary_lines(table, case["loaded"], 1)


@pytest.mark.parametrize("args,env,message", [
    (["-paf", "-dedup"], {}, b"Option -dedup needs -pile, -sites, -vcf, -cons or -depth"),
    (["-dedup"], {}, b"Option -dedup needs -pile, -sites, -vcf, -cons or -depth"),
    (["-pile", "-dslots", "64"], {}, b"Option -dslots needs -dedup"),
    (["-pile", "-dedup", "-dslots", "100"], {}, b"Option -dslots needs a power of two of at least 64"),
    (["-pile", "-dedup"], {"SLAMEM_GPUS": "2"}, b"Option -dedup runs on one GPU"),
    (["-dedup", "-depth"], {"SLAMEM_LOGICAL_GPUS": "2"}, b"Option -dedup runs on one GPU"),
])
def test_refusals_come_before_any_gpu_work(args, env, message, tmp_path):
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"r", b"ACGT" * 30)])
    write_fasta(q_fa, [(b"q", b"ACGT" * 10)])
    r = subprocess.run([EXE] + args + [ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", **env))  # (no device: it never asks for one)
    assert r.returncode == 255 and message in r.stdout and b"Building index" not in r.stdout
    assert not os.path.exists(str(tmp_path / "ref-mems.txt"))
