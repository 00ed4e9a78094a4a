"""-aln, -paf and -pile on the MI355X above the default of 31 edits per gap: the designed gaps of tests/aln_gap_cases.py at edit
limits from 31 to 127, every result compared for exact equality with the definition (aln_spec with the edit-distance matrix,
map_spec, pile_spec, events_spec) applied to the complete -mem list of the same engine.  From 32 edits on a lane of k_aln_wave
holds more than one diagonal of a wavefront, the traceback's run list grows to hundreds of entries, and at 127 edits the kernel
has 514 workgroups, so that a batch of 1,190 listed gaps makes every one of them close a second gap in the same LDS and slab;
downstream the mapper emits deletions of up to 127 and insertions above 31 letters, and segments of hundreds of operations.
What the batches have to contain is asserted from the gaps the spec saw on the engine's own rows
(aln_gap_cases.assert_coverage), not assumed from the builder."""
import os
import subprocess

import numpy as np
import pytest

import aln_gap_cases as cases
import aln_spec
import events_spec
import map_spec
import pile_spec
from conftest import search_path
from test_gpu_aln import assert_equals_blocks, assert_is_aln_of, seg_rows
from test_gpu_events import got_events
from test_gpu_map import assert_equals_reads, assert_is_map_of, rec_rows
from test_gpu_pile import same, spec_results, windows, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
L20 = cases.MIN_LEN


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


class Catalogue:
    """The catalogue batch, one index for the module, the engine's -mem rows and the spec's results per edit limit (computed
    once, never changed)."""

    def __init__(self, eng):
        self.ref, self.q, self.off, self.labels = cases.catalogue()
        self.idx = eng.Index.build(self.ref)
        self.mem, self.boff = self.idx.find_mems(self.q, self.off, L20, True)
        self._blocks, self._maps = {}, {}

    def blocks(self, E):
        if E not in self._blocks:
            gaps = []
            self._blocks[E] = (aln_spec.filter_blocks(self.mem, self.boff, self.ref, self.q, self.off, True, E=E, gaps_out=gaps), gaps)
        return self._blocks[E]

    def maps(self, E):
        if E not in self._maps:
            self._maps[E] = map_spec.filter_reads(self.mem, self.boff, self.ref, self.q, self.off, True, E=E)
        return self._maps[E]


@pytest.fixture(scope="module")
def cat(eng):
    c = Catalogue(eng)
    yield c
    c.idx.close()


@pytest.mark.parametrize("E,path", [(E, "seed") for E in cases.EDITS] + [(127, "walk")])
def test_find_alns_is_the_definition_at_every_edit_limit(eng, cat, E, path):
    with search_path(path):
        mem, boff = cat.idx.find_mems(cat.q, cat.off, L20, True)
        got = cat.idx.find_alns(cat.q, cat.off, L20, True, max_edits=E)
    for f in ("ref_pos", "query_pos", "length"):
        assert np.array_equal(mem[f], cat.mem[f])
    assert np.array_equal(boff, cat.boff)
    blocks, gaps = cat.blocks(E)
    assert_equals_blocks(got, blocks)
    cases.assert_coverage(gaps, E)  # (on the engine's own rows)


def test_more_listed_gaps_than_workgroups(eng, cat):
    """1,190 listed gaps on the 514 one-wave workgroups of 127 edits: the loop li += gridDim.x takes every workgroup through a
    second and a third gap with the LDS and the wavefront slab of the one before; compared in full."""
    ref, q, off, _ = cases.bulk()
    assert np.array_equal(ref, cat.ref)
    mem, boff = cat.idx.find_mems(q, off, L20, True)
    gaps = []
    assert_is_aln_of(cat.idx.find_alns(q, off, L20, True, max_edits=127), mem, boff, ref, q, off, True, E=127, gaps_out=gaps)
    assert cases.listed_and_closed(gaps) > 1100
    assert sum(g is not None and g[1] > 100 for _, _, g in gaps) >= 8  # (the expensive gaps among them)


def test_capacity_edges_at_127_edits(eng, cat):
    """An operations capacity of exactly enough is also a slab of exactly enough for run lists of up to 255 entries."""
    from slamem_amd import capi
    segs, boff, ops, ooff = cat.idx.find_alns(cat.q, cat.off, L20, True, max_edits=127)
    assert_equals_blocks((segs, boff, ops, ooff), cat.blocks(127)[0])
    want = (len(cat.mem), len(segs), len(ops))
    assert max(np.diff(ooff.astype(np.int64))) > 200
    got = cat.idx.find_alns(cat.q, cat.off, L20, True, max_edits=127, capacities=want)
    for a, b in zip(got, (segs, boff, ops, ooff)):
        assert np.array_equal(a, b)
    with pytest.raises(capi.SlamemError) as e:
        cat.idx.find_alns(cat.q, cat.off, L20, True, max_edits=127, capacities=(want[0], want[1], want[2] - 1))
    assert e.value.code == capi.SLAMEM_ERR_CAPACITY and e.value.totals == want


def test_map_reads_is_the_definition_at_127_edits(eng, cat):
    got = cat.idx.map_reads(cat.q, cat.off, L20, True, max_edits=127)
    want = cat.maps(127)
    assert_equals_reads(got, want)
    strands = [w[0] for w in want]
    assert strands.count(1) > 40 and strands.count(2) > 40 and 0 not in strands
    assert sum(len(w[4]) == 1 for w in want) > 120 and any(len(w[4]) == 2 for w in want)  # (the breaks: 128 edits, an N)


def test_pileup_and_events_at_127_edits(eng, cat):
    """Through real alignments: a deletion of 127 rows is an event, the insertions above 31 letters are counted in skipped[0]
    and nowhere else, and segments of hundreds of operations go through the wave kernels of the pileup and of the events."""
    res = spec_results(cat.idx, cat.ref, cat.q, cat.off, L20, True, E=127)
    assert res == cat.maps(127)
    p = eng.Pileup(cat.idx, events=True)
    recs = p.add(cat.q, cat.off, L20, True, max_edits=127)
    assert np.array_equal(rec_rows(recs), map_spec.pack(res)[4])
    same(p.counts(), pile_spec.pile(res, cat.q, cat.off, len(cat.ref)))
    want = events_spec.events(res, cat.q, cat.off, cat.ref)
    assert got_events(p) == want
    p.close()
    evs, skipped = want
    assert any(e[1] == 0 and e[2] == 127 for e in evs) and any(e[1] == 1 and e[2] == 31 for e in evs)
    assert skipped[0] > 0 and skipped[1:] == [0, 0]
    for strand in (1, 2):
        assert any(len(s[5]) > eng.PILE_LANE_OPS for r in res if r[0] == strand for s in r[4])
    assert max(len(s[5]) for r in res for s in r[4]) > 200


def run_stream(eng, cat, **kw):
    per = 13
    wins = windows(cat.off, per)
    st = eng.Stream(cat.idx, 3, 1 << 16, per, True, max_edits=127, **kw)
    g_segs, g_counts, g_ops, g_nops, g_reads = [], [], [], [], []
    st.submit(cat.q, wins[0], L20)
    st.submit(cat.q, wins[1], L20)
    for b in range(len(wins)):
        m, bo, tm = st.next()
        o, oo = st.alns()
        assert len(m) == int(bo[-1]) == len(oo) - 1 and int(oo[-1]) == len(o) and int(oo[0]) == 0
        if kw.get("paf"):
            g_reads.append(rec_rows(st.maps()))
        if b + 2 < len(wins):
            st.submit(cat.q, wins[b + 2], L20)  # every slot in use
        g_segs.append(seg_rows(m))
        g_counts.append(np.diff(bo.astype(np.int64)))
        g_ops.append(o)
        g_nops.append(np.diff(oo.astype(np.int64)))
    st.close()
    assert len(wins) > 6
    return np.concatenate(g_segs), np.concatenate(g_counts), np.concatenate(g_ops), np.concatenate(g_nops), g_reads


@pytest.mark.parametrize("mode", ["aln", "paf"])
def test_stream_is_the_definition_at_127_edits(eng, cat, mode):
    if mode == "aln":
        w_segs, w_boff, w_ops, w_ooff = aln_spec.pack(cat.blocks(127)[0])
    else:
        w_segs, w_boff, w_ops, w_ooff, w_reads = map_spec.pack(cat.maps(127))
    segs, counts, ops, nops, reads = run_stream(eng, cat, **{mode: True})
    assert np.array_equal(segs, w_segs) and np.array_equal(counts, np.diff(w_boff))
    assert np.array_equal(ops, w_ops) and np.array_equal(nops, np.diff(w_ooff))
    if mode == "paf":
        assert np.array_equal(np.concatenate(reads), w_reads)


@pytest.mark.parametrize("mode,gpus", [("aln", 1), ("paf", 1), ("paf", 2)])
def test_executable_at_maxed_127(eng, cat, mode, gpus, tmp_path):
    """slaMEM-hip -b -l 20 -aln | -paf -maxed 127 on the catalogue as FASTA: byte for byte what the spec's writers make of the
    spec's results."""
    import hostlib
    ref_fa, q_fa, out = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), str(tmp_path / "out.txt")
    write_fasta(ref_fa, [(b"designed", cat.ref)])
    write_fasta(q_fa, [(b"r%d %s" % (k, cat.labels[k].encode()), cat.q[int(cat.off[k]):int(cat.off[k + 1])]) for k in range(len(cat.labels))])
    ref, qs = hostlib.Loaded(ref_fa, 1), hostlib.Loaded(q_fa, 0)
    assert ref.chars == bytes(cat.ref) and qs.n == len(cat.labels)
    if mode == "aln":
        want = b"".join(aln_spec.format_block(qs.names[b // 2], b % 2, segl, ref) for b, segl in enumerate(cat.blocks(127)[0]))
    else:
        want = map_spec.paf_file(cat.maps(127), qs.names, qs.sizes, ref)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if gpus == 2:
        env.update(SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1")
    r = subprocess.run([EXE, "-b", "-l", str(L20), "-" + mode, "-maxed", "127", "-o", out, ref_fa, q_fa], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=env, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    assert b"; maximum edits = 127\n" in r.stdout
    if gpus == 2:
        assert b"replicated to 2 logical GPUs by RCCL broadcast ... OK" in r.stdout
    assert open(out, "rb").read() == want and want.count(b"127D") >= 1
