"""-affine on the MI355X: k_aln_wave_affine and the inline rule of k_aln_geom held to the matrix form of
tests/affine_spec.py -- every result compared for exact equality with the definition applied to the complete -mem list of the
same engine -- through find_alns, map_reads, the pileup with events, MapStats, both kinds of stream and the executable; costs
1,0,1 through the affine kernel against the unit-cost kernel; and the executable without -affine against the unit-cost spec."""
import os
import subprocess

import numpy as np
import pytest

import affine_spec
import aln_gap_cases as cases
import aln_spec
import events_spec
import ext_spec
import gt_spec
import map_spec
import pile_spec
from golden_cases import CASES, MANIFEST, case_paths, opt_value
from test_affine_host import three_substitutions
from test_gpu_aln import assert_equals_blocks, batch, seg_rows
from test_gpu_chain import indel_reads
from test_gpu_events import got_events
from test_gpu_map import assert_equals_reads, rec_rows
from test_gpu_pile import same, windows, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]
DEFAULT = (4, 6, 2)
ACGT = cases.ACGT


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def spec_blocks(mem, boff, ref, q, off, both, E, costs, gaps_out=None):
    return affine_spec.filter_blocks(mem, boff, ref, q, off, both, E=E, costs=costs, gaps_out=gaps_out)


def spec_reads(mem, boff, ref, q, off, both, E, costs):
    with affine_spec.in_aln_spec(costs):
        return map_spec.filter_reads(mem, boff, ref, q, off, both, E=E)


# ---- constructed reads against the definition ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases(eng, case):
    idx = None
    for costs in (DEFAULT, (5, 10, 1)):
        for E in (31, 3, 0):
            want, _, ref, qs, opts = affine_spec.golden_aln(case, E=E, costs=costs)
            text = np.frombuffer(ref.chars, dtype=np.uint8).copy()
            idx = idx or eng.Index.build(text)
            q, off = np.frombuffer(qs.chars, dtype=np.uint8), np.array(qs.offsets, dtype=np.uint64)
            min_len, both = int(opt_value(opts, "-l", 20)), "-b" in opts
            assert_equals_blocks(idx.find_alns(q, off, min_len, both, max_edits=E, gap_costs=costs), want)
    idx.close()


@pytest.fixture(scope="module")
def constructed(eng):
    """240 constructed reads and 160 indel reads of 200 letters on texts of 40 kbp, both strands: the engine's -mem rows, once."""
    out = []
    for ref, q, off in (aln_spec.constructed_reads(11)[:3], indel_reads(21)):
        idx = eng.Index.build(ref)
        out.append((idx, ref, q, off) + tuple(idx.find_mems(q, off, 20, True)))
    yield out
    for t in out:
        t[0].close()


@pytest.mark.parametrize("E", [31, 3, 0])
@pytest.mark.parametrize("costs", [DEFAULT, (5, 10, 1)])
def test_constructed_and_indel_reads(eng, constructed, costs, E):
    closed = indel = 0
    for idx, ref, q, off, mem, boff in constructed:
        gaps = []
        assert_equals_blocks(idx.find_alns(q, off, 20, True, max_edits=E, gap_costs=costs), spec_blocks(mem, boff, ref, q, off, True, E, costs, gaps))
        assert_equals_reads(idx.map_reads(q, off, 20, True, max_edits=E, gap_costs=costs), spec_reads(mem, boff, ref, q, off, True, E, costs))
        closed += sum(g is not None for _, _, g in gaps)
        indel += sum(g is not None and ("I" in g[0] or "D" in g[0]) for _, _, g in gaps)
    assert closed > 100 and (indel > 50 or E == 0)


def test_costs_1_0_1_through_the_affine_kernel_equal_the_unit_cost_kernel(eng, constructed):
    for idx, ref, q, off, mem, boff in constructed:
        for E in (31, 3, 0):
            unit = idx.find_alns(q, off, 20, True, max_edits=E)
            aff = idx.find_alns(q, off, 20, True, max_edits=E, gap_costs=(1, 0, 1))
            for a, b in zip(unit, aff):
                assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- the designed gaps -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cat(eng):
    ref, q, off, labels = cases.catalogue()
    idx = eng.Index.build(ref)
    mem, boff = idx.find_mems(q, off, cases.MIN_LEN, True)
    yield idx, ref, q, off, labels, mem, boff
    idx.close()


@pytest.mark.parametrize("E", [31, 64, 127])
def test_designed_gaps(eng, cat, E):
    """From 32 edits on a lane holds more than one diagonal, at 127 the cost runs to 260 and a slab is 800 KB.  What the
    catalogue is there for is asserted from the gaps the spec saw on the engine's rows."""
    idx, ref, q, off, labels, mem, boff = cat
    gaps = []
    want = spec_blocks(mem, boff, ref, q, off, True, E, DEFAULT, gaps)
    assert_equals_blocks(idx.find_alns(q, off, cases.MIN_LEN, True, max_edits=E, gap_costs=DEFAULT), want)
    closed = [(len(A), len(B), g) for A, B, g in gaps if g is not None]
    broken = [(A, B) for A, B, g in gaps if g is None]
    assert len(closed) >= 10 and len(broken) >= 10
    assert sum(not aln_spec.all_acgt(A[65:]) or not aln_spec.all_acgt(B[65:]) for A, B in broken) >= 2  # an N beyond letter 64
    if E == 127:
        assert sum(a == 0 for a, b, _ in closed) >= 2 and sum(b == 0 for a, b, _ in closed) >= 2
        for n in (63, 64, 65, 127, 128, 129):  # pieces at the borders of the 64-letter windows
            assert any(a == n or b == n for a, b, _ in closed), n
        assert any(g[2] > 200 for _, _, g in closed) and any(len(aln_spec.runs(g[0])) > 100 for _, _, g in closed)
        at = {l: k for k, l in enumerate(labels)}
        for label in ("repeat:AC-40", "repeat:AC-40+sub"):  # an indel inside (AC)n: the read has a segment across it
            segl = [s for b in (2 * at[label], 2 * at[label] + 1) for s in want[b]]
            assert any("D" in [c for c, _ in s[5]] for s in segl), label


def test_more_listed_gaps_than_workgroups_at_127_edits(eng, cat):
    """230 reads with one listed gap each on the 84 one-wave workgroups that the slab rule admits at 127 edits and costs 4,6,2:
    every workgroup closes a second and a third gap in the same LDS and slab."""
    idx, ref = cat[0], cat[1]
    bref, q, off, _ = cases.bulk()
    assert np.array_equal(bref, ref)
    n = 230
    q, off = q[:int(off[n])], off[:n + 1]
    mem, boff = idx.find_mems(q, off, cases.MIN_LEN, True)
    gaps = []
    want = spec_blocks(mem, boff, ref, q, off, True, 127, DEFAULT, gaps)
    assert_equals_blocks(idx.find_alns(q, off, cases.MIN_LEN, True, max_edits=127, gap_costs=DEFAULT), want)
    listed = sum(g is not None and (len(A) != len(B) or g[1] > 4) for A, B, g in gaps)
    assert listed >= 200 > (64 << 20) // (3 * 261 * 255 * 4)


# ---- the inline tier ---------------------------------------------------------------------------------------------------------------

def test_three_and_four_differing_letters_at_every_position_of_a_64_letter_piece(eng):
    """Reads of 160 exact letters, a piece of 64 with 3 or 4 substitutions (its first and its last letter among them, the others
    at every position in turn) and 160 exact letters, searched with -l 70 so that no match inside the piece is an anchor: gaps
    with a == b == 64 that k_aln_geom decides itself at costs 4,6,2 (d x <= 16) and hands to the wave kernel at unit cost."""
    rng = np.random.default_rng(4290)
    ref = rng.choice(ACGT, size=30_000)
    reads = []
    for d in (3, 4):
        for p in range(64):
            places = {0, 63, p if 0 < p < 63 else 31}
            if d == 4:
                places.add(next(t for t in range(1 + (7 * p + 5) % 62, 200) if 0 < t % 63 < 63 and t % 63 not in places) % 63)
            a = int(rng.integers(200, len(ref) - 600))
            r = ref[a:a + 384].copy()
            for t in places:
                r[160 + t] = rng.choice(ACGT[ACGT != r[160 + t]])
            assert len(places) == d
            reads.append(ext_spec.revcomp(r) if len(reads) % 2 else r)
    q, off = batch(reads)
    idx = eng.Index.build(ref)
    mem, boff = idx.find_mems(q, off, 70, True)
    for E, costs in ((31, DEFAULT), (3, DEFAULT), (31, (5, 10, 1)), (1, (4, 6, 2))):
        gaps = []
        want = spec_blocks(mem, boff, ref, q, off, True, E, costs, gaps)
        assert_equals_blocks(idx.find_alns(q, off, 70, True, max_edits=E, gap_costs=costs), want)
        assert len(gaps) == 128 and all(len(A) == len(B) == 64 for A, B, _ in gaps)
        ds = [sum(x != y for x, y in zip(A, B)) for A, B, _ in gaps]
        assert ds.count(3) == ds.count(4) == 64
        for (A, B, g), d in zip(gaps, ds):  # closed on the diagonal iff d x <= C
            assert (g is not None) == (d * costs[0] <= affine_spec.bound(E, costs))
            assert g is None or (set(g[0]) == {"=", "X"} and g[1] == d)
    idx.close()


# ---- integration -------------------------------------------------------------------------------------------------------------------

def clustered_sample():
    """The motivating case as a sample: 13 reads of 330 letters across the 12 letters with three substitutions, every other one
    reverse-complemented."""
    ref, read = three_substitutions()
    mutated = np.concatenate([ref[:100], read, ref[-100:]])
    assert len(mutated) == len(ref)
    reads = [mutated[8 * k:8 * k + 330] for k in range(13)]
    q, off = batch([ext_spec.revcomp(r) if k % 2 else r for k, r in enumerate(reads)])
    return ref, q, off


def test_pileup_events_of_three_clustered_substitutions(eng):
    """At unit cost every read shows an inserted and a deleted letter: two indel events.  At 4,6,2 it shows three X: none."""
    ref, q, off = clustered_sample()
    idx = eng.Index.build(ref)
    mem, boff = idx.find_mems(q, off, 20, True)
    found = {}
    for costs in (None, DEFAULT):
        res = map_spec.filter_reads(mem, boff, ref, q, off, True) if costs is None else spec_reads(mem, boff, ref, q, off, True, 31, costs)
        p = eng.Pileup(idx, events=True)
        recs = p.add(q, off, 20, True, gap_costs=costs)
        assert np.array_equal(rec_rows(recs), map_spec.pack(res)[4])
        same(p.counts(), pile_spec.pile(res, q, off, len(ref)))
        want = events_spec.events(res, q, off, ref)
        assert got_events(p) == want
        found[costs] = (want[0], p.counts().astype(np.int64))
        p.close()
    assert len(found[None][0]) == 2 and sorted(e[1] for e in found[None][0]) == [0, 1] and len(found[DEFAULT][0]) == 0
    # the three letters are mismatches of all 13 reads at 4,6,2 (columns A C G T of the rows 260, 265, 270)
    table = found[DEFAULT][1]
    for row, letter in ((260, b"T"), (265, b"G"), (270, b"A")):
        assert table[row, b"ACGT".index(letter)] == 13 and table[row, :4].sum() == 13
    idx.close()


def run_stream(eng, idx, q, off, per, **kw):
    wins = windows(off, per)
    st = eng.Stream(idx, 3, 1 << 16, per, True, **kw)
    segs, counts, ops, nops, reads = [], [], [], [], []
    for w in wins[:2]:
        st.submit(q, w, cases.MIN_LEN)
    for b in range(len(wins)):
        m, bo, _ = st.next()
        o, oo = st.alns()
        if kw.get("paf"):
            reads.append(rec_rows(st.maps()))
        if b + 2 < len(wins):
            st.submit(q, wins[b + 2], cases.MIN_LEN)
        segs.append(seg_rows(m)); counts.append(np.diff(bo.astype(np.int64))); ops.append(o); nops.append(np.diff(oo.astype(np.int64)))
    st.close()
    return np.concatenate(segs), np.concatenate(counts), np.concatenate(ops), np.concatenate(nops), reads


@pytest.mark.parametrize("mode", ["aln", "paf"])
def test_streams(eng, cat, mode):
    idx, ref, q, off, labels, mem, boff = cat
    E = 64
    if mode == "aln":
        w_segs, w_boff, w_ops, w_ooff = aln_spec.pack(spec_blocks(mem, boff, ref, q, off, True, E, DEFAULT))
    else:
        w_segs, w_boff, w_ops, w_ooff, w_reads = map_spec.pack(spec_reads(mem, boff, ref, q, off, True, E, DEFAULT))
    segs, counts, ops, nops, reads = run_stream(eng, idx, q, off, 29, max_edits=E, gap_costs=DEFAULT, **{mode: True})
    assert np.array_equal(segs, w_segs) and np.array_equal(counts, np.diff(w_boff))
    assert np.array_equal(ops, w_ops) and np.array_equal(nops, np.diff(w_ooff))
    if mode == "paf":
        assert np.array_equal(np.concatenate(reads), w_reads)


def test_stream_refuses_costs_without_an_alignment_mode_and_a_bound_above_the_cap(eng, cat):
    from slamem_amd import capi
    with pytest.raises(ValueError):
        eng.Stream(cat[0], 2, 1 << 12, 8, True, gap_costs=DEFAULT)
    with pytest.raises(ValueError):
        eng.Stream(cat[0], 2, 1 << 12, 8, True, aln=True, max_edits=127, gap_costs=(4, 6, 4))
    L = capi.lib()
    st = eng.Stream(cat[0], 2, 1 << 12, 8, True, aln=True)
    for word in (affine_spec.aln_word(127, (4, 6, 4)), affine_spec.aln_word(31, (32, 6, 2)), 31 | 6 << 16 | 2 << 24, 128):
        assert L.slamem_stream_set_max_edits(st._h, word) == capi.SLAMEM_ERR_ARG
    assert L.slamem_stream_set_max_edits(st._h, affine_spec.aln_word(126, (4, 8, 4))) == capi.SLAMEM_OK
    st.close()


def test_map_stats_and_the_pileup_take_the_costs(eng, constructed):
    idx, ref, q, off, mem, boff = constructed[1]
    got = idx.map_reads(q, off, 20, True, gap_costs=DEFAULT)
    a, b = eng.MapStats(idx), eng.MapStats(idx)
    recs = a.add(q, off, 20, True, gap_costs=DEFAULT)
    b.add_mapped(q, off, got)
    assert np.array_equal(rec_rows(recs), rec_rows(got[4])) and np.array_equal(a.raw(), b.raw())
    a.close(); b.close()
    p = eng.Pileup(idx)
    p.add(q, off, 20, True, gap_costs=DEFAULT)
    same(p.counts(), pile_spec.pile(spec_reads(mem, boff, ref, q, off, True, 31, DEFAULT), q, off, len(ref)))
    p.close()


def test_compact_index_and_bad_costs_are_refused(eng, monkeypatch):
    from slamem_amd import capi
    ref, q, off = indel_reads(13)
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    idx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    assert idx.info.layout == capi.LAYOUT_COMPACT
    with pytest.raises(capi.SlamemError) as e:
        idx.find_alns(q, off, 14, True, gap_costs=DEFAULT)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "text planes" in str(e.value) and "compact" in str(e.value)
    idx.close()
    idx = eng.Index.build(ref)
    with pytest.raises(ValueError):
        idx.find_alns(q, off, 14, True, max_edits=127, gap_costs=(4, 6, 4))
    with pytest.raises(capi.SlamemError) as e:  # the word itself, past the Python check
        idx._aln_like(q, off, 14, True, 0, 0, None, affine_spec.aln_word(127, (4, 6, 4)), None, False)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "512" in str(e.value)
    idx.close()


# ---- the executable ----------------------------------------------------------------------------------------------------------------

def run_exe(args):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                       timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return r.stdout


def test_executable_with_and_without_the_option(eng, cat, tmp_path):
    """slaMEM-hip -b -l 20 -aln -maxed 64 on the catalogue: with -affine 4,6,2 the file of the affine spec, without it the file
    the unit-cost spec writes and the parameter line of before."""
    import hostlib
    idx, cref, q, off, labels, mem, boff = cat
    ref_fa, q_fa, out = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), str(tmp_path / "out.txt")
    write_fasta(ref_fa, [(b"designed", cref)])
    write_fasta(q_fa, [(b"r%d %s" % (k, labels[k].encode()), q[int(off[k]):int(off[k + 1])]) for k in range(len(labels))])
    ref, qs = hostlib.Loaded(ref_fa, 1), hostlib.Loaded(q_fa, 0)
    files = {}
    for costs in (DEFAULT, None):
        blocks = aln_spec.filter_blocks(mem, boff, cref, q, off, True, E=64) if costs is None else spec_blocks(mem, boff, cref, q, off, True, 64, costs)
        files[costs] = affine_spec.aln_file(qs.names, blocks, ref, 2)
        stdout = run_exe(["-b", "-l", "20", "-aln", "-maxed", "64"] + (["-affine", "4,6,2"] if costs else []) + ["-o", out, ref_fa, q_fa])
        assert open(out, "rb").read() == files[costs]
        assert (b"; maximum edits = 64 ; gap costs = 4,6,2\n" if costs else b"; maximum edits = 64\n") in stdout
        assert (b"gap costs" in stdout) == (costs is not None)
    assert files[None] != files[DEFAULT]


def test_executable_vcf_gt(eng, tmp_path):
    """-vcf -gt on the clustered sample: at unit cost the file calls an insertion and a deletion, with -affine 4,6,2 three SNVs;
    both byte for byte what gt_spec formats from the spec's pileup and events."""
    import hostlib
    ref, q, off = clustered_sample()
    ref_fa, q_fa, out = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), str(tmp_path / "out.vcf")
    write_fasta(ref_fa, [(b"locus", ref)])
    write_fasta(q_fa, [(b"read%d" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    idx = eng.Index.build(ref)
    mem, boff = idx.find_mems(q, off, 20, True)
    idx.close()
    head = gt_spec.vcf_header(loaded)
    body = {}
    for costs in (None, DEFAULT):
        res = map_spec.filter_reads(mem, boff, ref, q, off, True) if costs is None else spec_reads(mem, boff, ref, q, off, True, 31, costs)
        want = gt_spec.vcf_file(pile_spec.pile(res, q, off, len(ref)), events_spec.events(res, q, off, ref)[0], loaded, gt_spec.params())
        run_exe(["-b", "-vcf", "-gt"] + (["-affine", "4,6,2"] if costs else []) + ["-o", out, ref_fa, q_fa])
        assert open(out, "rb").read() == want and want.startswith(head)
        body[costs] = [l.split(b"\t") for l in want[len(head):].split(b"\n")[:-1]]
    assert sorted(len(l[3]) - len(l[4]) for l in body[None]) == [-1, 1]          # one inserted, one deleted letter
    assert [(int(l[1]), l[3], l[4]) for l in body[DEFAULT]] == [(261, b"C", b"T"), (266, b"T", b"G"), (271, b"G", b"A")]
