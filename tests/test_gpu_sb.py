"""-sb on the MI355X (slamem_pileup_enable_strands, slamem_pileup_forward, engine.Pileup(strands=True), the k_strand_* kernels, the
executable): the expectation comes from code that was there before -- the owner's table is a plain Pileup's and pile_spec's of all
results, the forward accumulator's is pile_spec's of the results without the strand-2 reads and a plain Pileup's that was given the
strand-1 reads alone -- in one add, two adds in either order, through a stream, with a low-quality mask and with the duplicate
filter; reset, the refusals, planted tables, and the file the executable writes against tests/sb_spec.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dedup_spec as dd
import events_spec as es
import ext_spec
import gt_spec as gs
import lowq_spec
import pile_spec
import sb_spec as ss
from test_gpu_aln import batch
from test_gpu_chain import indel_reads
from test_gpu_gt import planted_table
from test_gpu_pile import halves, run_stream, spec_results, windows, write_fasta
from test_sb_host import host_sb_vcf

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
MIN_LEN, MIN_MAPQ = 14, 20
N = 2 * 2048 + 5


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def other(letter, k=1):
    return ACGT[(int(np.nonzero(ACGT == letter)[0][0]) + k) % 4]


def sb_batch():
    """(text, reads): a text of 2 * 2048 + 5 rows in two records (the separator at 3000) with an N at 2500 and a copy of rows 500 ..
    619 at 3500 (a read inside it maps to two places: quality 0), and about 200 reads of 60 to 150 letters over both strands --
    see the list below for the designed ones."""
    rng = np.random.default_rng(25)
    text = rng.choice(ACGT, size=N)
    text[3500:3620] = text[500:620]
    text[3000] = text[2500] = ord("N")

    def piece(a, b, rev):
        r = text[a:b].copy()
        return ext_spec.revcomp(r) if rev else r
    reads = []
    for k in range(170):  # anywhere, either strand
        length = int(rng.integers(60, 151))
        a = int(rng.integers(0, N - length + 1))
        reads.append(piece(a, a + length, k % 2))
    for rev in (0, 1):
        reads.append(piece(1990, 2110, rev))       # an = run over the tile edge 2047 / 2048
        reads.append(piece(4040, 4160 - 59, rev))  # ... over 4095 / 4096 and up to row n - 1
        reads.append(piece(2440, 2560, rev))       # over the N row, the read shows N there
        r = text[2450:2570].copy()                 # ... and one that shows a letter there
        r[50] = ord("A")
        reads.append(ext_spec.revcomp(r) if rev else r)
        r = text[1000:1120].copy()                 # mismatches
        for x in (30, 31, 77):
            r[x] = other(r[x])
        reads.append(ext_spec.revcomp(r) if rev else r)
        r = np.concatenate([text[1300:1360], text[1363:1423]])  # a deletion of three rows
        reads.append(ext_spec.revcomp(r) if rev else r)
        r = np.concatenate([text[1600:1660], [other(text[1660]), other(text[1660], 2)], text[1660:1720]])  # an insertion of two letters
        reads.append(ext_spec.revcomp(r) if rev else r)
        r = text[700 + 1500 * rev:850 + 1500 * rev].copy()  # exact ends and a mismatch every sixth letter between them: more than 32 operations
        for x in range(24, 126, 6):
            r[x] = other(r[x])
        reads.append(ext_spec.revcomp(r) if rev else r)
        reads.append(piece(520, 600, rev))         # inside the copied rows: quality 0, below MIN_MAPQ
        reads.append(piece(100, 200, rev))         # twice each, the second time a duplicate
        reads.append(piece(100, 200, rev))
    reads.append(rng.choice(ACGT, size=80))        # unmapped
    order = rng.permutation(len(reads))
    return text, [reads[i] for i in order]


def forward_only(res):
    """The results as the forward accumulator sees them: a read of strand 2 is unmapped."""
    return [r if r[0] == 1 else (0,) + tuple(r[1:]) for r in res]


@pytest.fixture(scope="module")
def world(eng):
    text, reads = sb_batch()
    idx = eng.Index.build(text)
    q, off = batch(reads)
    res = spec_results(idx, text, q, off, MIN_LEN, True)
    want = pile_spec.pile(res, q, off, N, MIN_MAPQ)
    fwant = pile_spec.pile(forward_only(res), q, off, N, MIN_MAPQ)
    yield dict(text=text, idx=idx, reads=reads, q=q, off=off, res=res, want=want, fwant=fwant)
    idx.close()


def same(got, want, what=None):
    assert got.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.nonzero((got.astype(np.int64) != want).any(axis=1))[0]
    assert len(bad) == 0, "%s rows %s: got %s, want %s" % (what, bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())


def both_tables(p, want, fwant, what=None):
    got, fgot = p.counts(), p.forward.counts()
    same(got, want, (what, "all"))
    same(fgot, fwant, (what, "forward"))
    assert bool((fgot <= got).all()), what
    return got, fgot


def test_the_batch_is_what_it_claims(eng, world):
    res, reads = world["res"], world["reads"]
    assert 180 <= len(reads) <= 220 and all(60 <= len(r) <= 150 for r in reads)
    strands = [r[0] for r in res]
    assert strands.count(1) > 60 and strands.count(2) > 60 and strands.count(0) >= 1
    assert any(r[0] != 0 and r[1] < MIN_MAPQ for r in res) and pile_spec.contributing(res, MIN_MAPQ) < pile_spec.contributing(res, 0)
    for strand in (1, 2):  # the wave kernels have a read of either strand
        assert any(r[0] == strand and r[1] >= MIN_MAPQ and max(len(s[5]) for s in r[4]) > eng.PILE_LANE_OPS for r in res), strand
        mine = [r for r in res if r[0] == strand and r[1] >= MIN_MAPQ]
        ops = [op for r in mine for s in r[4] for op in s[5]]
        assert {"=", "X", "D", "I"} <= {aln_op(op) for op in ops}, strand
    want, fwant = world["want"], world["fwant"]
    assert want[:, 4].sum() > 0 and want[:, 5].sum() > 0 and fwant[:, 4].sum() > 0 and fwant[:, 5].sum() > 0
    assert bool((fwant <= want).all()) and 0 < fwant.sum() < want.sum()
    for x in (2047, 2048, 4095, 4096, N - 1):  # the tile edges are covered on both strands
        assert 0 < fwant[x, :4].sum() < want[x, :4].sum(), x
    assert want[2500].sum() == 0 or want[2500, :4].sum() > 0  # (the N row: only a read that shows a letter there counts, under X)
    assert want[2499, :4].sum() >= 4 and want[2501, :4].sum() >= 4


def aln_op(op):
    """The letter of an operation as the results hold it: (letter, length) tuples or packed words."""
    if isinstance(op, tuple):
        return op[0] if isinstance(op[0], str) else "?ID????=X"[int(op[0])]
    return "?ID????=X???????"[int(op) & 15]


def test_one_add_equals_the_plain_pileup_and_the_spec(eng, world):
    idx, q, off, res = world["idx"], world["q"], world["off"], world["res"]
    p = eng.Pileup(idx, strands=True)
    assert p.forward is not None and p.forward.forward is None
    recs = p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ)
    got, fgot = both_tables(p, world["want"], world["fwant"], "one add")
    plain = eng.Pileup(idx)
    plain.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ)
    assert np.array_equal(plain.counts(), got)
    # a plain accumulator that is given the strand-1 reads alone
    keep = [k for k in range(len(recs)) if int(recs["strand"][k]) == 1]
    assert [k for k, r in enumerate(res) if r[0] == 1] == keep
    qf, of = batch([world["reads"][k] for k in keep])
    plain.reset()
    plain.add(qf, of, MIN_LEN, True, min_mapq=MIN_MAPQ)
    assert np.array_equal(plain.counts(), fgot)
    # every read-out works on the borrowed handle: ranges over the tile edges, listed rows, sites, depth runs
    for first, count in ((2040, 20), (4090, 11), (N - 1, 1), (0, 0), (2048, 2048)):
        assert np.array_equal(p.forward.counts(first, count), fgot[first:first + count])
    at = [0, 2047, 2048, 2500, 4095, 4096, N - 1]
    assert np.array_equal(p.forward.rows_at(at), fgot[at])
    plain_sites, fwd_sites = plain.sites(min_depth=1, min_pct=1), p.forward.sites(min_depth=1, min_pct=1)
    assert all(np.array_equal(a, b) for a, b in zip(plain_sites, fwd_sites)) and len(fwd_sites[0]) > 0
    assert all(np.array_equal(a, b) for a, b in zip(plain.depth_runs(), p.forward.depth_runs()))
    plain.close()
    p.close()
    assert p.forward._h is None


def test_two_adds_in_either_order_reset_and_a_second_round(eng, world):
    idx, q, off = world["idx"], world["q"], world["off"]
    (qa, oa), (qb, ob) = halves(q, off)
    p = eng.Pileup(idx, strands=True)
    for k, order in enumerate((((qa, oa), (qb, ob)), ((qb, ob), (qa, oa)), ((qa, oa), (qb, ob)))):
        for qq, oo in order:
            p.add(qq, oo, MIN_LEN, True, min_mapq=MIN_MAPQ)
        both_tables(p, world["want"], world["fwant"], ("order", k))
        p.reset()
        assert not p.counts().any() and not p.forward.counts().any()
        p.enable_strands()  # (on an empty accumulator, and a second time: nothing changes)
    p.close()


def test_stream_feeds_both_tables(eng, world):
    idx, q, off = world["idx"], world["q"], world["off"]
    p = eng.Pileup(idx, strands=True)
    run_stream(eng, idx, p, q, windows(off, 70), 2, MIN_MAPQ)
    both_tables(p, world["want"], world["fwant"], "stream")
    p.close()


def test_low_quality_mask_on_both_strands(eng, world):
    idx, q, off, res = world["idx"], world["q"], world["off"], world["res"]
    rng = np.random.default_rng(6)
    bits = (rng.random(int(off[-1])) < 0.08).astype(np.uint8)
    for strand in (1, 2):  # low letters in a read of either strand that counts, under = and under X
        k = next(k for k, r in enumerate(res) if r[0] == strand and r[1] >= MIN_MAPQ and max(len(s[5]) for s in r[4]) > eng.PILE_LANE_OPS)
        bits[int(off[k]) + 20:int(off[k]) + 40] = 1
        assert bits[int(off[k]):int(off[k + 1])].sum() >= 20
    mask = lowq_spec.from_bits(bits.tolist())
    want = lowq_spec.pile(res, q, off, N, mask, MIN_MAPQ)
    fwant = lowq_spec.pile(forward_only(res), q, off, N, mask, MIN_MAPQ)
    assert want.sum() < world["want"].sum() and fwant.sum() < world["fwant"].sum()
    p = eng.Pileup(idx, strands=True)
    p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, lowq=mask)
    got, _ = both_tables(p, want, fwant, "mask")
    plain = eng.Pileup(idx)
    plain.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, lowq=mask)
    assert np.array_equal(plain.counts(), got)
    plain.close()
    p.close()


def test_dedup_counts_a_duplicated_forward_read_once_in_both_tables(eng, world):
    idx, q, off, res = world["idx"], world["q"], world["off"], world["res"]
    flags = dd.flags([(res, off)], MIN_MAPQ)[0]
    dup_fwd = [k for k, r in enumerate(res) if flags[k] == 1 and r[0] == 1]
    assert dup_fwd and any(r[0] == 2 and flags[k] == 1 for k, r in enumerate(res))
    kept = dd.keep(res, flags)
    want = pile_spec.pile(kept, q, off, N, MIN_MAPQ)
    fwant = pile_spec.pile(forward_only(kept), q, off, N, MIN_MAPQ)
    assert fwant.sum() < world["fwant"].sum()
    p = eng.Pileup(idx, strands=True, dedup=True)
    _, dup = p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, dedup=True)
    assert np.array_equal(dup, flags)
    got, _ = both_tables(p, want, fwant, "dedup")
    plain = eng.Pileup(idx, dedup=True)
    plain.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, dedup=True)
    assert np.array_equal(plain.counts(), got)
    plain.close()
    p.close()


def test_refusals(eng, world, monkeypatch):
    from slamem_amd import capi
    idx, q, off = world["idx"], world["q"], world["off"]
    L = capi.lib()
    p = eng.Pileup(idx, strands=True)
    f = p.forward
    z = np.zeros(64, dtype=np.uint64).ctypes.data
    calls = [("slamem_pileup_add_device", lambda: L.slamem_pileup_add_device(f._h, z, z, 0, z, z, z, z, z, 0, None)),
             ("slamem_pileup_add_masked_device", lambda: L.slamem_pileup_add_masked_device(f._h, z, z, 0, z, z, z, z, z, 0, None, None)),
             ("slamem_pileup_add_dedup_device", lambda: L.slamem_pileup_add_dedup_device(f._h, z, z, 0, z, z, z, z, z, 0, None, z, None, None)),
             ("slamem_pileup_add_events_host", lambda: L.slamem_pileup_add_events_host(f._h, z, 0)),
             ("slamem_pileup_add_events_device", lambda: L.slamem_pileup_add_events_device(f._h, z, 0, None)),
             ("slamem_pileup_enable_events", lambda: L.slamem_pileup_enable_events(f._h, 0)),
             ("slamem_pileup_enable_dedup", lambda: L.slamem_pileup_enable_dedup(f._h, 0)),
             ("slamem_pileup_enable_strands", lambda: L.slamem_pileup_enable_strands(f._h)),
             ("slamem_pileup_free", lambda: L.slamem_pileup_free(f._h))]
    for name, call in calls:
        assert call() == capi.SLAMEM_ERR_ARG, name
        msg = L.slamem_last_error_message()
        assert name.encode() in msg and b"forward accumulator" in msg, name
    with pytest.raises(capi.SlamemError) as e:
        f.add(q, off, MIN_LEN, True)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "forward accumulator" in str(e.value)
    with pytest.raises(capi.SlamemError) as e:
        eng.Stream(idx, 2, 1 << 16, 64, True, pile=f)
    assert "slamem_stream_set_pileup" in str(e.value)
    assert not p.counts().any() and not f.counts().any()  # (nothing of the above added anything)
    # add_counts on the borrowed handle is allowed
    rows = np.zeros((N, 6), dtype=np.uint32)
    rows[7] = (1, 2, 3, 4, 5, 6)
    f.add_counts(rows)
    assert np.array_equal(f.counts(), rows) and not p.counts().any()
    p.close()
    # enabling on an accumulator that holds something is refused, after a reset it is not
    for fill in ("add", "add_counts"):
        plain = eng.Pileup(idx)
        if fill == "add":
            plain.add(q, off, MIN_LEN, True)
        else:
            plain.add_counts(rows)
        with pytest.raises(capi.SlamemError) as e:
            plain.enable_strands()
        assert e.value.code == capi.SLAMEM_ERR_ARG and "empty" in str(e.value) and plain.forward is None
        h = C.c_void_p()
        assert L.slamem_pileup_forward(plain._h, C.byref(h)) == capi.SLAMEM_ERR_ARG and not h.value
        plain.reset()
        plain.enable_strands()
        assert plain.forward is not None and not plain.forward.counts().any()
        plain.close()
    assert L.slamem_pileup_enable_strands(None) == capi.SLAMEM_ERR_ARG and L.slamem_pileup_forward(None, None) == capi.SLAMEM_ERR_ARG
    # the compact layout is refused at create, as before
    ref, _, _ = indel_reads(13)
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    cidx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    with pytest.raises(capi.SlamemError) as e:
        eng.Pileup(cidx, strands=True)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "text planes" in str(e.value) and "slamem_pileup_create" in str(e.value)
    cidx.close()


# ---- planted tables and the executable -----------------------------------------------------------------------------------------

def test_planted_tables_through_add_counts(eng):
    """gt's planted table with a forward share per row -- all forward, all reverse, half -- goes in through add_counts on the owner
    and on the forward accumulator; the file the host formatter makes of the engine's read-outs is sb_spec's of the tables."""
    from test_map_host import FakeRef
    text, table = planted_table()
    n = len(text)
    share = np.arange(n) % 3
    ftable = np.where(share[:, None] == 0, table, np.where(share[:, None] == 1, 0, table // 2))
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, strands=True, events=True)
    p.add_counts(table.astype(np.uint32))
    p.forward.add_counts(ftable.astype(np.uint32))
    got, fgot = both_tables(p, table, ftable, "planted")
    ev = [(2048, 1, 1, b"A", 7, 7), (2049, 0, 3, b"", 30, 0), (11, 0, 1, b"", 0, 12)]
    p.add_events(es.to_records(sorted(ev, key=es.order_key)))
    evs = es.from_records(p.events()[0])
    assert len(evs) == 3
    ref = FakeRef([bytes(text[:3000]), bytes(text[3001:])], [b"one", b"two x"])
    assert ref.chars == bytes(text)
    for prm, fs in ((gs.params(), None), (gs.params(), 30), (gs.params(ploidy=1, min_qual=0), 10)):
        want = ss.vcf_file(table, ftable, evs, ref, prm, fs)
        assert host_sb_vcf(ref, got.astype(np.int64), fgot.astype(np.int64), evs, prm, fs) == want
        assert want.count(b"\n") > 100
    want = ss.vcf_file(table, ftable, evs, ref, gs.params(), 30)
    # (a row that is all forward or all reverse has a one-sided table, FS 0: what FS catches is an allele on a strand of its own)
    assert want.count(b"\tsb\t") >= 1 and want.count(b"\tPASS\t") > 10
    p.close()
    idx.close()


def sample_reads(text):
    """Reads of a sample beside the batch's: at rows 300, 1500, 2300 and 3900 another letter on four forward and four reverse reads,
    at rows 900 and 3300 another letter on ten forward reads and the text's own on ten reverse reads -- an allele on a strand of its own."""
    out = []
    for k, x in enumerate((300, 900, 1500, 2300, 3300, 3900)):
        biased = k % 3 == 1
        for j in range(20 if biased else 8):
            a = x - 20 - 3 * j
            r = text[a:a + 100].copy()
            rev = j % 2
            if not (biased and rev):
                r[x - a] = other(r[x - a])
            out.append(ext_spec.revcomp(r) if rev else r)
    return out


def test_cli_file_is_the_spec_of_the_engines_tables(eng, world, tmp_path):
    """slaMEM-hip -b -vcf -gt -sb: byte for byte the file sb_spec formats from the engine's two tables and its events, with and
    without -fs 30, on one GPU and on two logical ones (the forward accumulators merged as their owners are); without -sb the file
    of gt_spec, as before."""
    import hostlib
    text, idx = world["text"], world["idx"]
    reads = world["reads"] + sample_reads(text)
    q, off = batch(reads)
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"one first", text[:3000]), (b"two\tsecond", text[3001:])])
    write_fasta(q_fa, [(b"read%d x" % k, r) for k, r in enumerate(reads)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(text)
    p = eng.Pileup(idx, strands=True, events=True)
    p.add(q, off, 20, True, min_mapq=MIN_MAPQ)
    table, ftable = p.counts().astype(np.int64), p.forward.counts().astype(np.int64)
    ev = es.from_records(p.events()[0])
    p.close()
    prm = gs.params(min_depth=2, min_qual=3)
    args = ["-mdep", "2", "-qual", "3", "-minq", str(MIN_MAPQ)]
    plain = gs.vcf_file(table, ev, loaded, prm)
    sb = ss.vcf_file(table, ftable, ev, loaded, prm)
    sb30 = ss.vcf_file(table, ftable, ev, loaded, prm, 30)
    lines = sb[len(ss.vcf_header(loaded)):].split(b"\n")[:-1]
    assert len(lines) >= 7 and any(len(line.split(b"\t")[3]) != len(line.split(b"\t")[4]) for line in lines)  # (SNVs and indels)
    assert sb30.count(b"\tsb\t") == 2 and sb30.count(b"\tPASS\t") == len(lines) - 2  # (rows 900 and 3300)
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    two = dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1")
    for name, env, extra, want in (("sb1", base, ["-sb"], sb), ("sb2", two, ["-sb"], sb), ("fs1", base, ["-sb", "-fs", "30"], sb30),
                                   ("fs2", two, ["-fs", "30", "-sb"], sb30), ("gt", base, [], plain)):
        out = str(tmp_path / (name + ".vcf"))
        r = subprocess.run([EXE, "-b", "-vcf", "-gt"] + extra + args + ["-o", out, ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert open(out, "rb").read() == want, name
        assert (b"; strand bias = on" in r.stdout) == bool(extra) and (b"; maximum FS = 30" in r.stdout) == ("-fs" in extra)
