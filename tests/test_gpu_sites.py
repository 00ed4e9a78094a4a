"""-sites on the MI355X (slamem_pileup_sites_*, slamem_pileup_add_counts_*, engine.Pileup.sites / add_counts, the executable):
every result is tests/sites_spec.py applied to the table the same accumulator gives through counts(), compared for exact
equality -- on tables planted row by row (full and empty tiles, tile borders, thresholds at equality, products beyond 2^32), on
ranges, on a capacity that is too small, on real mappings with indels and on a reference of several records, whatever the
batches' order, the stream or the number of accumulators; and, without the spec, a known answer: twenty planted substitutions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sites_spec
from sites_spec import NONZERO, VARIANT
from test_gpu_chain import indel_reads
from test_gpu_map import multi_record_batch
from test_sites_host import PLANTED_SEED, planted_answer_holds, planted_sample

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
RULES = [(VARIANT, 4, 20), (VARIANT, 1, 0), (VARIANT, 2, 100), (VARIANT, 1, 3), (VARIANT, 1, 2), (VARIANT, 2 ** 31 - 1, 20), (NONZERO, 4, 20)]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def same_sites(got, want, what=None):
    for g, w, dtype in zip(got, want, (np.uint64, np.uint32, np.uint8)):
        assert g.dtype == dtype and g.shape == w.shape, (what, g.shape, w.shape)
        assert np.array_equal(g, w), what


def check_all(p, text, table, rules=RULES, ranges=((0, None),)):
    for mode, dep, pct in rules:
        for first, count in ranges:
            got = p.sites(dep, pct, mode, first, count)
            same_sites(got, sites_spec.sites(table, text, mode, dep, pct, first, count), (mode, dep, pct, first, count))


# ---- planted tables ------------------------------------------------------------------------------------------------------------

def planted_table():
    """A text of 10,000 letters (five tiles of 2,048 rows, the last one short) with a few N, and a table: tile 1 has every row
    selected in both modes, tile 3 none; rows 0, 2047, 2048, 4095, 4096 and n - 1 are selected; tile 0 holds the threshold rows
    of test_sites_host.py, tiles 2 and 4 random rows."""
    rng = np.random.default_rng(17)
    n = 10000
    text = rng.choice(ACGT, size=n)
    for x in (100, 1999, 4500, 5000, 9000, 9001):
        text[x] = ord("N")
    text[10:40] = ord("A")  # (the rows of the CPU test stand under its letter)
    col = {ord(c): k for k, c in enumerate("ACGT")}
    t = np.zeros((n, 6), dtype=np.int64)

    def variant(x, depth=10):  # the text's letter and another one, half each
        t[x] = 0
        t[x, col[int(text[x])]] = depth
        t[x, (col[int(text[x])] + 1 + x % 3) % 4] = depth
    for x in range(2048, 4096):
        variant(x)
    for x in (0, 2047, 4096, n - 1):
        variant(x)
    # tile 0: the rows of the CPU test -- thresholds at equality and one off, each column alone, products beyond 2^32
    for x, row in ((10, (16, 4, 0, 0, 0, 0)), (11, (17, 4, 0, 0, 0, 0)), (12, (16, 3, 0, 0, 1, 0)), (13, (20, 0, 0, 0, 0, 4)),
                   (14, (20, 0, 0, 0, 0, 3)), (15, (2, 2, 0, 0, 0, 0)), (16, (1, 2, 0, 0, 0, 0)), (17, (1, 2, 0, 0, 1, 0)),
                   (18, (0, 5, 0, 0, 0, 0)), (19, (1, 5, 0, 0, 0, 0)), (20, (9, 0, 0, 0, 0, 0)), (21, (0, 9, 0, 0, 0, 0)),
                   (22, (0, 0, 9, 0, 0, 0)), (23, (0, 0, 0, 9, 0, 0)), (24, (0, 0, 0, 0, 9, 0)), (25, (0, 0, 0, 0, 0, 9)),
                   (30, (2_000_000_000, 0, 50_000_000, 0, 0, 0)), (31, (50_000_000, 2_000_000_000, 0, 0, 0, 0)),
                   (32, (0, 0, 50_000_000, 2_000_000_000, 0, 0)), (33, (0, 50_000_000, 0, 2_000_000_000, 0, 0)),
                   (34, (2 ** 31 - 1,) * 6), (100, (3, 0, 0, 2, 1, 1)), (1999, (0, 0, 0, 0, 7, 0))):
        t[x] = row
    for x in np.nonzero(rng.random(n) < 0.3)[0]:
        if 4097 <= x < 6144 or 8192 <= x < n - 1:
            t[x] = rng.integers(0, 12, size=6) * (rng.random(6) < 0.5)
    return text, t


def test_planted_table_both_modes_and_ranges(eng):
    text, table = planted_table()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    p.add_counts(table.astype(np.uint32))
    assert np.array_equal(p.counts().astype(np.int64), table)
    # the table is what the docstring says it is
    pos, _, _ = sites_spec.sites(table, text, VARIANT, 4, 20)
    sel = set(int(x) for x in pos)
    assert set(range(2048, 4096)) <= sel and not any(6144 <= x < 8192 for x in sel) and {0, 2047, 4096, n - 1} <= sel
    assert {10, 13, 15} <= sel and not {11, 12, 14, 16, 20, 100, 1999} & sel
    assert 30 not in set(int(x) for x in sites_spec.sites(table, text, VARIANT, 1, 3)[0])
    assert 30 in set(int(x) for x in sites_spec.sites(table, text, VARIANT, 1, 2)[0])
    assert [int(x) for x in sites_spec.sites(table, text, VARIANT, 2 ** 31 - 1, 20)[0]] == [34]
    zero = set(int(x) for x in sites_spec.sites(table, text, NONZERO)[0])
    assert {100, 1999, 20} <= zero and not any(6144 <= x < 8192 for x in zero)
    check_all(p, text, table)
    ranges = ((2037, 4101), (2047, 2), (2048, 2048), (n - 70, 70), (n, 0), (0, 0), (5, 50), (4100, 1), (6144, 2048), (6000, 3000))
    check_all(p, text, table, rules=[(VARIANT, 4, 20), (NONZERO, 4, 20)], ranges=ranges)
    # the read-out leaves the accumulator alone
    assert np.array_equal(p.counts().astype(np.int64), table)
    p.close()
    idx.close()


def test_add_counts_adds(eng):
    import torch
    rng = np.random.default_rng(5)
    text = rng.choice(ACGT, size=6000)
    idx = eng.Index.build(text)
    table = (rng.integers(0, 50, size=(6000, 6)) * (rng.random((6000, 6)) < 0.2)).astype(np.uint32)
    p = eng.Pileup(idx)
    p.add_counts(table)
    p.add_counts(table)
    assert np.array_equal(p.counts().astype(np.int64), 2 * table.astype(np.int64))
    # a piece whose first row lies inside a tile and whose last row lies in the next; a device tensor
    p.add_counts(torch.from_numpy(table[3000:5000].view(np.int32)).to(idx.device), first=3000)
    want = 2 * table.astype(np.int64)
    want[3000:5000] += table[3000:5000]
    assert np.array_equal(p.counts().astype(np.int64), want)
    p.add_counts(table[:1], first=5999)
    want[5999] += table[0]
    p.add_counts(table[:0], first=6000)
    assert np.array_equal(p.counts().astype(np.int64), want)
    check_all(p, text, want, rules=[(VARIANT, 4, 20), (NONZERO, 1, 0)])
    from slamem_amd import capi
    for first, rows in ((5999, table[:2]), (6001, table[:0])):
        with pytest.raises(capi.SlamemError) as e:
            p.add_counts(rows, first=first)
        assert e.value.code == capi.SLAMEM_ERR_ARG
    L = capi.lib()
    rows = np.ascontiguousarray(table[100:400])
    assert L.slamem_pileup_add_counts_host(p._h, 2000, 300, rows.ctypes.data) == capi.SLAMEM_OK
    want[2000:2300] += table[100:400]
    assert L.slamem_pileup_add_counts_host(p._h, 5900, 101, rows.ctypes.data) == capi.SLAMEM_ERR_ARG
    assert np.array_equal(p.counts().astype(np.int64), want)
    with pytest.raises(ValueError):
        p.add_counts(table[:, :5])
    with pytest.raises(ValueError):
        p.add_counts(table.astype(np.int64))
    p.close()
    idx.close()


# ---- capacity and arguments ----------------------------------------------------------------------------------------------------

def test_capacity_too_small_reports_the_need_and_writes_nothing_beyond(eng):
    import torch
    from slamem_amd import capi
    text, table = planted_table()
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    p.add_counts(table.astype(np.uint32))
    want = sites_spec.sites(table, text, VARIANT, 4, 20)
    need = len(want[0])
    assert need > 2048
    L = capi.lib()
    dev = idx.device
    cap = 3
    pos = torch.full((cap + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    rows = torch.full((cap + 8, 6), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    alleles = torch.full((cap + 8,), 0x5A, dtype=torch.uint8, device=dev)
    total = C.c_uint64()
    rc = L.slamem_pileup_sites_device(p._h, 0, len(text), VARIANT, 4, 20, cap, pos.data_ptr(), rows.data_ptr(), alleles.data_ptr(),
                                      C.byref(total), None)
    torch.cuda.synchronize()
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need
    assert b"selected" in L.slamem_last_error_message()
    assert bool((pos[cap:] == 0x5A5A5A5A5A5A5A5A).all()) and bool((rows[cap:] == 0x5A5A5A5A).all()) and bool((alleles[cap:] == 0x5A).all())
    # (what fits is the head of the result)
    assert np.array_equal(pos[:cap].cpu().numpy().view(np.uint64), want[0][:cap])
    assert np.array_equal(rows[:cap].cpu().numpy().view(np.uint32), want[1][:cap])
    # the host call: the same need, and room for it gives the result
    hp, hc, ha = np.zeros(need + 2, dtype=np.uint64), np.zeros((need + 2, 6), dtype=np.uint32), np.full(need + 2, 0x5A, dtype=np.uint8)
    rc = L.slamem_pileup_sites_host(p._h, 0, len(text), VARIANT, 4, 20, 5, hp.ctypes.data, hc.ctypes.data, ha.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and bool((ha[5:] == 0x5A).all())
    rc = L.slamem_pileup_sites_host(p._h, 0, len(text), VARIANT, 4, 20, need, hp.ctypes.data, hc.ctypes.data, ha.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_OK and total.value == need and bool((ha[need:] == 0x5A).all())
    same_sites((hp[:need], hc[:need], ha[:need]), want)
    # no room at all: the count alone
    rc = L.slamem_pileup_sites_device(p._h, 0, len(text), NONZERO, 0, 0, 0, None, None, None, C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(sites_spec.sites(table, text, NONZERO)[0])
    # the wrapper asks again with the need
    same_sites(p.sites(4, 20, capacity=3), want)
    same_sites(p.sites(4, 20, capacity=need), want)
    p.close()
    idx.close()


def test_argument_refusals(eng):
    from slamem_amd import capi
    text, table = planted_table()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    L = capi.lib()
    out = np.zeros(64, dtype=np.uint64)
    total = C.c_uint64()
    o = out.ctypes.data

    def dev_call(first, count, mode, dep, pct):
        return L.slamem_pileup_sites_device(p._h, first, count, mode, dep, pct, 1, o, o, o, C.byref(total), None)

    def host_call(first, count, mode, dep, pct):
        return L.slamem_pileup_sites_host(p._h, first, count, mode, dep, pct, 1, o, o, o, C.byref(total))
    for call in (dev_call, host_call):
        for args in ((n + 1, 0, VARIANT, 4, 20), (n - 3, 4, VARIANT, 4, 20), (0, n + 1, NONZERO, 4, 20), (0, 10, 2, 4, 20),
                     (0, 10, VARIANT, 4, 101), (0, 10, NONZERO, 4, 101), (0, 10, VARIANT, 0, 20), (0, 10, VARIANT, 2 ** 31, 20)):
            assert call(*args) == capi.SLAMEM_ERR_ARG, args
            assert b"slamem_pileup_sites" in L.slamem_last_error_message()
    assert L.slamem_pileup_sites_device(None, 0, 0, 0, 1, 0, 0, None, None, None, C.byref(total), None) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_sites_device(p._h, 0, 10, 0, 1, 0, 0, None, None, None, None, None) == capi.SLAMEM_ERR_ARG
    # mode 0 takes any depth; the largest depth of mode 1 is 2^31 - 1; an empty table selects nothing
    assert host_call(0, n, NONZERO, 0, 100) == capi.SLAMEM_OK and total.value == 0
    assert host_call(0, n, VARIANT, 2 ** 31 - 1, 0) == capi.SLAMEM_OK and total.value == 0
    for bad in (dict(mode=2), dict(min_pct=101), dict(min_depth=0), dict(first=n + 1, count=0)):
        with pytest.raises(capi.SlamemError) as e:
            p.sites(**bad)
        assert e.value.code == capi.SLAMEM_ERR_ARG
    p.close()
    idx.close()


def test_compact_index_is_refused(eng, monkeypatch):
    from slamem_amd import capi
    ref, q, off = indel_reads(13)
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    idx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    assert idx.info.layout == capi.LAYOUT_COMPACT
    with pytest.raises(capi.SlamemError) as e:
        eng.Pileup(idx)
    assert e.value.code == capi.SLAMEM_ERR_ARG
    assert "text planes" in str(e.value) and "compact" in str(e.value) and "-pile" in str(e.value)
    idx.close()


# ---- real mappings -------------------------------------------------------------------------------------------------------------

REAL_RULES = [(VARIANT, 1, 0), (VARIANT, 4, 20), (VARIANT, 2, 100), (NONZERO, 4, 20)]


def halves(q, off):
    h = (len(off) - 1) // 2
    cut = int(off[h])
    return (q[:cut], off[:h + 1].copy()), (q[cut:], (off[h:] - off[h]).astype(np.uint64))


def windows(off, per):
    nq = len(off) - 1
    return [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]


def run_stream(eng, idx, pile, q, wins, slots, min_len):
    st = eng.Stream(idx, slots, 1 << 16, len(wins[0]) - 1, True, pile=pile)
    for b in range(min(slots - 1, len(wins))):
        st.submit(q, wins[b], min_len)
    for b in range(len(wins)):
        st.next()
        if b + slots - 1 < len(wins):
            st.submit(q, wins[b + slots - 1], min_len)
    st.close()


@pytest.mark.parametrize("case", ["indel_reads", "multi_record"])
def test_real_mappings_any_order_and_the_stream(eng, case):
    if case == "indel_reads":
        ref, q, off = indel_reads(21)
        min_len = 14
    else:
        ref, q, off = multi_record_batch()
        min_len = 20
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx)
    recs = p.add(q, off, min_len, True)
    assert int((recs["strand"] == 1).sum()) > 10 and int((recs["strand"] == 2).sum()) > 10
    table = p.counts().astype(np.int64)
    whole = {}
    for mode, dep, pct in REAL_RULES:
        got = p.sites(dep, pct, mode)
        same_sites(got, sites_spec.sites(table, ref, mode, dep, pct), (mode, dep, pct))
        whole[(mode, dep, pct)] = got
    # the comparison is not between empty lists: letters, deletions and (where the reads have them) insertions are called
    alleles = whole[(VARIANT, 1, 0)][2]
    assert bool((alleles & 0x0F).any()) and len(whole[(NONZERO, 4, 20)][0]) > len(alleles) > 0
    if case == "indel_reads":
        assert bool((alleles & 0x10).any()) and bool((alleles & 0x20).any())
        assert len(whole[(VARIANT, 4, 20)][0]) < len(alleles)
    check_all(p, ref, table, rules=[(VARIANT, 1, 0)], ranges=((2037, 4101), (len(ref) - 70, 70)))
    # the halves in the other order
    (qa, oa), (qb, ob) = halves(q, off)
    p.reset()
    p.add(qb, ob, min_len, True)
    p.add(qa, oa, min_len, True)
    for rule, want in whole.items():
        same_sites(p.sites(rule[1], rule[2], rule[0]), want, rule)
    # a stream of match type 8 feeds the accumulator
    p.reset()
    run_stream(eng, idx, p, q, windows(off, (len(off) - 1 + 2) // 3), 2, min_len)
    for rule, want in whole.items():
        same_sites(p.sites(rule[1], rule[2], rule[0]), want, rule)
    # two accumulators, a half each, merged
    a, b = eng.Pileup(idx), eng.Pileup(idx)
    a.add(qa, oa, min_len, True)
    b.add(qb, ob, min_len, True)
    a.add_counts(b.counts())
    assert np.array_equal(a.counts().astype(np.int64), table)
    for rule, want in whole.items():
        same_sites(a.sites(rule[1], rule[2], rule[0]), want, rule)
    for x in (a, b, p):
        x.close()
    idx.close()


def test_planted_substitutions_are_the_sites(eng):
    """A known answer, judged without the spec: a random reference of 12,000 letters, a sample genome with 20 substitutions at
    least 300 letters apart, error-free reads of 150 letters from every fifth position of the sample, alternating strands.
    sites(4, 20) is exactly the 20 planted positions, each with the one bit of the sample's letter, a depth of at least 4 and an
    empty column of the reference letter: every X a mapping holds is a planted letter, and a substitution near a read's end only
    makes that read end earlier.  The seed (test_sites_host.PLANTED_SEED = 20261) is fixed, and
    test_sites_host.test_planted_sample_answer_holds_on_the_definition confirms the answer for it on the CPU (map_spec.filter_reads
    over the oracle's MEM list).  All 20 are required."""
    ref, sample, at, q, off = planted_sample(PLANTED_SEED)
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx)
    recs = p.add(q, off, 20, True)
    assert np.array_equal(recs["strand"], 1 + np.arange(len(off) - 1) % 2)
    pos, counts, alleles = p.sites(4, 20)
    print("planted", list(at), "got", list(pos), counts.tolist(), list(alleles))
    assert planted_answer_holds(ref, sample, at, pos, counts, alleles)
    p.close()
    idx.close()


# ---- the executable ------------------------------------------------------------------------------------------------------------

def write_fasta(path, records):
    with open(path, "wb") as f:
        for name, letters in records:
            f.write(b">" + name + b"\n")
            for a in range(0, len(letters), 70):
                f.write(bytes(letters[a:a + 70]) + b"\n")


def test_cli_file_is_the_spec_of_the_engines_table(eng, tmp_path):
    """slaMEM-hip -b -l 20 -sites -mdep 1 -mpct 0 -minq 1 ref.fa reads.fa: byte for byte the file sites_spec formats from the
    engine's table, on a reference of three records; with two logical GPUs (an accumulator each, added on the device before the
    read-out) the same bytes; at the defaults another file, under the default name."""
    import hostlib
    ref, q, off = multi_record_batch()
    recs = [ref[:3000], ref[3001:8001], ref[8002:]]
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"one first", recs[0]), (b"two\tsecond", recs[1]), (b"three", recs[2])])
    write_fasta(q_fa, [(b"read%d x" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(ref)
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx)
    p.add(q, off, 20, True, min_mapq=1)
    table = p.counts().astype(np.int64)
    p.reset()
    p.add(q, off, 20, True)
    zero = p.counts().astype(np.int64)
    p.close()
    idx.close()
    want = sites_spec.sites_file(table, loaded, 1, 0)
    dflt = sites_spec.sites_file(zero, loaded)
    assert want.count(b"\n") > 20 and want != dflt
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for name, env in (("one", base), ("two", dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1"))):
        out = str(tmp_path / (name + ".txt"))
        r = subprocess.run([EXE, "-b", "-l", "20", "-sites", "-mdep", "1", "-mpct", "0", "-minq", "1", "-o", out, ref_fa, q_fa],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        got = open(out, "rb").read()
        assert got == want and b">" not in got
        assert b"Saving variant sites" in r.stdout and b"; minimum mapping quality = 1 ; minimum depth = 1 ; minimum share = 0 %\n" in r.stdout
    r = subprocess.run([EXE, "-sites", "-b", ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=base, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    assert open(str(tmp_path / "ref-mems.txt"), "rb").read() == dflt
    assert b"; minimum mapping quality = 0 ; minimum depth = 4 ; minimum share = 20 %\n" in r.stdout
