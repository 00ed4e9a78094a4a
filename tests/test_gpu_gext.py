"""-gext on the MI355X: k_aln_wave_ends and the inline rule (c) of k_aln_geom held to tests/gext_spec.py -- every
result compared for exact equality with the definition applied to the complete -mem list of the same engine -- through
find_alns, map_reads, the pileup with events, MapStats and both kinds of stream, on the designed ends of
tests/gext_end_cases.py; and end_band = 0 against the -affine path as it was."""
import numpy as np
import pytest

import affine_spec
import aln_spec
import events_spec
import gext_end_cases as cases
import gext_spec
import map_spec
import pile_spec
import sam_spec
from test_gpu_affine import run_stream
from test_gpu_aln import assert_equals_blocks
from test_gpu_events import got_events
from test_gpu_map import assert_equals_reads, rec_rows
from test_gpu_pile import same

pytestmark = pytest.mark.gpu

DEFAULT = (4, 6, 2)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def spec_reads(mem, boff, ref, q, off, costs, Z):
    with gext_spec.in_aln_spec(costs, Z):
        return map_spec.filter_reads(mem, boff, ref, q, off, True)


@pytest.fixture(scope="module")
def cat(eng):
    """The catalogue at Z = 8, the engine's -mem rows, and the spec's blocks and ends per band: once."""
    ref, q, off, labels = cases.catalogue(8)
    idx = eng.Index.build(ref)
    mem, boff = idx.find_mems(q, off, cases.MIN_LEN, True)
    want = {}
    for Z in (1, 8, 31):
        ends = []
        want[Z] = (gext_spec.filter_blocks(mem, boff, ref, q, off, True, costs=DEFAULT, Z=Z, ends_out=ends), ends)
    yield idx, ref, q, off, labels, mem, boff, want
    idx.close()


@pytest.mark.parametrize("Z", [1, 8, 31])
def test_designed_ends(eng, cat, Z):
    idx, ref, q, off, labels, mem, boff, want = cat
    blocks, ends = want[Z]
    assert_equals_blocks(idx.find_alns(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=Z), blocks)
    assert_equals_reads(idx.map_reads(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=Z),
                        spec_reads(mem, boff, ref, q, off, DEFAULT, Z))
    replaced = [e for e in ends if e["replaced"]]
    assert any(e["side"] < 0 for e in replaced) and any(e["side"] > 0 for e in replaced)
    assert any("I" in e["ops"] for e in replaced) and any("D" in e["ops"] for e in replaced)


def ends_of_read(ends, mem, boff, k):
    """The spec's end records of read k: two per strand block that has rows, in block order."""
    has = [int(boff[b + 1]) > int(boff[b]) for b in range(len(boff) - 1)]
    first = 2 * sum(has[:2 * k])
    return ends[first:first + 2 * sum(has[2 * k:2 * k + 2])]


def test_the_catalogue_meets_its_edges(cat):
    """Asserted from the spec at Z = 8 on the engine's rows."""
    idx, ref, q, off, labels, mem, boff, want = cat
    blocks, ends = want[8]
    replaced = [e for e in ends if e["replaced"]]
    listed = [e for e in ends if e.get("listed")]
    # indels of 1 and 2 letters at 12, 19 and 25 letters from either end score d - (6 + 2 L) > 0, more than the side behind an indel
    assert len(replaced) >= 20 and len(listed) > len(replaced)
    assert any(e["listed"] and not e["replaced"] and e["gapped"] == e["ungapped"] for e in listed)      # a tie keeps the ungapped side
    assert any(e["hit_cost_max"] for e in listed)                                                       # an end that passes Cp
    assert any(e["replaced"] and "X" in e["ops"] for e in replaced)                                     # an indel plus a mismatch
    assert any(e["b"] < e["a"] for e in listed)                                                         # B clamped by the text or a border
    # the named cases, by label: the end of read k on the side the case was built for is ends[4 k + 2 strand + side]
    at = {l.split(":rc")[0]: (k, l.endswith(":rc")) for k, l in enumerate(labels)}

    def end_of(label):
        return ends_of_read(ends, mem, boff, at[label][0])
    for label in ("text-start", "text-end", "record-border", "record-border:left"):                    # each of the four clamps
        assert any(e.get("listed") and e["b"] < e["a"] for e in end_of(label)), label
    for label in ("homopolymer:D", "homopolymer:D:left", "repeat:AC:D"):
        assert any(e["replaced"] and "D" in e["ops"] for e in end_of(label)), label
    assert any(e.get("a") == 18 and not e["replaced"] for e in end_of("repeat:AC:D:left"))  # (there the ungapped side scores more)
    # the N in the tail, 5 letters from the end behind a deletion 23 from it: A is the 18 letters up to the N
    # (17 when the deleted letter equals its neighbour and the MEM runs one letter on); the gapped end takes all of A
    assert any(e["replaced"] and e["a"] in (17, 18) and "D" in e["ops"] and len(e["ops"]) - e["ops"].count("D") == e["a"]
               for e in end_of("D1@23+N@5"))
    for n in (63, 64, 65, 127, 128, 129):                                                               # long tails without a MEM
        assert any(e["replaced"] and len(e["ops"]) - e["ops"].count("D") == n for e in replaced), n
    runs = lambda e: [n for c, n in aln_spec.runs(e["ops"]) if c in "ID"]
    assert {1, 2} <= {n for e in replaced for n in runs(e)}
    # an indel whose cost is above the drop (Z and Z + 1 letters at costs 4,6,2 and X = 20) is not found: no run that long
    assert max(n for e in replaced for n in runs(e)) <= (20 - 6) // 2


def test_more_listed_ends_than_workgroups_at_band_31(eng, cat):
    """400 reads with a listed end each on the 173 one-wave workgroups that the slab rule admits at Z = 31: every workgroup
    runs a second and a third end in the same LDS and slab."""
    idx, ref = cat[0], cat[1]
    bref, q, off = cases.bulk(400)
    assert np.array_equal(bref, ref)
    mem, boff = idx.find_mems(q, off, cases.MIN_LEN, True)
    ends = []
    want = gext_spec.filter_blocks(mem, boff, ref, q, off, True, costs=DEFAULT, Z=31, ends_out=ends)
    assert_equals_blocks(idx.find_alns(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=31), want)
    assert sum(bool(e.get("listed")) for e in ends) >= 390 and sum(e["replaced"] for e in ends) >= 380  # (390 > 2 * 173)


def test_band_0_is_the_affine_path(eng, cat):
    idx, ref, q, off, labels, mem, boff, want = cat
    was = affine_spec.filter_blocks(mem, boff, ref, q, off, True, costs=DEFAULT)
    got = idx.find_alns(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=0)
    assert_equals_blocks(got, was)
    for a, b in zip(got, idx.find_alns(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    ref2, q2, off2 = aln_spec.constructed_reads(11)[:3]
    idx2 = eng.Index.build(ref2)
    for a, b in zip(idx2.find_alns(q2, off2, 20, True, gap_costs=DEFAULT, end_band=0), idx2.find_alns(q2, off2, 20, True, gap_costs=DEFAULT)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    m2, b2 = idx2.find_mems(q2, off2, 20, True)
    assert_equals_blocks(idx2.find_alns(q2, off2, 20, True, gap_costs=DEFAULT, end_band=8),
                         gext_spec.filter_blocks(m2, b2, ref2, q2, off2, True, costs=DEFAULT, Z=8))
    idx2.close()


def test_pileup_events_and_map_stats(eng, cat):
    """The event of an end's indel is there with end_band and absent without it."""
    idx, ref, q, off, labels, mem, boff, want = cat
    found = {}
    for Z in (0, 8):
        res = spec_reads(mem, boff, ref, q, off, DEFAULT, Z)
        p = eng.Pileup(idx, events=True)
        recs = p.add(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=Z)
        assert np.array_equal(rec_rows(recs), map_spec.pack(res)[4])
        same(p.counts(), pile_spec.pile(res, q, off, len(ref)))
        ev = events_spec.events(res, q, off, ref)
        assert got_events(p) == ev
        found[Z] = len(ev[0])
        p.close()
    assert found[8] >= found[0] + 20  # (the 20 replaced ends of test_the_catalogue_meets_its_edges lie in windows of their own)
    got = idx.map_reads(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=8)
    a, b = eng.MapStats(idx), eng.MapStats(idx)
    recs = a.add(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=8)
    b.add_mapped(q, off, got)
    assert np.array_equal(rec_rows(recs), rec_rows(got[4])) and np.array_equal(a.raw(), b.raw())
    a.close(); b.close()


@pytest.mark.parametrize("mode", ["aln", "paf"])
def test_streams(eng, cat, mode):
    idx, ref, q, off, labels, mem, boff, want = cat
    keep = len(labels) - 1  # (the long record does not fit the stream's batches)
    q, off = q[:int(off[keep])], off[:keep + 1]
    mem, boff = idx.find_mems(q, off, cases.MIN_LEN, True)
    if mode == "aln":
        w_segs, w_boff, w_ops, w_ooff = aln_spec.pack(gext_spec.filter_blocks(mem, boff, ref, q, off, True, costs=DEFAULT, Z=8))
    else:
        w_segs, w_boff, w_ops, w_ooff, w_reads = map_spec.pack(spec_reads(mem, boff, ref, q, off, DEFAULT, 8))
    segs, counts, ops, nops, reads = run_stream(eng, idx, q, off, 29, gap_costs=DEFAULT, end_band=8, **{mode: True})
    assert np.array_equal(segs, w_segs) and np.array_equal(counts, np.diff(w_boff))
    assert np.array_equal(ops, w_ops) and np.array_equal(nops, np.diff(w_ooff))
    if mode == "paf":
        assert np.array_equal(np.concatenate(reads), w_reads)


def test_refusals(eng, cat):
    from slamem_amd import capi
    idx, ref, q, off = cat[:4]
    with pytest.raises(ValueError):
        idx.find_alns(q, off, 20, True, end_band=8)
    with pytest.raises(ValueError):
        idx.find_alns(q, off, 20, True, gap_costs=DEFAULT, end_band=32)
    with pytest.raises(ValueError):
        eng.Stream(idx, 2, 1 << 12, 8, True, aln=True, end_band=8)
    with pytest.raises(capi.SlamemError) as e:  # past the Python check
        idx._aln_like(q, off, 20, True, 0, 0, None, 31, None, False, end_band=8)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "end band" in str(e.value)
    L = capi.lib()
    st = eng.Stream(idx, 2, 1 << 12, 8, True, aln=True)
    assert L.slamem_stream_set_end_band(st._h, 8) == capi.SLAMEM_ERR_ARG  # no costs yet
    assert L.slamem_stream_set_max_edits(st._h, affine_spec.aln_word(31, DEFAULT)) == capi.SLAMEM_OK
    assert L.slamem_stream_set_end_band(st._h, 32) == capi.SLAMEM_ERR_ARG
    assert L.slamem_stream_set_end_band(st._h, 31) == capi.SLAMEM_OK
    assert L.slamem_stream_set_max_edits(st._h, 31) == capi.SLAMEM_ERR_ARG  # a word without costs under a band that is set
    assert L.slamem_stream_set_max_edits(st._h, affine_spec.aln_word(64, DEFAULT)) == capi.SLAMEM_OK
    st.close()


# ---- the executable ----------------------------------------------------------------------------------------------------------------

def test_executable_with_and_without_the_option(eng, cat, tmp_path):
    """slaMEM-hip -b -l 20 -aln -affine 4,6,2 on the catalogue: with -gext 8 the file of the spec at Z = 8 and the parameter line
    with the band, without it the file and the parameter line of before; -sam carries the end's indel in its CIGAR."""
    import hostlib
    from test_gpu_affine import run_exe
    from test_gpu_pile import write_fasta
    idx, cref, q, off, labels, mem, boff, want = cat
    ref_fa, q_fa, out = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), str(tmp_path / "out.txt")
    write_fasta(ref_fa, [(b"designed", cref[:cases.N_AT]), (b"second", cref[cases.N_AT + 1:])])
    write_fasta(q_fa, [(b"r%d %s" % (k, labels[k].encode()), q[int(off[k]):int(off[k + 1])]) for k in range(len(labels))])
    ref, qs = hostlib.Loaded(ref_fa, 1), hostlib.Loaded(q_fa, 0)
    assert np.array_equal(np.frombuffer(ref.chars, dtype=np.uint8) & 0xDF == ord("N"), cref == ord("N"))
    files = {}
    for Z in (8, 0):
        blocks = want[8][0] if Z else affine_spec.filter_blocks(mem, boff, cref, q, off, True, costs=DEFAULT)
        files[Z] = affine_spec.aln_file(qs.names, blocks, ref, 2)
        stdout = run_exe(["-b", "-l", "20", "-aln", "-affine", "4,6,2"] + (["-gext", "8"] if Z else []) + ["-o", out, ref_fa, q_fa])
        assert open(out, "rb").read() == files[Z]
        assert (b"; gap costs = 4,6,2 ; end band = 8\n" if Z else b"; gap costs = 4,6,2\n") in stdout
        assert (b"end band" in stdout) == bool(Z)
    assert files[0] != files[8]
    # -sam: the spec's mapping through the spec's SAM writer, byte for byte, and through the replay checker (POS, soft clips, NM, MD,
    # s1, s2 and SA of ends that hold I and D)
    letters = [qs.chars[qs.offsets[i]:qs.offsets[i + 1]] for i in range(qs.n)]
    sams = {}
    for Z in (8, 0):
        results = spec_reads(mem, boff, cref, q, off, DEFAULT, Z) if Z else affine_reads(mem, boff, cref, q, off)
        run_exe(["-b", "-l", "20", "-sam", "-affine", "4,6,2"] + (["-gext", "8"] if Z else []) + ["-o", out, ref_fa, q_fa])
        sams[Z] = open(out, "rb").read()
        assert sams[Z] == sam_spec.sam_file(results, qs.names, letters, None, ref)
        assert sam_spec.replay_check(sams[Z], ref, qs.names, letters, results) == sum(len(x[4]) for x in results if x[0])
    assert sams[0] != sams[8]


def affine_reads(mem, boff, ref, q, off):
    with affine_spec.in_aln_spec(DEFAULT):
        return map_spec.filter_reads(mem, boff, ref, q, off, True)


def test_md_pass_over_replaced_ends(eng, cat):
    """map_reads(md=True): the MD entries, the letters under = and the primary segments of ends where ref_len != query_len; the
    same through slamem_find_maps_md_host_gext, called as C callers call it."""
    import ctypes as C
    from slamem_amd import capi
    from test_gpu_sam import assert_md_equals
    idx, ref, q, off, labels, mem, boff, want = cat
    reads = spec_reads(mem, boff, ref, q, off, DEFAULT, 8)
    assert sum(s[2] != s[3] for r in reads for s in r[4]) >= 20
    got = idx.map_reads(q, off, cases.MIN_LEN, True, md=True, gap_costs=DEFAULT, end_band=8)
    assert_md_equals(got, reads, bytes(ref))
    L = capi.lib()
    vp = C.c_void_p
    segs, roff, ops, ooff, recs, md, moff, eq, prim = (vp() for _ in range(9))
    totals, nmd = (C.c_uint64 * 3)(), C.c_uint64()
    offs = np.ascontiguousarray(off, dtype=np.uint64)
    capi.check(L.slamem_find_maps_md_host_gext(idx._h, bytes(q), offs.ctypes.data_as(vp), len(offs) - 1, cases.MIN_LEN, 1, 0, 0,
                                               0xFFFFFFFF, affine_spec.aln_word(31, DEFAULT), 8, C.byref(segs), C.byref(roff), C.byref(ops),
                                               C.byref(ooff), C.byref(recs), totals, C.byref(md), C.byref(moff), C.byref(eq), C.byref(prim),
                                               C.byref(nmd)))
    nseg, nops = int(totals[1]), int(totals[2])
    view = lambda ptr, n, t: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(t)), shape=(n,)).copy()
    assert np.array_equal(view(segs, nseg * 5, C.c_uint32), got[0].view(np.uint32).reshape(-1))
    assert np.array_equal(view(ops, nops, C.c_uint32), got[2]) and np.array_equal(view(md, int(nmd.value), C.c_uint32), got[5])
    assert np.array_equal(view(roff, len(offs), C.c_uint64), got[1]) and np.array_equal(view(prim, len(offs) - 1, C.c_uint32), got[8])
    for ptr in (segs, roff, ops, ooff, recs, md, moff, eq, prim):
        L.slamem_host_free(ptr)
    # and slamem_find_alns_host_gext
    totals = (C.c_uint64 * 3)()
    segs, boffp, ops, ooff = (vp() for _ in range(4))
    capi.check(L.slamem_find_alns_host_gext(idx._h, bytes(q), offs.ctypes.data_as(vp), len(offs) - 1, cases.MIN_LEN, 1, 0, 0, 0xFFFFFFFF,
                                            affine_spec.aln_word(31, DEFAULT), 8, C.byref(segs), C.byref(boffp), C.byref(ops), C.byref(ooff),
                                            totals))
    alns = idx.find_alns(q, off, cases.MIN_LEN, True, gap_costs=DEFAULT, end_band=8)
    assert np.array_equal(view(segs, int(totals[1]) * 5, C.c_uint32), alns[0].view(np.uint32).reshape(-1))
    assert np.array_equal(view(ops, int(totals[2]), C.c_uint32), alns[2])
    for ptr in (segs, boffp, ops, ooff):
        L.slamem_host_free(ptr)


@pytest.mark.parametrize("costs,P,X,Z", [((1, 0, 1), 1, 60, 8), ((5, 10, 1), 4, 60, 8), ((1, 0, 1), 1, 200, 31), ((4, 6, 2), 6, 10, 8)])
def test_other_costs_penalties_and_drops(eng, costs, P, X, Z):
    """Other shapes of the penalty: o = 0 (o' + e' = 3 < x'), a cheap gap letter, a drop under which gaps of Z letters are found
    and those of Z + 1 are not, because the band decides (the catalogue built for that Z), and a small drop with another -pen."""
    ref, q, off, labels = cases.catalogue(Z)
    idx = eng.Index.build(ref)
    mem, boff = idx.find_mems(q, off, cases.MIN_LEN, True)
    ends = []
    want = gext_spec.filter_blocks(mem, boff, ref, q, off, True, P=P, X=X, costs=costs, Z=Z, ends_out=ends)
    assert_equals_blocks(idx.find_alns(q, off, cases.MIN_LEN, True, penalty=P, xdrop=X, gap_costs=costs, end_band=Z), want)
    longest = max([n for e in ends if e["replaced"] for c, n in aln_spec.runs(e["ops"]) if c in "ID"], default=0)
    assert sum(e["replaced"] for e in ends) >= 10
    if X >= 60:  # a gap of Z letters is found, one of Z + 1 is not: the band's clamp decided
        assert longest == Z
    idx.close()


def test_end_counts(eng, cat):
    """slamem_find_alns_end_counts_device: the ends the kernels listed and replaced, against the spec's."""
    import ctypes as C
    import torch
    from slamem_amd import capi
    from slamem_amd.engine import _ptr
    idx, ref, q, off, labels, mem, boff, want = cat
    ends = want[8][1]
    L = capi.lib()
    dev = idx.device
    num, qbytes = len(off) - 1, int(off[-1])
    qd = torch.zeros((len(q) + 15) // 8 * 8, dtype=torch.uint8, device=dev)
    qd[:len(q)] = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    od = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).to(dev)
    cap, scap, ocap, word = 4096, 4096, 16384, affine_spec.aln_word(31, DEFAULT)
    need = C.c_uint64()
    capi.check(L.slamem_find_alns_workspace_bytes_gext(num, 1, qbytes, cap, ocap, word, 8, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    segs = torch.zeros((scap + 1) * 5, dtype=torch.int32, device=dev)
    ops = torch.zeros(ocap + 1, dtype=torch.int32, device=dev)
    ooff = torch.zeros(scap + 2, dtype=torch.int64, device=dev)
    bo = torch.zeros(2 * num + 1, dtype=torch.int64, device=dev)
    totals, counts = (C.c_uint64 * 3)(), (C.c_uint64 * 2)()
    torch.cuda.synchronize()
    capi.check(L.slamem_find_alns_device_gext(idx._h, _ptr(qd), _ptr(od), num, qbytes, cases.MIN_LEN, 1, 0, 0, 0xFFFFFFFF, word, 8, cap,
                                              _ptr(segs), scap, _ptr(bo), _ptr(ops), ocap, _ptr(ooff), _ptr(ws), need.value, None, totals))
    capi.check(L.slamem_find_alns_end_counts_device(num, 1, qbytes, cap, ocap, word, 8, _ptr(ws), None, counts))
    replaced = sum(e["replaced"] for e in ends)
    # (k_aln_geom lists every end the spec lists -- fact (c) with a known -- and those whose a it does not know)
    assert counts[1] == replaced and sum(bool(e.get("listed")) for e in ends) <= counts[0] <= len(ends)
