"""-sv on the MI355X (slamem_pileup_enable_junctions / _junctions_* / _add_junctions_*, engine.Pileup(junctions=True)): every table is
tests/sv_spec.py applied to map_spec.filter_reads of the same engine's -mem list, compared for exact equality -- the designed reads
of tests/sv_cases.py (tests/test_sv_host.py proves on the CPU what each of them yields) and its random batch of planted long indels,
on both search paths, in one add and in two adds in either order, through a stream, under -dedup; planted junctions for the
read-out's ranges, its capacity protocol and a table that is too small."""
import ctypes as C

import numpy as np
import pytest

import sv_cases
import sv_spec as sv
from conftest import search_path
from test_gpu_pile import spec_results
from test_gpu_sites import halves, run_stream, windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


@pytest.fixture(scope="module")
def world(eng):
    """The reference's index and, per batch, the reads, the spec's read_map tuples and the spec's table: computed once."""
    T, cases = sv_cases.catalogue()
    idx = eng.Index.build(T)
    w = dict(T=T, idx=idx, cases=cases)
    q, off = sv_cases.batch(cases)
    w["catalogue"] = (q, off, spec_results(idx, T, q, off, sv_cases.MIN_LEN, True))
    _, q, off, plants = sv_cases.random_batch()
    w["random"] = (q, off, spec_results(idx, T, q, off, sv_cases.MIN_LEN, True))
    w["plants"] = plants
    yield w
    idx.close()


def got_junctions(p, **kw):
    arr, skipped = p.junctions(**kw)
    assert arr.dtype == sv.JUNCTION_DTYPE and not arr["pad"].any()
    return sv.from_records(arr), skipped


def test_dtype_is_the_specs(eng):
    assert eng.JUNCTION_DTYPE == sv.JUNCTION_DTYPE and eng.JUNCTION_DTYPE.itemsize == 24


@pytest.mark.parametrize("path", ["seed", "walk"])
@pytest.mark.parametrize("name", ["catalogue", "random"])
def test_junctions_are_the_specs_on_both_search_paths(eng, world, name, path):
    q, off, res = world[name]
    T, idx = world["T"], world["idx"]
    for mis in (3, 4) if name == "catalogue" else (3,):
        want = sv.junctions(res, q, off, T, mis)
        p = eng.Pileup(idx, junctions=True, junction_max_mis=mis)
        with search_path(path):
            p.add(q, off, sv_cases.MIN_LEN, True)
        got = got_junctions(p)
        print(name, path, mis, len(got[0]), got[1])
        assert got == want
        p.close()
    if name == "catalogue":  # the designed answers themselves, which tests/test_sv_host.py derives without the engine
        assert want == sv_cases.expected_table(world["cases"], "expect4")
    else:
        assert len(want[0]) >= 300 and any(k[1] == 0 for k in want[0]) and any(k[1] == 1 for k in want[0])
        assert any(k[3] for k in want[0]) and any(k[4] for k in want[0])


def test_two_adds_in_either_order_a_stream_and_the_other_tables(eng, world):
    q, off, res = world["catalogue"]
    T, idx = world["T"], world["idx"]
    want = sv.junctions(res, q, off, T)
    (qa, oa), (qb, ob) = halves(q, off)
    plain = eng.Pileup(idx, events=True)
    plain.add(q, off, sv_cases.MIN_LEN, True)
    table, events = plain.counts(), plain.events()
    plain.close()
    p = eng.Pileup(idx, events=True, junctions=True)
    for first, second in (((qa, oa), (qb, ob)), ((qb, ob), (qa, oa))):
        p.reset()
        assert got_junctions(p) == ([], [0, 0, 0, 0])
        p.add(*first, sv_cases.MIN_LEN, True)
        p.add(*second, sv_cases.MIN_LEN, True)
        assert got_junctions(p) == want
    # counts() and events() are those of an accumulator without junctions: the deleted rows get no D
    assert np.array_equal(p.counts(), table)
    ev = p.events()
    assert np.array_equal(ev[0], events[0]) and ev[1] == events[1]
    d = next(k for k in want[0] if k[1] == 0 and k[2] == 300)
    assert not table[d[0] + 20:d[0] + 280, 4].any()
    # a stream of match type 8 with two batches in flight
    p.reset()
    run_stream(eng, idx, p, q, windows(off, (len(off) - 1 + 2) // 3), 3, sv_cases.MIN_LEN)
    assert got_junctions(p) == want and np.array_equal(p.counts(), table)
    # a minimum mapping quality
    p.reset()
    p.add(q, off, sv_cases.MIN_LEN, True, min_mapq=50)
    assert got_junctions(p) == sv.junctions(res, q, off, T, min_mapq=50) != want
    p.close()


def test_read_out_slices_round_trip_and_capacity(eng, world):
    import torch
    from slamem_amd import capi
    q, off, res = world["random"]
    T, idx = world["T"], world["idx"]
    n = len(T)
    spec = sv.Table(T).add_batch(res, q, off)
    spec.add_batch(res[:50], q[:int(off[50])], off[:51])  # (some keys seen twice)
    whole = spec.junctions()
    p = eng.Pileup(idx, junctions=True)
    p.add(q, off, sv_cases.MIN_LEN, True)
    p.add(q[:int(off[50])], off[:51].copy(), sv_cases.MIN_LEN, True)
    assert got_junctions(p) == (whole, spec.skipped)
    # min_len, min_count and sub-ranges are slices of the whole read-out
    mid = whole[len(whole) // 2][0]
    for kw in (dict(min_len=131), dict(min_len=1000), dict(min_len=2001), dict(min_count=2), dict(min_count=3), dict(first=mid),
               dict(first=mid + 1), dict(first=mid, count=1), dict(first=0, count=mid), dict(first=n, count=0), dict(first=0, count=0),
               dict(min_len=800, min_count=2, first=3000, count=30000)):
        want = [k for k in whole if kw.get("first", 0) <= k[0] < kw.get("first", 0) + kw.get("count", n - kw.get("first", 0))
                and k[3] + k[4] >= kw.get("min_count", 1) and k[2] >= kw.get("min_len", 1)]
        assert want == spec.junctions(kw.get("first", 0), kw.get("count"), kw.get("min_count", 1), kw.get("min_len", 1))
        assert got_junctions(p, **kw)[0] == want, kw
    assert len(spec.junctions(min_count=2)) >= 20 and spec.junctions(min_len=2001) == [] and 0 < len(spec.junctions(min_len=1000)) < len(whole)
    assert got_junctions(p)[0] == whole  # (the read-out left the table alone)
    # the capacity protocol, with guard rows behind the output
    L = capi.lib()
    dev = idx.device
    cap = 7
    buf = torch.full(((cap + 4) * 24,), 0x5A, dtype=torch.uint8, device=dev)
    total, sk = C.c_uint64(), (C.c_uint64 * 4)()
    rc = L.slamem_pileup_junctions_device(p._h, 0, n, 1, 1, cap, buf.data_ptr(), sk, C.byref(total), None)
    torch.cuda.synchronize()
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(whole) and b"selected" in L.slamem_last_error_message()
    assert bool((buf[cap * 24:] == 0x5A).all())
    assert sv.from_records(buf[:cap * 24].cpu().numpy().view(sv.JUNCTION_DTYPE)) == whole[:cap]
    rc = L.slamem_pileup_junctions_device(p._h, 0, n, 1, 1, 0, None, sk, C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(whole) and list(sk) == spec.skipped
    host = np.zeros(len(whole) + 2, dtype=sv.JUNCTION_DTYPE)
    rc = L.slamem_pileup_junctions_host(p._h, 0, n, 1, 1, 3, host.ctypes.data, sk, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(whole) and sv.from_records(host[:3]) == whole[:3] and not host[3:]["len"].any()
    rc = L.slamem_pileup_junctions_host(p._h, 0, n, 1, 1, len(host), host.ctypes.data, sk, C.byref(total))
    assert rc == capi.SLAMEM_OK and sv.from_records(host[:total.value]) == whole
    assert got_junctions(p, capacity=3)[0] == whole
    # add_junctions round-trips a read-out into a fresh accumulator, through the device call and the host call
    a, b = eng.Pileup(idx, junctions=True, junction_slots=1024), eng.Pileup(idx, junctions=True)
    a.add_junctions(p.junctions()[0])
    assert L.slamem_pileup_add_junctions_host(b._h, host.ctypes.data, len(whole)) == capi.SLAMEM_OK
    assert got_junctions(a) == (whole, [0, 0, 0, 0]) == got_junctions(b)
    # ... and twice the table is twice the counts
    a.add_junctions(p.junctions()[0])
    assert got_junctions(a)[0] == [k[:3] + (2 * k[3], 2 * k[4]) for k in whole]
    # reset clears the table and its counters
    p.reset()
    assert got_junctions(p) == ([], [0, 0, 0, 0])
    # refusals
    for bad in (dict(first=n + 1, count=0), dict(first=n - 1, count=2), dict(min_count=0)):
        with pytest.raises(capi.SlamemError) as err:
            p.junctions(**bad)
        assert err.value.code == capi.SLAMEM_ERR_ARG
    plain = eng.Pileup(idx)
    for call in (lambda: plain.junctions(), lambda: plain.add_junctions(sv.to_records(whole[:1]))):
        with pytest.raises(capi.SlamemError) as err:
            call()
        assert err.value.code == capi.SLAMEM_ERR_ARG and "not enabled" in str(err.value)
    assert L.slamem_pileup_enable_junctions(p._h, 64, 3) == capi.SLAMEM_ERR_ARG and b"already" in L.slamem_last_error_message()
    for slots, mis in ((63, 3), (32, 3), (100, 3), (2 ** 32, 3), (64, 65)):
        assert L.slamem_pileup_enable_junctions(plain._h, slots, mis) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_enable_junctions(plain._h, 0, 0) == capi.SLAMEM_OK  # the default size
    assert got_junctions(plain) == ([], [0, 0, 0, 0])
    with pytest.raises(ValueError):
        eng.Pileup(idx, junction_slots=64)
    for x in (a, b, p, plain):
        x.close()


def test_planted_junctions_follow_the_planting_rule(eng, world):
    T, idx = world["T"], world["idx"]
    n = len(T)
    R = sv_cases.REPEAT
    plants = [(R + 100, 0, 40, 1, 0), (R + 41, 0, 40, 0, 2), (R, 0, 40, 3, 0),          # one deletion inside the repeat
              (R + 100, 1, 40, 1, 0), (R + 100, 1, 40, 0, 1), (R + 100, 1, 41, 1, 0),   # insertions stay where they are given
              (500, 0, 5000, 1, 1), (500, 1, 100000, 2, 0),                             # any length
              (sv_cases.SEPARATOR - 10, 0, 20, 1, 0), (sv_cases.PLANTED_N, 0, 1, 0, 3), # over an N
              (n - 5, 0, 6, 1, 0), (n, 1, 3, 1, 0), (n, 0, 1, 1, 0),                    # beyond n, at n
              (700, 0, 0, 1, 0), (700, 1, 0, 1, 0), (700, 0, 3, 0, 0),                  # no length; no observation
              (n - 5, 0, 5, 0, 1), (0, 0, 1, 1, 0), (0, 1, 1, 1, 0), (n - 1, 1, 7, 1, 0)]
    spec = sv.Table(T)
    for j in plants:
        spec.observe(*j)
    assert spec.skipped == [0, 0, 9, 0] and (R, 0, 40) in spec.keys and spec.keys[(R, 0, 40)] == [4, 2]
    recs = sv.to_records(plants)
    bad_kind = sv.to_records([(700, 0, 3, 2, 2)])
    bad_kind["kind"] = 2
    spec.observe(700, 2, 3, 2, 2)
    p = eng.Pileup(idx, junctions=True, junction_slots=64)
    p.add_junctions(np.concatenate([recs, bad_kind]))
    assert got_junctions(p) == (spec.junctions(), spec.skipped)
    p.add_junctions(recs[:0])
    assert got_junctions(p) == (spec.junctions(), spec.skipped)
    p.close()


def test_full_table_counts_what_it_could_not_store(eng, world):
    T, idx = world["T"], world["idx"]
    rng = np.random.default_rng(53)
    plants = [(1000 + 7 * k, 1, 200 + k, int(rng.integers(1, 9)), int(rng.integers(0, 9))) for k in range(200)]
    p = eng.Pileup(idx, junctions=True, junction_slots=64)
    p.add_junctions(sv.to_records(plants))
    p.add_junctions(sv.to_records(plants))
    got, skipped = got_junctions(p)
    counts = {j[:3]: j[3:] for j in plants}
    assert 0 < len(got) <= 64 and skipped[0] == skipped[2] == skipped[3] == 0 and skipped[1] > 0
    for g in got:  # every key that got in carries its exact counts
        assert g[3:] == (2 * counts[g[:3]][0], 2 * counts[g[:3]][1])
    assert sum(g[3] + g[4] for g in got) + skipped[1] == 2 * sum(j[3] + j[4] for j in plants)
    p.close()
    # the same through an add of reads: stored plus skipped is what the spec observed
    q, off, res = world["random"]
    spec = sv.Table(T).add_batch(res, q, off)
    p = eng.Pileup(idx, junctions=True, junction_slots=64)
    p.add(q, off, sv_cases.MIN_LEN, True)
    got, skipped = got_junctions(p)
    assert len(spec.keys) > 64 and 0 < len(got) <= 64 and skipped[1] > 0
    assert [skipped[0], skipped[2], skipped[3]] == [spec.skipped[0], spec.skipped[2], spec.skipped[3]]
    assert all(list(g[3:]) == spec.keys[g[:3]] for g in got)
    assert sum(g[3] + g[4] for g in got) + sum(skipped) == spec.observed
    p.close()


def test_duplicates_leave_no_junction(eng, world):
    """The catalogue twice in one batch under -dedup: every read's second copy is a duplicate of the first (its flag says so), and
    the table is that of the reads the filter keeps."""
    q, off, res = world["catalogue"]
    T, idx = world["T"], world["idx"]
    q2 = np.concatenate([q, q])
    off2 = np.concatenate([off, off[1:] + off[-1]]).astype(np.uint64)
    p = eng.Pileup(idx, junctions=True, dedup=True)
    recs, dup = p.add(q2, off2, sv_cases.MIN_LEN, True, dedup=True)
    nq = len(off) - 1
    assert not dup[:nq].any() and int((dup[nq:] == 1).sum()) == nq
    kept = [r if dup[i] != 1 else (0, 0, 0, 0, []) for i, r in enumerate(res + res)]
    want = sv.junctions(kept, q2, off2, T)
    assert want == sv.junctions(res, q, off, T)
    assert got_junctions(p) == want
    p.close()
    # without the filter both copies count
    p = eng.Pileup(idx, junctions=True)
    p.add(q2, off2, sv_cases.MIN_LEN, True)
    assert got_junctions(p) == sv.junctions(res + res, q2, off2, T)
    p.close()


# ---- the executable ------------------------------------------------------------------------------------------------------------

def test_cli_file_is_the_spec_of_the_engines_tables(eng, world, tmp_path):
    """slaMEM-hip -b -l 20 -vcf -sv -mdep 1 -mpct 0 ref.fa reads.fa on the catalogue (the reference's two records): byte for byte the
    file sv_spec formats from the engine's pileup, events and junctions; the same with two logical GPUs (the junctions of GPU 1
    merged into GPU 0's) and with a small table given by -svslots; -svmin and -svmis move what is written; the same command
    without -sv writes the file of 4.18."""
    import os
    import subprocess

    import events_spec as es
    import hostlib
    from test_gpu_sites import write_fasta
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slamem_amd", "host", "slaMEM-hip")
    q, off, res = world["catalogue"]
    T, idx = world["T"], world["idx"]
    sep = sv_cases.SEPARATOR
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"one first", T[:sep]), (b"two\tsecond", T[sep + 1:])])
    write_fasta(q_fa, [(b"read%d x" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(T)
    tables = {}
    for mis in (3, 4):
        p = eng.Pileup(idx, events=True, junctions=True, junction_max_mis=mis)
        p.add(q, off, sv_cases.MIN_LEN, True)
        tables[mis] = (p.counts().astype(np.int64), es.from_records(p.events()[0]), got_junctions(p)[0])
        p.close()
    table, ev, jn = tables[3]
    assert jn == sv.junctions(res, q, off, T)[0]
    want = sv.vcf_file(table, ev, jn, loaded, 1, 0)
    plain = es.vcf_file(table, ev, loaded, 1, 0)
    # 12 deletions and 3 insertions are stored; the anchors of mis_a3, mis_a20 and mis3 lie among the letters that both segments own,
    # which no segment piles: depth 0 there, so the rule of 4.18 does not call them even at -mdep 1
    assert len(jn) == 15 and want.count(b"SVTYPE=DEL") == 9 and want.count(b"SVTYPE=INS") == 3 and want.startswith(sv.vcf_header(loaded))
    assert b"\none\t" in want and want != sv.vcf_file(table, ev, jn, loaded)
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    runs = [("one", base, [], want, b"; sv min = 32\n"),
            ("two", dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1"), [], want, b"; sv min = 32\n"),
            ("slots", base, ["-svslots", "4096"], want, b"; sv min = 32\n"),
            ("min41", base, ["-svmin", "41"], sv.vcf_file(table, ev, jn, loaded, 1, 0, 41), b"; sv min = 41\n"),
            ("mis4", base, ["-svmis", "4"], sv.vcf_file(*tables[4], loaded, 1, 0), b"; sv min = 32\n"),
            ("maxed", base, ["-maxed", "20"], None, b"; sv min = 21\n")]
    for name, env, extra, file, line in runs:
        out = str(tmp_path / (name + ".vcf"))
        r = subprocess.run([exe, "-b", "-l", "20", "-vcf", "-sv", "-mdep", "1", "-mpct", "0", "-o", out] + extra + [ref_fa, q_fa],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert file is None or open(out, "rb").read() == file, name
        assert line in r.stdout and b"> Junctions: " in r.stderr and b"WARNING" not in r.stderr, name
        if name in ("one", "two"):
            assert (b"> Junctions: %d stored, 12 lines written, 0 at a record's first row left out; not stored: 2 balanced, 0 without "
                    b"room in the table, 6 with a letter that is none of A,C,G,T, 4 with more than 64 shared letters or too many "
                    b"mismatches\n" % len(jn)) in r.stderr, r.stderr
    # -svmin 41 drops lines; -svmis 4 stores slop64's junction as well (its anchor lies among the shared letters: stored, not written)
    assert len(sv.vcf_file(table, ev, jn, loaded, 1, 0, 41)) < len(want) and len(tables[4][2]) == len(jn) + 1
    # the same command without -sv: the bytes of 4.18
    out = str(tmp_path / "plain.vcf")
    r = subprocess.run([exe, "-b", "-l", "20", "-vcf", "-mdep", "1", "-mpct", "0", "-o", out, ref_fa, q_fa], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=base, timeout=300)
    assert r.returncode == 0 and open(out, "rb").read() == plain
    assert b"sv min" not in r.stdout and b"Junctions" not in r.stderr
