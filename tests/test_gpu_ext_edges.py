"""-ext on the MI355X on the designed batches of tests/ext_edge_cases.py: mismatches, sequence ends and X-drop decisions placed
on the 64-letter windows of walk / window / strand_window, records at every byte offset and on both sides of the lane / listed
pack, strand blocks on both sides of the lane / wave de-duplication with twins up to 65 rows apart.  Every result is
tests/ext_spec.py's filter of the engine's own -mem rows -- rows, block offsets and mismatches exactly equal -- and those -mem rows
are the rows the designs say (tests/test_ext_edge_cases.py holds the same against the oracle), so the edges are reached on the
device.  On the long records and the large blocks the spec runs as extend_side_np, which test_ext_edge_cases.py holds to the
letter-wise rule on every designed row.
The `distances` and `alignment` batches go through -aln as well, whose kernels read the same packed units and windows."""
import numpy as np
import pytest

import aln_spec
import ext_edge_cases as ec
import ext_spec
from conftest import search_path
from test_gpu_aln import assert_equals_blocks
from test_gpu_ext import assert_is_ext_of, triples

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def assert_designed_rows(mem, mem_boff, b: ec.Batch) -> None:
    """The engine's -mem rows are the designed ones, block by block."""
    t, want = triples(mem), ec.expected_blocks(b)
    assert len(mem_boff) == len(want) + 1
    for k, w in enumerate(want):
        g = t[int(mem_boff[k]):int(mem_boff[k + 1])]
        assert np.array_equal(g[np.lexsort((g[:, 2], g[:, 1], g[:, 0]))], w), (b.meta["name"], b.both, k)


def build(eng, design):
    idx = eng.Index.build(design.ref)
    assert ec.MIN_LEN >= int(idx.info.seed_k) + 2   # the fixed minimum length is one the seed path takes on this text
    return idx


@pytest.mark.parametrize("design", ec.designs(), ids=repr)
def test_ext_equals_the_spec(eng, design):
    idx = build(eng, design)
    q, off = design.arrays()
    for both in (True, False):
        found = {}
        for path in ("seed", "walk"):
            with search_path(path):
                found[path] = idx.find_mems(q, off, ec.MIN_LEN, both)
        mem, mem_boff = found["seed"]
        assert np.array_equal(triples(found["walk"][0]), triples(mem)) and np.array_equal(found["walk"][1], mem_boff)
        assert_designed_rows(mem, mem_boff, design.batch(both, *design.params[0]))
        for P, X in design.params:
            got = {}
            for path in ("seed", "walk"):
                with search_path(path):
                    got[path] = idx.find_exts(q, off, ec.MIN_LEN, both, penalty=P, xdrop=X)
                assert eng.timings()["mum_filter_ms"] > 0
            rows, boff, mm = got["seed"]
            # (letter by letter where that is quick; the records of a thousand letters and the blocks of hundreds of rows by numpy)
            assert_is_ext_of(rows, boff, mm, mem, mem_boff, design.ref, q, off, both, P, X, fast=design.family in ("alignment", "blocks"))
            assert np.array_equal(triples(got["walk"][0]), triples(rows)) and np.array_equal(got["walk"][1], boff)
            assert np.array_equal(got["walk"][2], mm)
    idx.close()


@pytest.mark.parametrize("design", ec.designs("blocks"), ids=repr)
def test_blocks_through_a_stream(eng, design):
    """Two batches in flight, a few reads each: a batch's blocks start anywhere in the catalogue's order."""
    idx = build(eng, design)
    q, off = design.arrays()
    mem, mem_boff = idx.find_mems(q, off, ec.MIN_LEN, True)
    want, want_boff, want_mm = ext_spec.filter_blocks(mem, mem_boff, design.ref, q, off, True, fast=True)
    per, nq = 5, len(off) - 1
    wins = [off[b * per: min(nq, (b + 1) * per) + 1].copy() for b in range((nq + per - 1) // per)]
    st = eng.Stream(idx, 3, 1 << 16, per, True, ext=True)
    got, got_mm, got_counts = [], [], []
    st.submit(q, wins[0], ec.MIN_LEN)
    st.submit(q, wins[1], ec.MIN_LEN)
    for b in range(len(wins)):
        m, boff, _ = st.next()
        x = st.mismatches()
        assert len(x) == len(m) == int(boff[-1])
        if b + 2 < len(wins):
            st.submit(q, wins[b + 2], ec.MIN_LEN)
        got.append(triples(m))
        got_mm.append(x.astype(np.int64))
        got_counts.append(np.diff(boff.astype(np.int64)))
    st.close()
    assert np.array_equal(np.concatenate(got_counts), np.diff(want_boff))
    assert np.array_equal(np.concatenate(got), want)
    assert np.array_equal(np.concatenate(got_mm), want_mm)
    idx.close()


@pytest.mark.parametrize("both", [True, False], ids=["both", "forward"])
@pytest.mark.parametrize("design", ec.designs("blocks"), ids=repr)
def test_blocks_at_the_exact_capacity(eng, design, both):
    """A capacity of exactly the -mem rows (one less is refused), guard rows behind both output buffers: the kept rows and
    their mismatches are the spec's, and nothing behind them is written."""
    import torch
    from slamem_amd import capi
    idx = build(eng, design)
    q, off = design.arrays()
    mem, mem_boff = idx.find_mems(q, off, ec.MIN_LEN, both)
    want, want_boff, want_mm = ext_spec.filter_blocks(mem, mem_boff, design.ref, q, off, both, fast=True)
    cap, nq, guard, mark = len(mem), len(off) - 1, 64, 0x5A5A5A5A
    assert len(want) < cap
    qd = torch.zeros((len(q) + 15) // 8 * 8, dtype=torch.uint8, device=idx.device)
    qd[: len(q)] = torch.from_numpy(q).to(idx.device)
    od = torch.from_numpy(off.view(np.int64)).to(idx.device)
    small = idx.matcher(nq, both, cap - 1, int(off[-1]), ext=True)
    with pytest.raises(capi.SlamemError) as e:
        small.run(qd, od, ec.MIN_LEN)
    assert e.value.code == capi.SLAMEM_ERR_CAPACITY and small.last_total == cap
    m = idx.matcher(nq, both, cap, int(off[-1]), ext=True)
    rows_buf = torch.full((cap + guard, 3), mark, dtype=torch.int32, device=idx.device)
    mm_buf = torch.full((cap + guard,), mark, dtype=torch.int32, device=idx.device)
    m.mems, m.mismatches = rows_buf[:cap], mm_buf[:cap]
    total = m.run(qd, od, ec.MIN_LEN)
    assert total == len(want)
    assert np.array_equal(m.block_offsets.cpu().numpy(), want_boff)
    assert np.array_equal(rows_buf[:total].cpu().numpy().view(np.uint32).astype(np.int64), want)
    assert np.array_equal(mm_buf[:total].cpu().numpy().view(np.uint32).astype(np.int64), want_mm)
    assert bool((rows_buf[total:] == mark).all()) and bool((mm_buf[total:] == mark).all())
    idx.close()


@pytest.mark.parametrize("design", ec.designs("distances") + ec.designs("alignment"), ids=repr)
def test_aln_on_the_same_windows(eng, design):
    """k_aln_geom and k_aln_wave read the reads through the same packed units and strand_window: nothing is designed for -aln,
    the result is tests/aln_spec.py's of the engine's -mem rows."""
    idx = build(eng, design)
    q, off = design.arrays()
    for both in (True, False):
        mem, mem_boff = idx.find_mems(q, off, ec.MIN_LEN, both)
        got = idx.find_alns(q, off, ec.MIN_LEN, both, max_edits=31)
        assert_equals_blocks(got, aln_spec.filter_blocks(mem, mem_boff, design.ref, q, off, both, 5000, 4, 20, 31))
    idx.close()
