"""-chain, -smem and -mum on the designed -mem lists of tests/filter_list_cases.py, through the door of tests/filters.py: the
product's filters (libslamem_hip.so behind tests/filters/libfilters_shim.so) on lists that sit on their block-size limits --
32/33 and 1024/1025 rows for -chain, 256/257 and 2048/2049 for -smem, 256/257 for -mum -- with predecessors a trip or a tile
away, windows that end on the 64th row, containers in the neighbouring thread's rows, runs across a tile edge under a cap,
coordinates above 2^31 and ends above 2^32.  tests/test_filter_list_cases.py asserts that the lists are what this says.

Every comparison is exact: kept rows, new block offsets, the scalars and -chain's scores against chain_spec / smem_spec /
mum_spec.  filters.run() checks the guards of every buffer and that no output row behind the kept ones was written.

host_scalars[1] of -chain and -smem: the HIGHEST-numbered block out of the emission order + 1 (the kernels take an atomic
maximum); test_out_of_order pins that, and that such a block contributes no rows while every other block is the spec's.
"""
import numpy as np
import pytest

import filter_list_cases as fc
import filters

pytestmark = pytest.mark.gpu

TYPE = {"mum": filters.MUM, "smem": filters.SMEM, "chain": filters.CHAIN}


@pytest.fixture(scope="module")
def door():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (there is no CPU path)")
    return filters.lib()


def first_diff(got: np.ndarray, want: np.ndarray, what: str) -> None:
    """Equal, or fail with the first differing element and its neighbours (never the arrays)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if np.array_equal(got, want):
        return
    ne = got != want
    if ne.ndim > 1:
        ne = ne.any(axis=1)
    i = int(np.argmax(ne))
    a, b = max(0, i - 2), i + 3
    pytest.fail(f"{what}: {int(ne.sum())} of {got.shape[0]} differ, first at {i}: got[{a}:{b}] = {got[a:b].tolist()}, "
                f"want[{a}:{b}] = {want[a:b].tolist()}")


def large_word(case) -> int:
    """What -mum's run() reports in scalars[1]: its blocks of more than 256 rows << 40 | their rows."""
    big = [len(b) for b in case.blocks if len(b) > fc.MUM_PAIR_MAX]
    return (len(big) << 40) | sum(big)


def check(case, tri, boff, want) -> None:
    want_rows, want_boff, want_scores = want
    r = filters.run(TYPE[case.filter], tri, boff, capacity=len(tri) + case.slack, max_occ=case.max_occ, max_gap=case.gap)
    first_diff(r.boff, want_boff, f"{case}: block offsets")
    first_diff(r.rows, want_rows, f"{case}: kept rows")
    assert r.total == len(want_rows)
    if case.filter == "chain":
        first_diff(r.column.astype(np.int64), want_scores, f"{case}: scores")
    if case.filter == "mum":
        # before finish(): [1] is not 0 exactly when a block exceeds the pair limit, and then [0] is not final
        assert r.scalars[1] == large_word(case), f"{case}: scalars {r.scalars}"
        assert r.scalars[1] or r.scalars[0] == len(want_rows)
    else:
        assert r.scalars == (len(want_rows), 0), f"{case}: scalars {r.scalars}"


@pytest.mark.parametrize("case", fc.chain_cases(), ids=repr)
def test_chain(door, case):
    check(case, *case.batch(), fc.expected(case))


@pytest.mark.parametrize("case", fc.smem_cases(), ids=repr)
def test_smem(door, case):
    check(case, *case.batch(), fc.expected(case))


@pytest.mark.parametrize("case", fc.mum_cases(), ids=repr)
def test_mum(door, case):
    check(case, *case.batch(), fc.expected(case))


@pytest.mark.parametrize("case", fc.batch_cases(), ids=repr)
def test_batch(door, case):
    check(case, *case.batch(), fc.expected(case))


def test_workspace_door(door):
    """The second door: a workspace grows with the list and is refused (0) for what is no list filter."""
    for t in TYPE.values():
        small, big = filters.workspace_bytes(t, 16, 1000), filters.workspace_bytes(t, 16, 100_000)
        assert 0 < small < big
    assert filters.workspace_bytes(5, 16, 1000) == 0 and filters.workspace_bytes(0, 16, 1000) == 0


@pytest.mark.parametrize("case", fc.order_cases(), ids=repr)
def test_out_of_order(door, case):
    """The door returns the filter's result; scalars[1] names the highest-numbered bad block; the bad blocks contribute no rows
    (their count is 0, -chain's score 0) and every good block is exactly the spec's."""
    tri, boff = case.batch()
    bad = [k for k, m in enumerate(case.meta) if m["bad"]]
    good = fc.Case(case.name + "/good", case.filter, [np.zeros((0, 3), np.int64) if m["bad"] else b for b, m in zip(case.blocks, case.meta)],
                   gap=case.gap, max_occ=case.max_occ)
    want_rows, want_boff, want_scores = fc.expected(good)
    r = filters.run(TYPE[case.filter], tri, boff, max_occ=case.max_occ, max_gap=case.gap)
    assert r.scalars[1] == max(bad) + 1, f"{case}: scalars {r.scalars}, bad blocks {bad}"
    first_diff(r.boff, want_boff, f"{case}: block offsets")
    first_diff(r.rows, want_rows, f"{case}: kept rows")
    assert r.scalars[0] == r.total == len(want_rows)
    for k in bad:
        assert r.boff[k] == r.boff[k + 1]
    if case.filter == "chain":
        first_diff(r.column.astype(np.int64), want_scores, f"{case}: scores")


def test_door_equals_public_api(door):
    """The door is the product: on the -mem rows of a small read batch it returns, byte for byte, what find_chains, find_smems
    and find_mums return for the same reads."""
    from slamem_amd import engine
    from test_gpu_chain import indel_reads
    ref, q, off = indel_reads(3)
    idx = engine.Index.build(ref)
    min_len = (int(idx.info.seed_k) or 12) + 1
    mem, mem_boff = idx.find_mems(q, off, min_len, True)
    tri = np.stack([mem["ref_pos"], mem["query_pos"], mem["length"]], axis=1).astype(np.int64)
    assert len(tri) > 500 and len(mem_boff) == 2 * (len(off) - 1) + 1

    def raw(rows):
        return np.ascontiguousarray(rows.astype(np.uint32)).tobytes()

    for gap in (0, 100):
        ch, ch_boff, scores = idx.find_chains(q, off, min_len, True, max_gap=gap)
        r = filters.run(filters.CHAIN, tri, mem_boff, max_gap=gap)
        assert raw(r.rows) == ch.tobytes() and r.boff.astype(np.uint64).tobytes() == np.asarray(ch_boff, np.uint64).tobytes()
        assert r.column.tobytes() == np.asarray(scores, np.uint32).tobytes() and 0 < len(ch) < len(mem)
    for occ in (0, 1):
        sm, sm_boff = idx.find_mems(q, off, min_len, True, smem=True, max_occ=occ)
        r = filters.run(filters.SMEM, tri, mem_boff, max_occ=occ)
        assert raw(r.rows) == sm.tobytes() and r.boff.astype(np.uint64).tobytes() == np.asarray(sm_boff, np.uint64).tobytes()
    mu, mu_boff = idx.find_mems(q, off, min_len, True, mum=True)
    r = filters.run(filters.MUM, tri, mem_boff)
    assert raw(r.rows) == mu.tobytes() and r.boff.astype(np.uint64).tobytes() == np.asarray(mu_boff, np.uint64).tobytes()
    assert 0 < len(mu) < len(mem)
    idx.close()
