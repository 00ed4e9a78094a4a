"""The designed lists of tests/filter_list_cases.py, checked with the specs alone (no GPU): they are in the emission order,
sit on the kernels' limits as those stand in the sources today, and have the predecessors, ties, containers and runs that
their builders promise -- so that tests/test_gpu_filter_lists.py compares the product on the edges it says it does."""
import os
import re

import numpy as np

import chain_spec
import filter_list_cases as fc
import mum_spec
import smem_spec

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slamem_amd", "csrc")


def constexprs(name: str) -> dict:
    """name = value of every `constexpr <type> a = 1, b = a * 2;` line of a source file whose values are integers or products of
    earlier ones."""
    out = {}
    for line in open(os.path.join(CSRC, name)):
        m = re.match(r"\s*constexpr\s+(?:unsigned|uint32_t|uint64_t)\s+(.*?);", line)
        if not m:
            continue
        for part in m.group(1).split(","):
            k, _, v = part.partition("=")
            v = v.strip().rstrip("u")
            if re.fullmatch(r"\d+", v):
                out[k.strip()] = int(v)
            elif re.fullmatch(r"\w+\s*\*\s*\w+", v):
                x, y = (t.strip() for t in v.split("*"))
                if x in out and y in out:
                    out[k.strip()] = out[x] * out[y]
    return out


def test_the_limits_are_the_kernels():
    c = constexprs("chain_filter.hip")
    assert (c["kChainLaneMax"], c["kChainTile"], c["kChainWaveGrid"]) == (32, 1024, 2048) == (fc.CHAIN_LANE_MAX, fc.CHAIN_TILE, fc.CHAIN_WAVE_GRID)
    s = constexprs("smem_filter.hip")
    assert (s["kSmemLaneMax"], s["kSmemTile"], s["kSmemItems"], s["kSmemWg"], s["kSmemLargeGrid"]) == (256, 2048, 8, 256, 256) == \
        (fc.SMEM_LANE_MAX, fc.SMEM_TILE, fc.SMEM_ITEMS, fc.SMEM_WG, fc.SMEM_LARGE_GRID)
    assert constexprs("mum_filter.hip")["kMumPairMax"] == 256 == fc.MUM_PAIR_MAX
    # both sides of every limit are among the sizes
    for sizes, limits in ((fc.CHAIN_SIZES, (32, 64, 128, 1024, 1088, 2048)), (fc.SMEM_SIZES, (256, 512, 2048, 4096)), (fc.MUM_SIZES, (256,))):
        for x in limits:
            assert {x - 1, x, x + 1} <= set(sizes), (sizes, x)


def test_names_are_unique_and_rows_fit_32_bits():
    cases = fc.all_cases() + fc.order_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        tri, boff = c.batch()
        if len(tri):
            assert tri.min() >= 0 and tri[:, :2].max() <= 2**32 - 1 and tri[:, 2].min() >= 1, c
            if c.filter != "smem":  # (-smem alone is given ends beyond 2^32)
                assert (tri[:, :2].max(axis=1) + tri[:, 2]).max() <= 2**32 - 1, c


def test_emission_order():
    """Every block of the -chain and -smem cases is in the order, every block marked bad is not (and by one pair of rows)."""
    for c in fc.all_cases():
        if c.filter != "mum":
            for k, b in enumerate(c.blocks):
                assert chain_spec.in_emission_order(b) and smem_spec.in_emission_order(b), (c, k)
    bad = 0
    for c in fc.order_cases():
        for b, m in zip(c.blocks, c.meta):
            assert chain_spec.in_emission_order(b) == smem_spec.in_emission_order(b) == (not m["bad"]), c
            if m["bad"]:
                dq, dl = np.diff(b[:, 1]), np.diff(b[:, 2])
                assert int(((dq > 0) | ((dq == 0) & (dl > 0))).sum()) == 1
                bad += 1
    assert bad > 50


def scores_into(a: np.ndarray, f, i: int, gap: int):
    """(admissible mask, f(j) + link(j, i)) over all rows j of the block, by the definition's formulas, vectorised."""
    p, q, ln = a[:, 0], a[:, 1], a[:, 2]
    dq, dp, de = q[i] - q, p[i] - p, ln[i] - ln
    ok = (dq > 0) & (dq <= gap) & (dp > 0) & (dp <= gap) & (dq + de > 0) & (dp + de > 0)
    s = np.asarray(f, np.int64) + np.minimum(ln[i], np.minimum(dq + de, dp + de)) - np.abs(dp - dq)
    return ok, s


def chain_of(f, pred) -> list:
    """The rows of the block's chain from (f, pred): what chain_spec.block_chain keeps."""
    i = max(range(len(f)), key=lambda k: (f[k], -k))
    out = []
    while i >= 0:
        out.append(i)
        i = pred[i]
    return out


def by_pattern(cases, pattern):
    for c in cases:
        for b, m in zip(c.blocks, c.meta):
            if m.get("pattern") == pattern:
                yield c, b, m


def test_chain_far_predecessors():
    seen, places = set(), set()
    for c, a, m in by_pattern(fc.chain_cases(), "far"):
        i, k, n = m["i"], m["k"], m["n"]
        f, pred = chain_spec.chain_dp_windowed(a, c.gap)
        assert pred[i] == i + k and f[i] == 2000 + k == max(f) and f.index(max(f)) == i, (c, m)
        ok, _ = scores_into(a, f, i, c.gap)
        assert ok.sum() == 1 and ok[i + k], (c, m)                      # the only admissible one
        q = a[:, 1]
        assert np.all(q[i] - q[i + 1:i + k + 1] <= c.gap)               # the rows between are inside the q window
        assert chain_of(f, pred) == [i, i + k]
        if m["between"] == "end" and c.gap >= k + 5:
            j = np.arange(i + 1, i + k)
            assert np.all((a[i, 0] - a[j, 0] > 0) & (a[i, 0] - a[j, 0] <= c.gap) & (a[j, 1] + a[j, 2] == a[i, 1] + a[i, 2]))
            seen.add(("end", k))
        seen.add(("dp", k))
        # where the predecessor lies, seen from the wave's tiles (cut from the block's end)
        if n > fc.CHAIN_LANE_MAX:
            ti, tp = (n - 1 - i) // fc.CHAIN_TILE, (n - 1 - (i + k)) // fc.CHAIN_TILE
            places.add((k, "same tile" if ti == tp else "behind"))
            if i + k == n - 1:
                places.add((k, "last row"))
    assert {("dp", k) for k in fc.FAR_K} <= seen and {("end", k) for k in fc.FAR_K if k > 1} <= seen
    for k in fc.FAR_K:
        assert (k, "behind") in places and (k, "last row") in places
        assert (k, "same tile") in places or k >= fc.CHAIN_TILE


def test_chain_ties():
    """two_chains: two rows reach the best score, row 0 ends the chain.  one_diagonal from gap 2 on: two predecessors reach a
    row's best score, the nearer one is taken -- in blocks on both sides of the lane limit and of a tile."""
    for c, a, m in by_pattern(fc.chain_cases(), "two_chains"):
        if m["n"] < 2:
            continue
        f, pred = chain_spec.chain_dp_windowed(a, c.gap)
        assert f.count(max(f)) == 2 and f[0] == f[1] == max(f), (c, m)
        kept = chain_of(f, pred)
        assert kept[0] == 0 and 1 not in kept and len(kept) == m["n"] // 2
    tied = set()
    for c, a, m in by_pattern(fc.chain_cases(), "one_diagonal"):
        n = m["n"]
        f, pred = chain_spec.chain_dp_windowed(a, c.gap)
        assert n == 0 or sorted(chain_of(f, pred)) == list(range(n)), (c, m)   # every row is kept
        for i in {0, n - 3, n - fc.CHAIN_TILE - 1, n - fc.CHAIN_TILE - 2} if n >= 3 and c.gap >= 4 else ():
            if 0 <= i < n - 2:
                ok, s = scores_into(a, f, i, c.gap)
                best = s[ok].max()
                assert (s[ok] == best).sum() >= 2 and pred[i] == i + 1 == int(np.flatnonzero(ok & (s == best))[0]), (c, m, i)
                tied.add(n)
    assert {33, 1025, 2049} <= tied


def test_chain_window_edges():
    kinds = set()
    for c, a, m in by_pattern(fc.chain_cases(), "window"):
        i, e = m["i"], m["edge"]
        assert e - i == m["dist"]
        f, pred = chain_spec.chain_dp_windowed(a, c.gap)
        if m["kind"] == "out":
            assert pred[i] == -1, (c, m)
            assert chain_spec.chain_dp_windowed(a, c.gap + 1)[1][i] == e, (c, m)   # one more letter of gap and it links
            d = (a[i, 1] - a[e, 1], a[i, 0] - a[e, 0])
            assert max(d) == c.gap + 1
        else:
            assert pred[i] == e and (a[i, 1] - a[e, 1], a[i, 0] - a[e, 0]) == (c.gap, c.gap), (c, m)
        assert max(range(len(f)), key=lambda k: (f[k], -k)) == i   # the chain ends in row i: its predecessor shows in the result
        kinds.add((m["axis"], m["kind"], m["dist"], m["n"] - 1 == e))
    for axis in "qp":
        for dist in (1, 64, 65, 128):
            assert (axis, "in", dist, True) in kinds and (axis, "out", dist, True) in kinds and (axis, "both", dist, False) in kinds


def test_chain_no_gain_and_groups():
    for c, a, m in by_pattern(fc.chain_cases(), "no_gain"):
        if m["n"] < 2:
            continue
        f, pred = chain_spec.chain_dp_windowed(a, c.gap)
        assert set(pred) == {-1} and chain_of(f, pred) == [0]
        if c.gap >= 50:
            assert scores_into(a, f, 0, c.gap)[0].any()   # (there are admissible rows: it is the gain that fails)
    edge = 0
    for c, a, m in by_pattern(fc.chain_cases(), "start_groups"):
        n = m["n"]
        if n > fc.CHAIN_TILE:
            t = n - fc.CHAIN_TILE   # the first row of the last tile
            edge += a[t, 1] == a[t - 1, 1]
    assert edge >= 4   # groups that lie across a tile edge


def test_chain_all_pairs_equals_windowed_up_to_129_rows():
    """chain_dp tests every pair in any order; chain_dp_windowed is what the large blocks are compared with."""
    n = 0
    for c in fc.chain_cases() + [b for b in fc.batch_cases() if b.filter == "chain" and "sizes" in b.name]:
        for a in c.blocks:
            if len(a) <= 129:
                assert chain_spec.chain_dp(a, c.gap or chain_spec.DEFAULT_GAP) == chain_spec.chain_dp_windowed(a, c.gap or chain_spec.DEFAULT_GAP), c
                n += 1
    assert n > 300


def test_chain_large_coordinates():
    n = 0
    for c in fc.chain_cases():
        if "large-coordinates" in c.name:
            for a in c.blocks:
                n += int((a[:, :2].min(axis=1) >= fc.BIG).sum())
                assert a[:, :2].max() >= fc.BIG
    assert n > 5000


def test_smem_containers_and_ends():
    dist, rule_a, ends64 = set(), set(), 0
    for c in fc.smem_cases():
        if not c.name.startswith("smem-containers") or c.max_occ:
            continue
        for a, m in zip(c.blocks, c.meta):
            keep = smem_spec.smem_keep(a)
            if m["pattern"] in ("container-b", "container-a"):
                i, k = m["i"], m["container"]
                without = np.delete(a, k, axis=0)
                assert not keep[i] and smem_spec.smem_keep(without)[i - (k < i)], (c, m)   # the container decides
                if m["pattern"] == "container-b":
                    assert a[k, 1] < a[i, 1] and a[k, 1] + a[k, 2] == a[i, 1] + a[i, 2]
                    dist.add((k - i, m["n"] > fc.SMEM_LANE_MAX))
                    ends64 += int(a[i, 1] + a[i, 2] >= 2**32)
                else:
                    assert a[k, 1] == a[i, 1] and a[k, 2] > a[i, 2]
                    rule_a.add(k + 1)
            else:
                assert not keep[m["contained"]].any() and keep[m["free"]].all() and m["contained"] and m["free"], (c, m)
                ends64 += int((a[m["contained"], 1] + a[m["contained"], 2] >= 2**32).sum())
    assert {(d, True) for d in fc.CONTAINER_D} <= dist and {(d, False) for d in (1, 7, 8, 9)} <= dist
    assert rule_a == {fc.SMEM_ITEMS, fc.SMEM_WAVE_ROWS, fc.SMEM_TILE, 2 * fc.SMEM_TILE}
    assert ends64 >= 10


def test_smem_runs_and_caps():
    caps = {c.max_occ for c in fc.smem_cases() if c.name.startswith("smem-runs")}
    assert caps == set(fc.run_caps()) >= {0, 1, 2, 5}
    seen = set()
    for c, a, m in by_pattern(fc.smem_cases(), "run"):
        s, ln = m["start"], m["length"]
        assert {ln - 1, ln, ln + 1} <= caps
        assert (s + 3) in (fc.SMEM_ITEMS, fc.SMEM_WAVE_ROWS, fc.SMEM_TILE)
        assert np.all(a[s:s + ln, 1:] == a[s, 1:]) and smem_spec.runs_adjacent(a) and smem_spec.occurrence_counts(a)[s] == ln
        assert smem_spec.block_keep(a, 0)[s:s + ln].all() and smem_spec.block_keep(a, ln)[s:s + ln].all()
        if ln >= 2:
            assert not smem_spec.block_keep(a, ln - 1)[s:s + ln].any()
        seen.add((ln, s + 3))
    assert len(seen) == len(fc.RUN_LENGTHS) * 3


def test_mum_kinds_and_shuffles():
    c = fc.mum_cases()[0]
    want = {"q-only": False, "p-only": False, "equal-interval": False, "equal-start": False, "equal-end": False, "duplicate": False}
    seen = set()
    for k, (a, m) in enumerate(zip(c.blocks, c.meta)):
        keep = mum_spec.containment_keep(a)
        if m["pattern"] == "as built":
            for y, kind in enumerate(m["kinds"]):
                if kind:
                    assert keep[y] == want[kind], (m["n"], y, kind)
                    # equal intervals and duplicates: both rows go; otherwise the containing row stays
                    assert keep[y - 1] == (kind not in ("equal-interval", "duplicate"))
                    seen.add(kind)
        elif m["pattern"] == "shuffled":
            assert np.array_equal(keep, mum_spec.containment_keep(c.blocks[m["of"]])[m["perm"]])   # the same rows, wherever they stand
    assert seen == set(fc.MUM_KINDS)
    big = fc.mum_cases()[1]
    tri, _ = big.batch()
    assert tri[:, :2].min() >= fc.BIG - 10 and (tri[:, :2].max(axis=1) + tri[:, 2]).max() == 2**32 - 1


def test_batches():
    by = {c.name: c for c in fc.batch_cases()}
    for f, sizes in (("chain", fc.CHAIN_SIZES), ("smem", fc.SMEM_SIZES), ("mum", fc.MUM_SIZES)):
        for slack in (0, 5):
            c = by[f"batch-{f}-sizes-slack{slack}"]
            got = [len(b) for b in c.blocks]
            assert sorted(x for x in got if x) == sorted(x for x in sizes if x) and got.count(0) >= 4 and c.slack == slack
            assert [x for x in got if x] != sorted(x for x in got if x)
    assert [len(b) for b in by["batch-chain-2100x33"].blocks] == [33] * 2100 and 2100 > fc.CHAIN_WAVE_GRID
    assert [len(b) for b in by["batch-smem-260x257"].blocks] == [257] * 260 and 260 > fc.SMEM_LARGE_GRID
    assert [len(b) for b in by["batch-mum-300x257"].blocks] == [257] * 300 and 300 > 256
    assert max(c.rows for c in fc.batch_cases()) <= 80_000


def test_order_cases_cover_what_they_say():
    seen = set()
    for c in fc.order_cases():
        bad = [k for k, m in enumerate(c.meta) if m["bad"]]
        assert len(c.blocks) == 16 and bad in ([5], [3, 11])
        for k in bad:
            b = c.blocks[k]
            dq, dl = np.diff(b[:, 1]), np.diff(b[:, 2])
            i = int(np.flatnonzero((dq > 0) | ((dq == 0) & (dl > 0)))[0])
            seen.add((c.filter, len(b), i if i in (0, 7, 511, 1023, 2047) else "n-2" if i == len(b) - 2 else "mid", "q" if dq[i] > 0 else "L"))
    for f, (sizes, places) in fc.ORDER_SIZES.items():
        for n in sizes:
            for pl in places:
                i = n - 2 if pl == "n-2" else pl
                if 0 <= i <= n - 2:
                    for how in "qL":
                        assert (f, n, "n-2" if i == n - 2 and i not in (0, 7, 511, 1023, 2047) else i, how) in seen, (f, n, pl, how)
