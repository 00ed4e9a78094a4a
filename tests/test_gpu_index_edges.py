"""The built index against the oracle on the texts of tests/index_edge_cases.py: repeats of 45,000 to 70,000 letters (the
256-letter hand-over of k_lcp_kasai, the 4096-letter steps of wave_extend_lcp, both sampled LCP passes, the zero words
behind the text, 12 to 13 doubling rounds), one text of 4.3 M letters (the third level of the scans and the fifth level
of the min hierarchy inside a real build), and plain random texts whose row counts sit on the tile and switch edges.

SA, BWT, LCP, PSV and NSV are uniquely defined by the text, so the comparison is bit-exact, as in
test_gpu_parity.py::test_index_arrays_match_oracle."""
import numpy as np
import pytest

import index_edge_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (there is no CPU path)")
    from slamem_amd import engine
    return engine


def same(got: np.ndarray, want: np.ndarray, what: str, first: int = 0) -> None:
    """Bit-exact, or the first differing row and the values around it (never the arrays)."""
    assert got.shape == want.shape, f"{what}: {got.shape[0]} rows, want {want.shape[0]}"
    if np.array_equal(got, want):
        return
    ne = np.nonzero(got != want)[0]
    i = int(ne[0])
    a, b = max(0, i - 3), i + 4
    pytest.fail(f"{what}: {ne.shape[0]} of {got.shape[0]} rows differ, first at row {i + first}: rows {a + first}..{b + first - 1} "
                f"got {got[a:b].tolist()}, want {want[a:b].tolist()}")


def arrays_of(g, n):
    from slamem_amd import capi
    return {"SA": g.download(capi.ARRAY_SA).astype(np.int64), "BWT": g.download(capi.ARRAY_BWT),
            "LCP": g.download(capi.ARRAY_LCP).astype(np.int64),
            "PSV": g.download(capi.ARRAY_PSV).astype(np.int64)[1:n + 1],
            "NSV": g.download(capi.ARRAY_NSV).astype(np.int64)[1:n + 1]}


def check_against_oracle(eng, text: bytes, name: str, compact: bool):
    from oracle import pyoracle as po
    from slamem_amd import capi
    n = len(text)
    o = po.OracleIndex(text)
    want = {"SA": o.sa, "BWT": o.bwt, "LCP": o.lcp, "PSV": o.psv[1:n + 1], "NSV": o.nsv[1:n + 1]}
    g = eng.Index.build(text, layout=capi.LAYOUT_FULL)
    assert g.bwt_size() == n + 1 and g.info.layout == capi.LAYOUT_FULL
    got = arrays_of(g, n)
    max_lcp, rounds = int(g.info.max_lcp), int(g.info.sort_rounds)
    g.close()
    print(f"{name}: n {n} max_lcp {max_lcp} sort_rounds {rounds}")
    for k in ("SA", "BWT", "LCP", "PSV", "NSV"):
        same(got[k], want[k], f"{name} {k} vs oracle", first=1 if k in ("PSV", "NSV") else 0)
    oracle_max = int(want["LCP"][1:n + 1].max()) if n else 0
    assert max_lcp == oracle_max, f"{name}: header max_lcp {max_lcp}, oracle {oracle_max}"
    assert rounds >= ec.min_sort_rounds(oracle_max), f"{name}: {rounds} doubling rounds cannot tell {oracle_max} shared letters apart"
    if compact:
        c = eng.Index.build(text, layout=capi.LAYOUT_COMPACT)
        assert c.info.layout == capi.LAYOUT_COMPACT
        cgot = arrays_of(c, n)
        assert int(c.info.max_lcp) == max_lcp
        c.close()
        for k in ("SA", "BWT", "LCP", "PSV", "NSV"):
            same(cgot[k], got[k], f"{name} {k} compact vs full layout", first=1 if k in ("PSV", "NSV") else 0)
    return max_lcp, rounds


@pytest.mark.parametrize("name", list(ec.DESIGNED))
def test_designed_text_index_matches_oracle(eng, name):
    max_lcp, rounds = check_against_oracle(eng, ec.designed_text(name), name, compact=name not in ec.NO_COMPACT)
    assert max_lcp == ec.DESIGNED[name][1]
    assert rounds >= (12 if name == "tail" else 13)


@pytest.mark.parametrize("n", ec.RANDOM_SIZES)
def test_random_text_index_matches_oracle(eng, n):
    check_against_oracle(eng, ec.random_text(n), f"random{n}", compact=False)
