"""-cons -gt without a GPU: tests/cons_gt_spec.py on designed rows and events, its three properties on random
tables, three wrong rules that each change the designed case's bytes, and what the library's new entry points refuse before
they touch a device.  (The command line has no -cons -gt: 4.32 says why.)"""
import ctypes as C

import numpy as np
import pytest

import cons_gt_cases as cases
import cons_gt_spec as cg
import cons_spec as cs
import gt_spec

MD = cases.MIN_DEPTH


def call(case, ploidy=2, weighted=False, min_gq=20, costs=None, E=None, **kw):
    P_row, P_ev = cg.params(ploidy, weighted=weighted, costs=costs)
    return cg.consensus(case["T"], case["table"], case["E"] if E is None else E, P_row, P_ev, MD, min_gq, case["qtable"] if weighted else None, **kw)


def byte_at(case, p, **kw):
    seq, offs, _ = call(case, first=p, count=1, bounds=[p, p + 1], **kw)
    return seq


def row_of(case, p, ploidy=2, weighted=False, min_gq=20, costs=None):
    P_row, _ = cg.params(ploidy, weighted=weighted, costs=costs)
    return cg.row(case["T"], case["table"], case["qtable"], p, P_row, MD, min_gq, weighted)


def test_the_spec_on_designed_rows():
    case = cases.designed()
    T, own = case["T"], case["own"]

    def letter(p, shift=0):
        return b"ACGT"[(int(own[p]) + shift) % 4:(int(own[p]) + shift) % 4 + 1]

    def code(p, s1, s2):
        a, b = sorted(((int(own[p]) + s1) % 4, (int(own[p]) + s2) % 4))
        return cg.IUPAC[(a, b)]
    for ploidy in (1, 2):
        assert row_of(case, cases.HOM_REF, ploidy) == ("called", letter(cases.HOM_REF), "hom")
        assert row_of(case, cases.HOM_ALT, ploidy) == ("called", letter(cases.HOM_ALT, 1), "hom")
        assert row_of(case, cases.SHALLOW, ploidy) == ("uncalled", letter(cases.SHALLOW).lower(), "depth")
        assert row_of(case, cases.EMPTY, ploidy) == ("uncalled", letter(cases.EMPTY).lower(), "empty")
        assert row_of(case, cases.NROW, ploidy) == ("N", b"N", "")
    assert row_of(case, cases.HET_REF) == ("called", code(cases.HET_REF, 0, 1), "het")
    assert row_of(case, cases.HET_ALT) == ("called", code(cases.HET_ALT, 1, 2), "het")
    # 10:10 and haploid: the likelihoods tie and the prior of 30 Phred decides for the reference -- with exactly that GQ
    assert row_of(case, cases.HET_REF, ploidy=1) == ("called", letter(cases.HET_REF), "hom")
    assert row_of(case, cases.HET_REF, ploidy=1, min_gq=31)[::2] == ("uncalled", "gq")
    assert row_of(case, cases.BIG) == ("called", code(cases.BIG, 0, 1), "het")  # counters of 2^20: sums beyond 32 bits
    assert 2 ** 20 * gt_spec.gt_costs(20)[2] > 2 ** 32
    # the qualities decide: many poor reference letters against few good other ones
    assert row_of(case, cases.WQ_ROW, ploidy=1) == ("called", letter(cases.WQ_ROW), "hom")
    assert row_of(case, cases.WQ_ROW, ploidy=1, weighted=True) == ("called", letter(cases.WQ_ROW, 1), "hom")
    # exactly on the threshold, and one milli-Phred below it
    found = 0
    for combo, pair in case["edges"].items():
        ploidy, weighted, min_gq, costs = combo
        if pair is None:
            # GQ is never below 0; a haploid GQ at -gt's own costs moves in steps of E - M = 24,727 (weighted: the search's rows with
            # a quality sum within 93 a letter reach the threshold but not the number below it), so only these have no pair
            assert min_gq == 0 or (ploidy == 1 and costs is None), combo
            continue
        found += 1
        on, below = pair
        P_row, _ = cg.params(ploidy, weighted=weighted, costs=costs)
        for p, gq in ((on, 1000 * min_gq), (below, 1000 * min_gq - 1)):
            assert cases.gq_of([int(v) for v in case["table"][p][:4]], [int(v) for v in case["qtable"][p][:4]], int(own[p]), P_row, weighted) == gq
        assert row_of(case, on, ploidy, weighted, min_gq, costs)[0] == "called"
        assert row_of(case, below, ploidy, weighted, min_gq, costs)[::2] == ("uncalled", "gq")
    assert found == 8 and {c[:2] for c, p in case["edges"].items() if p is not None} == {(1, False), (1, True), (2, False), (2, True)}
    assert all(case["edges"][(2, w, gq, None)] is not None for w in (False, True) for gq in (20, 999))  # the real -gt and -wq costs
    # the statistics of the whole: every designed row lands where it is named
    for ploidy, weighted, min_gq, costs in cases.COMBOS:
        P_row, P_ev = cg.params(ploidy, weighted=weighted, costs=costs)
        em, het = cg.emissions(T, case["table"], case["E"], P_row, P_ev, MD, min_gq, case["qtable"] if weighted else None)
        seq, offs, st = call(case, ploidy, weighted, min_gq, costs, bounds=list(range(cases.N + 1)))
        assert st[0] == sum(r == "uncalled" for _, r, _, _ in em) and st[5] == sum(w == "het" for *_, w in em) and st[6] == sum(w == "gq" for *_, w in em)
        assert st[1] >= st[5] and st[0] >= st[6] + 2 and st[7] == het == (1 if ploidy == 2 and min_gq <= 20 else 0), (ploidy, weighted, min_gq, st)
        assert offs[-1] == len(seq) == sum(len(S) + len(l) for S, _, l, _ in em)
    assert call(case, min_gq=999)[2][6] > 300  # (no row of depth 8 is that sure)


def test_the_spec_on_designed_events():
    case = cases.designed()
    T, t, E = case["T"], case["table"], case["E"]
    _, P_ev = cg.params(2)
    calls = {e[:3]: cg.event_call(T, t, e, P_ev, MD, 20) for e in E}
    assert calls[(100, 0, 3)] == (True, False) and calls[(120, 0, 2)] == (False, True)
    assert calls[(140, 1, 2)] == (True, False) and calls[(140, 1, 1)] == (True, False) and calls[(51, 1, 2)] == (True, False)
    assert cs.anchor(T, 51) == 51 and cs.anchor(T, 100) == 99
    em, het = cg.emissions(T, t, E, *cg.params(2), MD, 20)
    assert het == 1
    assert [r for _, r, _, _ in em[100:103]] == ["deleted"] * 3 and em[120][1] == em[121][1] == "called"  # (the het deletion: the reference stays)
    assert em[140][0] == next(e[3] for e in E if e[:3] == (140, 1, 1)) and em[51][0] == b"CA"  # (20 observations beat 19)
    seq, offs, st = call(case, bounds=[51, 52, 140, 141])
    assert seq[offs[0]:offs[1]][:2] == b"CA" and offs[1] - offs[0] == 3 and offs[3] - offs[2] == 2
    assert st[2] == 3 and st[3] == 2 and st[4] == 3 and st[7] == 1
    # haploid: 10 of 20 is a tie between 0 and 1 -- nothing applied, nothing heterozygous
    _, P1 = cg.params(1)
    assert cg.event_call(T, t, next(e for e in E if e[:3] == (120, 0, 2)), P1, MD, 20) == (False, False)
    # a shallow or N anchor: not applied, whatever the genotype
    assert not cg.event_call(T, t, (cases.SHALLOW + 1, 0, 1, b"", 3, 0), P_ev, MD, 0)[0]
    assert not cg.event_call(T, t, (cases.NROW, 0, 1, b"", 30, 0), P_ev, 1, 0)[0] or cs.anchor(T, cases.NROW) != cases.NROW


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_three_properties_on_random_tables(seed):
    rng = np.random.default_rng(seed)
    n = 700
    text, t, q, raw, E = cases.random_table(n, rng)
    T = bytes(text)
    for ploidy, weighted, min_gq in ((2, False, 20), (1, False, 0), (2, True, 10), (1, True, 35)):
        P_row, P_ev = cg.params(ploidy, weighted=weighted)
        qt = q if weighted else None
        whole, offs, st = cg.consensus(T, t, E, P_row, P_ev, MD, min_gq, qt, bounds=list(range(n + 1)))
        # slice: any range's bytes are the whole's between offs, and the statistics add up over a cut into ranges
        cuts = [0] + sorted(int(v) for v in rng.choice(np.arange(1, n), size=5, replace=False)) + [n]
        total = [0] * 8
        for a, b in zip(cuts, cuts[1:]):
            part, poffs, pst = cg.consensus(T, t, E, P_row, P_ev, MD, min_gq, qt, a, b - a, bounds=[a, (a + b) // 2, b])
            assert part == whole[offs[a]:offs[b]] and poffs == [offs[x] - offs[a] for x in (a, (a + b) // 2, b)]
            total = [x + y for x, y in zip(total, pst)]
        assert total == st
        # containment: an upper-case byte that differs from the reference is a row genotypes(min_qual=min_gq) returns, same (a, b)
        if not weighted:
            P = gt_spec.check_params(tuple(P_row) + (MD, min_gq))
            pos, _, gts = gt_spec.genotypes(t, T, P)
            sel = {int(p): (int(g["a"]), int(g["b"])) for p, g in zip(pos, gts)}
            em, _ = cg.emissions(T, t, [], P_row, P_ev, MD, min_gq, None)
            seen = 0
            for p, (_, rule, letter, _) in enumerate(em):
                if rule == "called" and letter[0] != (T[p] & 0xDF):
                    assert p in sel and cg.letter_of(*sel[p]) == letter
                    seen += 1
            assert seen > 20
    # the degenerate case: min_gq 0, haploid, no events, one letter holds every observation: the plurality consensus
    one = t.copy()
    keep = one[:, :4].argmax(axis=1)
    for p in range(n):
        v = int(one[p][keep[p]])
        one[p][:4] = 0
        one[p][keep[p]] = v
    P_row, P_ev = cg.params(1)
    got = cg.consensus(T, one, [], P_row, P_ev, MD, 0)
    want = cs.consensus(T, one, [], MD)
    assert got[0] == want[0] and got[2][:5] == want[2] and got[2][5:] == [0, 0, 0]


def test_three_wrong_rules_show(monkeypatch):
    case = cases.designed()
    right = call(case)[0]
    # QUAL in the place of GQ: the 10:10 row of two other letters has a huge QUAL against the reference and is called either way,
    # but a row that is surely not the reference's and unsure between two others is not -- and a reference row has QUAL 0
    with monkeypatch.context() as m:
        m.setattr(cg, "confident", lambda g, min_gq: g[0] >= 1000 * min_gq)
        assert call(case)[0] != right
    with monkeypatch.context() as m:  # het events applied
        m.setattr(cg, "event_genotype_applies", lambda g: g[3] == 1)
        wrong = call(case)
        assert wrong[0] != right and wrong[2][2] == 5
    with monkeypatch.context() as m:  # the first allele of a het
        m.setattr(cg, "letter_of", lambda a, b: cg.ACGT[a:a + 1])
        wrong = call(case)[0]
        assert wrong != right and len(wrong) == len(right) and not set(wrong) & set(b"MRWSYK") and set(right) & set(b"MRWSYK")


# ---- the library, as far as it goes without a device ------------------------------------------------------------------------------

def test_the_library_exports_the_entry_points_and_refuses_null_arguments():
    from slamem_amd import capi
    L = capi.lib()
    assert {"slamem_pileup_consensus_gt_device", "slamem_pileup_consensus_gt_host"} <= set(capi.ABI_SYMBOLS)
    assert C.sizeof(capi.ConsGtParams) == 2 * C.sizeof(capi.GtParams) + 12 == 68
    prm = capi.ConsGtParams(capi.GtParams(2, 44, 3039, 24771, 30000, 4, 0), capi.GtParams(2, 44, 3039, 24771, 30000, 4, 0), 4, 20, 0)
    total, stats = C.c_uint64(), (C.c_uint64 * 8)()
    for fn, tail in ((L.slamem_pileup_consensus_gt_device, (None,)), (L.slamem_pileup_consensus_gt_host, ())):
        assert fn(None, 0, 0, C.byref(prm), 0, None, None, 0, None, stats, C.byref(total), *tail) == capi.SLAMEM_ERR_ARG
        assert b"null argument" in L.slamem_last_error_message() and b"consensus_gt" in L.slamem_last_error_message()
