"""-stats without a GPU: the spec's table on hand-made mappings whose counts are written out here; the C report
writer against the spec's text; the option's row in the table of slamem_host.c."""
import numpy as np
import pytest

import hostlib
import stats_host
import stats_spec
from stats_spec import SECTIONS, TOTALS

# The text: T[2:13] = ACG T AC GT A CC under read 1, T[20:24] = TTGA and T[40:44] = CAGT under read 2.
TEXT = bytearray(b"A" * 800)
TEXT[2:13] = b"ACGTACGTACC"
TEXT[20:24] = b"TTGA"
TEXT[40:44] = b"CAGT"
TEXT = bytes(TEXT)
# read 1, forward, mapq 40: one letter clipped, then 3= 1X 2= 1I 2= 1D 2= from reference place 2 (X: the text's T under the read's A)
R1 = b"NACGAACTGTCC"
Q1 = bytes(33 + v for v in (2, 30, 30, 30, 10, 30, 30, 5, 40, 40, 40, 40))
# read 2, reverse, mapq 10: the scanned strand is TTGACCCGGT; 4= of it at reference place 20, letters 4 and 5 in no segment,
# 1= 1X 2= from letter 6 at reference place 40 (X: the text's A under the strand's G)
R2 = b"ACCGGGTCAA"
Q2 = bytes([53, 53, 136, 53, 53, 53, 53, 53, 53, 20])  # (as given: index = cycle; 136 - 33 caps at 93, 20 is below the offset)
R3 = b"ACGTN"  # unmapped
R4 = b"ACGT" * 150  # forward, mapq 0: 600= -- cycles and length above the last bin
RESULTS = [(1, 40, 11, 0, [(2, 1, 11, 11, 3, [("=", 3), ("X", 1), ("=", 2), ("I", 1), ("=", 2), ("D", 1), ("=", 2)])]),
           (2, 10, 8, 6, [(20, 0, 4, 4, 0, [("=", 4)]), (40, 6, 4, 4, 1, [("=", 1), ("X", 1), ("=", 2)])]),
           (0, 0, 0, 0, []),
           (1, 0, 600, 600, [(100, 0, 600, 600, 0, [("=", 600)])])]
QUERIES = R1 + R2 + R3 + R4
QUALS = Q1 + Q2 + bytes([33 + 7] * 5) + bytes([33 + 33] * 600)
OFFSETS = np.array([0, 12, 22, 27, 627], dtype=np.uint64)


def filled(entries):
    t = np.zeros(stats_spec.WORDS, dtype=np.uint64)
    for section, bins in entries.items():
        for k, v in bins.items():
            t[SECTIONS[section][0] + k] = v
    return t


def totals(**kw):
    return {TOTALS.index(k.replace("_", " ")): v for k, v in kw.items()}


HAND_MINQ5 = {
    "totals": totals(reads=4, mapped=3, forward=2, reverse=1, counted=2, counted_split=1, segments=3, letters=627, counted_letters=22,
                     matches=16, mismatches=2, insertions=1, inserted_letters=1, deletions=1, deleted_letters=1, segment_letters=19),
    "mapq": {40: 1, 10: 1, 0: 1},
    "len": {12: 1, 10: 1, 5: 1, 511: 1},
    "nm": {3: 1, 1: 1},
    "cyc_aln": {0: 1, 1: 2, 2: 2, 3: 2, 4: 1, 5: 1, 6: 2, 7: 1, 8: 2, 9: 2, 10: 1, 11: 1},
    "cyc_mm": {4: 1, 2: 1},
    "cyc_ins": {7: 1},
    "cyc_del": {10: 1},
    "sub": {4 * 3 + 0: 1, 4 * 0 + 2: 1},
    "q_aln": {30: 5, 10: 1, 40: 4, 20: 6, 93: 1, 0: 1},
    "q_mm": {10: 1, 93: 1},
    "ins_len": {1: 1},
    "del_len": {1: 1},
}


def test_spec_on_hand_made_mappings():
    got = stats_spec.table(RESULTS, TEXT, QUERIES, OFFSETS, quals=QUALS, min_mapq=5)
    want = filled(HAND_MINQ5)
    for section, (a, n) in SECTIONS.items():
        assert np.array_equal(got[a:a + n], want[a:a + n]), section
    # min_mapq 0: read 4 counts as well -- 600 letters under =, cycles 0 .. 510 once and 89 in the last bin
    got0 = stats_spec.table(RESULTS, TEXT, QUERIES, OFFSETS, quals=QUALS, min_mapq=0)
    more = got0.astype(np.int64) - want.astype(np.int64)
    a = SECTIONS["cyc_aln"][0]
    assert list(more[a:a + 511]) == [1] * 511 and more[a + 511] == 89
    assert more[SECTIONS["q_aln"][0] + 33] == 600 and more[SECTIONS["nm"][0]] == 1
    t = SECTIONS["totals"][0]
    assert [int(more[t + TOTALS.index(k)]) for k in ("counted", "segments", "counted letters", "matches", "segment letters")] == [1, 1, 600, 600, 600]
    assert more.sum() == 600 + 600 + 1 + 1 + 1 + 600 + 600 + 600
    # without quality bytes: the two sections stay empty, everything else is the same
    none = stats_spec.table(RESULTS, TEXT, QUERIES, OFFSETS, min_mapq=5)
    qa, qm = SECTIONS["q_aln"][0], SECTIONS["q_mm"][0]
    assert not none[qa:qm + 96].any() and np.array_equal(none[:qa], want[:qa]) and np.array_equal(none[qm + 96:], want[qm + 96:])
    # an unmapped read and one below min_mapq touch nothing behind their own rows
    only = stats_spec.table(RESULTS[2:], TEXT, QUERIES, OFFSETS[2:], quals=QUALS, min_mapq=5)
    assert int(only.sum()) == 2 + 605 + 2 + 1 + 1 + 1  # reads, letters, len bins, mapped, forward, mapq
    with pytest.raises(AssertionError):  # a letter behind the read's end is no mapping of the engine's
        stats_spec.table([(1, 9, 1, 0, [(0, 3, 3, 3, 0, [("=", 3)])])], TEXT, b"ACGTA", np.array([0, 5], dtype=np.uint64))


def folded_table():
    rng = np.random.default_rng(11)
    t = rng.integers(0, 1 << 40, size=stats_spec.WORDS, dtype=np.uint64)
    t[16:24] = 0
    for s in ("len", "nm", "cyc_aln", "cyc_mm", "cyc_ins", "cyc_del", "ins_len", "del_len", "mapq", "q_aln", "q_mm"):
        a, n = SECTIONS[s]
        t[a + n - 1] = 5 + n  # the last bin of every section, folded ones among them
    a = SECTIONS["q_aln"][0]
    t[a + 7], t[SECTIONS["q_mm"][0] + 7] = 0, 3  # mismatches alone make a BQ row
    t[a + 8], t[SECTIONS["q_mm"][0] + 8] = 0, 0  # an all-zero row is left out
    for s in ("cyc_aln", "cyc_mm", "cyc_ins", "cyc_del"):
        t[SECTIONS[s][0] + 100] = 0
    return t


@pytest.mark.parametrize("name", ["folded", "empty", "no_quals", "hand"])
def test_report_writer_is_the_specs_text(name, tmp_path):
    t = {"folded": folded_table(), "empty": np.zeros(stats_spec.WORDS, dtype=np.uint64),
         "no_quals": stats_spec.table(RESULTS, TEXT, QUERIES, OFFSETS), "hand": filled(HAND_MINQ5)}[name]
    got, want = stats_host.write_report(t, tmp_path / "r.stats"), stats_spec.report(t)
    assert stats_spec.reports_equal(got, want), (got[:400], want[:400])
    tags = [line.split("\t")[0] for line in got.splitlines()]
    assert tags[:19] == ["SN"] * 19
    if name == "empty":
        assert got == want and len(tags) == 19 and got.endswith("SN\tmismatch rate\t0.000000\nSN\tindel rate\t0.000000\n")
    if name == "no_quals":
        assert got == want and "BQ" not in tags
    if name == "folded":
        for row in ("RL\t511+\t517", "NM\t127+\t133", "IL\t63+\t69", "DL\t63+\t69", "MQ\t63\t69", "BQ\t7\t0\t3\t"):
            assert ("\n" + row) in got, row
        assert "\nCY\t511+\t517\t517\t517\t517\n" in got and "\nCY\t100\t" not in got and "\nBQ\t8\t" not in got
    if name == "hand":
        assert "SN\tclipped letters\t3\n" in got and "SN\tmismatch rate\t%.6f\n" % (2 / 18) in got and "SN\tindel rate\t%.6f\n" % (2 / 18) in got
        assert "SU\tT\tA\t1\n" in got and "SU\tA\tG\t1\n" in got and "CY\t10\t1\t0\t0\t1\n" in got
        assert "BQ\t10\t1\t1\t%.2f\n" % 1.76 in got  # -10 log10(2 / 3)


MODES = ["-mam", "-mum", "-smem", "-chain", "-ext", "-aln", "-paf", "-sam", "-pile", "-sites", "-vcf", "-cons", "-depth"]
EXCLUDES = "Option -stats excludes -mam, -mum, -smem, -chain, -ext, -aln, -paf, -sam, -pile, -sites, -vcf, -cons and -depth"


def test_option_row_and_refusals():
    rows = dict(hostlib.option_rows())
    assert rows["stats"] is False and "stats"[0] not in "lomv"
    for args in (["x", "-stats", "r.fa", "q.fq"], ["x", "r.fa", "-b", "q.fq", "-STATS", "-l", "20"],
                 ["x", "-stats", "-mgap", "100", "-pen", "3", "-xdrop", "10", "-maxed", "40", "-minq", "20", "-o", "o.stats", "r.fa", "q.fq"]):
        rc, refusal, v = hostlib.parse_run(args)
        assert (rc, refusal) == (0, None), (args, refusal)
        assert stats_host.parse_stats(args) == 1 and [args[i] for i in v["files"]] == ["r.fa", "q.fq"]
    rc, refusal, v = hostlib.parse_run(["x", "-stats", "-mgap", "100", "-pen", "3", "-xdrop", "10", "-maxed", "40", "-minq", "20", "r.fa", "q.fq"])
    assert (v["max_gap"], v["ext_params"], v["max_edits"], v["min_mapq"]) == (100, [3, 10], 40, 20)
    assert hostlib.parse_options(["x", "-stats", "r.fa", "q.fq"])["match_type"] == 7
    assert stats_host.parse_stats(["x", "-sam", "r.fa", "q.fq"]) == 0 and stats_host.parse_stats(["x", "-s", "q.fq"]) == 0
    for mode in MODES:
        for args in (["x", "-stats", mode, "r.fa", "q.fq"], ["x", mode, "r.fa", "-stats", "q.fq"]):
            rc, refusal, _ = hostlib.parse_run(args)
            assert (rc, refusal) == (-1, EXCLUDES), (args, refusal)
    for extra, message in ((["-mpct", "30"], "Options -mdep and -mpct need -sites"), (["-mdep", "3"], "Options -mdep and -mpct need -sites"),
                           (["-bq", "10"], "Option -bq needs -pile"), (["-dedup"], "Option -dedup needs -pile, -sites, -vcf, -cons or -depth"),
                           (["-gt"], "Option -gt needs -vcf"), (["-sb"], "Option -sb needs -gt"), (["-wq"], "Option -wq needs -gt"),
                           (["-occ", "3"], "Option -occ needs -smem"), (["-evs", "64"], "Option -evs needs -vcf"),
                           (["-lev", "1,2"], "Options -lev and -win need -depth"), (["-err", "20"], "Option -err needs -gt"),
                           (["-minq", "61"], "Option -minq needs a whole number from 0 to 60")):
        rc, refusal, _ = hostlib.parse_run(["x", "-stats"] + extra + ["r.fa", "q.fq"])
        assert (rc, refusal) == (-1, message), (extra, refusal)
    # -minq without a mode that takes it is refused as before
    assert hostlib.parse_run(["x", "-paf", "-minq", "3", "r.fa", "q.fq"])[1] == "Option -minq needs -pile"
