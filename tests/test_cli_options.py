"""The command line's options after they moved into one table (slamem_host.c): what the front end did with a corpus of argument
vectors before the move is what it does now.

tests/cli_options_recorded.json was recorded by tests/tools/gen_cli_corpus.py from commit d419b5b ("Add -gt: ..."), the parent of
the commit that introduced the table: for every vector the return code and outputs of each slh_parse_* entry point, the file
arguments, and the exit status and first "> ERROR:" line of slaMEM-hip without a GPU ("accepted": it got as far as the index
build).  The expectations are that commit's, never the code under test's.  slh_parse_run, which that commit did not have, must
refuse with the executable's recorded line and hand out the values of the old entry points; the table must keep the property
the deleted chain of value-taking options kept by hand; and slh_next_piece, the one walk of the read-outs over the records of
a merged text, is compared with a position-by-position spec."""
import os
import sys

import pytest

import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import gen_cli_corpus as gen  # noqa: E402

EXE = os.path.join(hostlib.HOST_DIR, "slaMEM-hip")


@pytest.fixture(scope="module")
def recorded():
    commit, cases = gen.read_recorded(os.path.join(HERE, "cli_options_recorded.json"))  # (it checks that the corpus is the recorded one)
    assert commit.startswith("d419b5b")
    return cases


def test_entry_points_give_what_the_parent_gave(recorded):
    assert len(recorded) > 700
    for c in recorded:
        assert hostlib.entry_points(c["argv"]) == c["lib"], c["argv"]


def test_executable_refuses_as_the_parent_did(recorded, tmp_path):
    got = gen.run_all(EXE, [c["argv"] for c in recorded], str(tmp_path))
    for c, g in zip(recorded, got):
        assert g == c["exe"], c["argv"]
    assert sum(c["exe"] == "accepted" for c in recorded) > 100 and len({str(c["exe"]) for c in recorded}) > 50


def test_parse_run_refuses_with_the_executables_line_and_hands_out_the_old_values(recorded):
    refusals = set()
    results = [hostlib.parse_run(c["argv"]) for c in recorded]
    for c, (rc, refusal, v) in zip(recorded, results):
        lib, argv = c["lib"], c["argv"]
        assert rc in (0, -1, -2) and (refusal is None) == (rc == 0), argv
        if rc != 0:
            refusals.add(refusal)
            assert c["exe"] == [255, "> ERROR: " + refusal], argv
        if len(argv) < 3:
            assert v["usage"] == 1 and rc == 0
            continue
        for name in ("max_occ", "max_gap", "max_edits", "min_mapq", "min_bq"):
            assert v[name] == lib[name][1], (argv, name)
        assert v["bq_given"] == lib["min_bq"][0]
        depth_default = lib["depth"][0] and lib["sites_params"][0] == 0  # (-depth without -mdep: covered from depth 1)
        assert v["sites_params"] == ([1, lib["sites_params"][2]] if depth_default else lib["sites_params"][1:]), argv
        for name in ("ext_params", "gt_params"):
            assert v[name] == lib[name][1:], (argv, name)
        assert v["event_slots"] == lib["event_slots"][1] and v["dd_slots"] == lib["dedup"][1], argv
        assert v["dedup"] == (lib["dedup"][0] > 0 and lib["dedup"][0] & 1) and v["depth"] == lib["depth"][0], argv
        assert v["levels"] == lib["depth_params"][1] and v["window"] == lib["depth_params"][2], argv
        assert v["files"] == lib["files"], argv
    for c, (rc, refusal, v) in zip(recorded, results):  # what it lets through, the executable refuses for no reason of the parser's
        if rc == 0 and c["exe"] != "accepted":
            assert c["exe"][1] is None or c["exe"][1][len("> ERROR: "):] not in refusals, c["argv"]
    assert len(refusals) > 45


def first_letter_rule(opt):
    return opt[1].lower() in "lomv" and opt[1:3].lower() != "vc"


def test_table_says_which_options_take_the_next_argument():
    rows = hostlib.option_rows()
    names = [n for n, _ in rows]
    assert len(rows) == len(set(names)) > 40
    for opt, (_, inside, _) in gen.VALUES.items():  # every value option of the corpus is a row that takes a value
        assert (opt[1:], True) in rows, opt
    for name in ("pen", "xdrop", "bq", "win", "dslots", "evs", "ploidy", "err", "hetq", "qual"):  # the deleted chain's
        assert (name, True) in rows
    for name, takes in rows:
        if name == "r":
            continue  # (a string of its own rule)
        for opt in ("-" + name, "-" + name.upper()):
            files = hostlib.parse_options(["x", opt, "ref.fa", "a.fa", "b.fa"])["files"]
            want = ["a.fa", "b.fa"] if takes or first_letter_rule(opt) else ["ref.fa", "a.fa", "b.fa"]
            assert files == want, opt
    assert hostlib.parse_options(["x", "-vcf", "ref.fa", "a.fa"])["files"] == ["ref.fa", "a.fa"]
    assert hostlib.parse_options(["x", "-mam", "ref.fa", "a.fa"])["files"] == ["a.fa"]
    assert hostlib.parse_options(["x", "-zz", "ref.fa", "a.fa"])["files"] == ["ref.fa", "a.fa"]


# ---- slh_next_piece ------------------------------------------------------------------------------------------------------------

def spec_pieces(sizes, chunk):
    """Every position of the merged text mapped to its record or to a separator; per range the maximal runs of one record."""
    owner = []
    for k, s in enumerate(sizes):
        owner += [k] * s + [None]
    owner.pop()
    ends, at = [], 0
    for s in sizes:
        at += s
        ends.append(at)
        at += 1
    out = []
    for x0 in range(0, len(owner), chunk):
        got = []
        for x in range(x0, min(x0 + chunk, len(owner))):
            k = owner[x]
            if k is None:
                continue
            if got and got[-1][0] == k and got[-1][2] == x:
                got[-1][2] = x + 1
            else:
                got.append([k, x, x + 1])
        out.append([(k, a, b, int(b == ends[k])) for k, a, b in got])
    return out


PIECE_TEXTS = [[1], [2], [63], [64], [65], [1, 1], [1, 2, 1], [63, 64, 65], [65, 1, 63, 2], [64, 64], [63, 63, 1, 1, 1, 200], [150, 100],
               [129], [5, 130, 5]]


@pytest.mark.parametrize("sizes", PIECE_TEXTS)
def test_next_piece_is_the_position_by_position_walk(sizes):
    total = sum(sizes) + len(sizes) - 1
    for chunk in (1, 2, 64, total + 5):
        got, want = hostlib.pieces(sizes, chunk), spec_pieces(sizes, chunk)
        assert got == want, (sizes, chunk)
        for k, s in enumerate(sizes):  # every row of every record exactly once, and one piece that ends it
            mine = [p for rng in got for p in rng if p[0] == k]
            assert sum(b - a for _, a, b, _ in mine) == s and [e for *_, e in mine].count(1) == 1 and mine[-1][3] == 1


def test_next_piece_cases_of_the_borders():
    # a range that starts on a separator, one that ends on a record's last row, a record over three ranges
    assert hostlib.pieces([64, 64], 64) == [[(0, 0, 64, 1)], [(1, 65, 128, 0)], [(1, 128, 129, 1)]]
    assert hostlib.pieces([63, 64], 64) == [[(0, 0, 63, 1)], [(1, 64, 128, 1)]]
    assert hostlib.pieces([5, 130, 5], 64) == [[(0, 0, 5, 1), (1, 6, 64, 0)], [(1, 64, 128, 0)], [(1, 128, 136, 1), (2, 137, 142, 1)]]
    assert hostlib.pieces([150, 100], 64)[2] == [(0, 128, 150, 1), (1, 151, 192, 0)]
