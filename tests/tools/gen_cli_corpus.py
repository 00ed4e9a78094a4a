"""The corpus of argument vectors behind tests/test_cli_options.py, and the recorder of what a build of the front end does
with them.

    python tests/tools/gen_cli_corpus.py <root of a built checkout> <out.json>

runs every vector through each slh_parse_* entry point of that checkout's libslamem_host.so and through its slaMEM-hip (with no
GPU visible, as the refusal tests do) and writes the results.  tests/cli_options_recorded.json is the output for the commit named
in it; the test replays it against the current build.  REF and QRY in a vector stand for a small reference and a query file.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

MODES = ["-mem", "-mam", "-mum", "-smem", "-chain", "-ext", "-aln", "-paf", "-sam", "-pile", "-sites", "-vcf", "-cons", "-depth"]
SWITCHES = ["-dedup", "-gt", "-b", "-n"]
# value options: the mode that lets them through, the values just inside and just outside the range
VALUES = {
    "-occ": ("-smem", ["1", "2147483647"], ["0", "2147483648"]),
    "-mgap": ("-chain", ["1", "2147483647"], ["0", "2147483648"]),
    "-pen": ("-ext", ["1", "2147483647"], ["0", "2147483648"]),
    "-xdrop": ("-ext", ["0", "2147483647"], ["-1", "2147483648"]),
    "-maxed": ("-aln", ["0", "127"], ["-1", "128"]),
    "-minq": ("-pile", ["0", "60"], ["-1", "61"]),
    "-bq": ("-pile", ["0", "93"], ["-1", "94"]),
    "-mdep": ("-sites", ["1", "2147483647"], ["0", "2147483648"]),
    "-mpct": ("-sites", ["0", "100"], ["-1", "101"]),
    "-evs": ("-vcf", ["64", "2147483648"], ["32", "4294967296", "96"]),
    "-dslots": ("-pile -dedup", ["64", "4294967296"], ["32", "8589934592", "96"]),
    "-ploidy": ("-vcf -gt", ["1", "2"], ["0", "3"]),
    "-err": ("-vcf -gt", ["1", "93"], ["0", "94"]),
    "-hetq": ("-vcf -gt", ["0", "999"], ["-1", "1000"]),
    "-qual": ("-vcf -gt", ["0", "999"], ["-1", "1000"]),
    "-lev": ("-depth", ["1", "1,2,4294967295", ",".join(str(k) for k in range(1, 17))],
             ["0", "2,2", "3,2", "4294967296", ",".join(str(k) for k in range(1, 18)), "1,", ",1", "+1"]),
    "-win": ("-depth", ["1", "18446744073709551615"], ["0", "18446744073709551616", "+1", " 1"]),
    "-l": ("-mem", ["1", "20"], ["0", "-5"]),
    "-m": ("-mem", ["0", "50"], ["-1", "x"]),
}
FILES = ["REF", "QRY"]


def corpus():
    out = []

    def add(*args):
        v = ["slaMEM-hip"] + [a for a in args]
        if v not in out:
            out.append(v)
    singles = MODES + SWITCHES + list(VALUES) + ["-o", "-v", "-r", "-s", "-c", "-x", "-"]
    for opt in singles:  # every option alone, in upper case, and by its first two letters
        add(opt, *FILES)
        add(opt.upper(), *FILES)
        add(opt[:3], *FILES)
    for a in MODES:  # every ordered pair of mode options
        for b in MODES:
            if a != b:
                add(a, b, *FILES)
    for opt, (mode, inside, outside) in VALUES.items():
        m = mode.split()
        for v in inside + outside + ["7x", "x", "", "1.5"]:
            add(*m, opt, v, *FILES)
            add(opt, v, *FILES)  # (without its mode: "needs")
        add(*m, *FILES, opt)  # the value is missing
        add(*m, opt.upper(), inside[0], *FILES)
        add(*m, opt, inside[0], opt, "x", *FILES)  # twice: the first or the last counts
        add(*m, opt, "x", opt, inside[0], *FILES)
        add(opt, inside[0], *m, *FILES)  # before, between and after the two file names
        add(*m, "REF", opt, inside[0], "QRY")
        add(*m, *FILES, opt, inside[0])
    # the -m family, the -de / -ds family, -v against -vcf
    for args in (["-mam", "-maxed", "3"], ["-maxed", "3"], ["-aln", "-maxed", "3", "-mam"], ["-aln", "-max", "3"], ["-aln", "-maX", "3"],
                 ["-ma"], ["-max"], ["-mam", "QRY"], ["-mum", "-mam"], ["-mgap", "5", "-minq", "3", "-pile"], ["-pile", "-mdep", "3", "-mpct", "5"],
                 ["-sites", "-mdep", "3", "-mpct", "5"], ["-cons", "-mpct", "5"], ["-depth", "-mpct", "5"], ["-vcf", "-gt", "-mpct", "5"],
                 ["-cons", "-mdep", "2"], ["-depth", "-mdep", "2"], ["-mi", "3"], ["-md", "3"], ["-mp", "3"], ["-mg", "3"], ["-m", "3"],
                 ["-me"], ["-mx", "3"], ["-depth"], ["-dedup"], ["-depth", "-dedup"], ["-dedup", "-depth"], ["-de"], ["-ded"], ["-DED", "-pile"],
                 ["-dslots", "64"], ["-dslots", "64", "-dedup"], ["-depth", "-dedup", "-dslots", "128"], ["-ds", "64", "-ded", "-pile"],
                 ["-depth", "-lev", "1,2", "-win", "5"], ["-lev", "1,2", "-win", "5"], ["-depth", "-win", "7"], ["-v"], ["-vcf"], ["-vc"],
                 ["-V", "x.txt"], ["-vcf", "-v", "x.txt"], ["-vcf", "-gt"], ["-gt"], ["-sites", "-gt"], ["-vcf", "-evs", "128"],
                 ["-cons", "-evs", "128"], ["-sites", "-evs", "128"], ["-pen", "-xdrop", "3", "-ext"], ["-ext", "-pen", "2", "-xdrop", "9"],
                 ["-vcf", "-gt", "-ploidy", "1", "-err", "25", "-hetq", "10", "-qual", "0"], ["-qual", "3", "-hetq", "4"], ["-sam", "-bq", "3"],
                 ["-r", "name"], ["-r"], ["-r", "'two", "words'"], ["-r", "\"open"], ["-b", "-l", "10"], ["-o", "out.txt", "-b"]):
        add(*args, *FILES)
    add()
    add("REF")
    add("REF", "QRY")
    add("-pile", "REF")
    add("-s", "REF")
    add("-c", "REF")
    add("QRY", "-r")
    return out


def write_inputs(d):
    ref, qry = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")
    with open(ref, "wb") as f:
        f.write(b">r\n" + b"ACGT" * 30 + b"\n")
    with open(qry, "wb") as f:
        f.write(b">q\n" + b"ACGT" * 10 + b"\n")
    return {"REF": ref, "QRY": qry}


def run_exe(exe, args, d):
    """(exit status, the first "> ERROR:" line) of the executable without a GPU, or "accepted" when it got as far as the index."""
    paths = write_inputs(d)
    r = subprocess.run([exe] + [paths.get(a, a) for a in args[1:]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=d,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
    if b"Building index" in r.stdout:
        return "accepted"
    err = [l for l in r.stdout.split(b"\n") if l.startswith(b"> ERROR:")]
    return [r.returncode, err[0].decode(errors="replace").replace(d, "DIR") if err else None]


def run_all(exe, vectors, base):
    def one(kv):
        k, v = kv
        d = os.path.join(base, "c%d" % k)
        os.makedirs(d, exist_ok=True)
        return run_exe(exe, v, d)
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, enumerate(vectors)))


BASELINE = ["slaMEM-hip", "REF", "QRY"]  # the vector whose results the file spells out; the others say where they differ


def corpus_digest(vectors):
    return hashlib.sha256(json.dumps(vectors).encode()).hexdigest()


def write_recorded(path, commit, vectors, libs, exes):
    """One line per vector, in the corpus's order: [the entry points' results that differ from the baseline's, the number of the
    executable's outcome in "outcomes"]; of "options" only the fields that differ, by their position."""
    base = libs[vectors.index(BASELINE)]
    outcomes = []
    for e in exes:
        if e not in outcomes:
            outcomes.append(e)

    def diff(lib):
        d = {k: v for k, v in lib.items() if v != base[k]}
        if "options" in d:
            d["options"] = {str(i): v for i, (v, w) in enumerate(zip(lib["options"], base["options"])) if v != w}
        return d
    dumps = lambda x: json.dumps(x, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"recorded_from":%s,"corpus_sha256":%s,\n"baseline":%s,\n"outcomes":[\n%s\n],\n"cases":[\n'
                % (dumps(commit), dumps(corpus_digest(vectors)), dumps(base), ",\n".join(dumps(e) for e in outcomes)))
        f.write(",\n".join(dumps([diff(lib), outcomes.index(e)]) for lib, e in zip(libs, exes)) + "\n]}\n")


def read_recorded(path):
    """[{"argv", "lib", "exe"}] of a file that write_recorded wrote for today's corpus, and the commit it was recorded from."""
    with open(path) as f:
        d = json.load(f)
    vectors, base = corpus(), d["baseline"]
    assert d["corpus_sha256"] == corpus_digest(vectors) and len(d["cases"]) == len(vectors)
    out = []
    for v, (diff, e) in zip(vectors, d["cases"]):
        lib = dict(base, **diff)
        if "options" in diff:
            lib["options"] = [diff["options"].get(str(i), w) for i, w in enumerate(base["options"])]
        out.append({"argv": v, "lib": lib, "exe": d["outcomes"][e]})
    return d["recorded_from"], out


def main():
    import hostlib
    root, out = sys.argv[1], sys.argv[2]
    L = C.CDLL(os.path.join(root, "slamem_amd", "host", "libslamem_host.so"))
    exe = os.path.join(root, "slamem_amd", "host", "slaMEM-hip")
    commit = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    vectors = corpus()
    with tempfile.TemporaryDirectory() as base:
        exes = run_all(exe, vectors, base)
    write_recorded(out, commit, vectors, [hostlib.entry_points(v, L) for v in vectors], exes)
    print(len(vectors), "cases recorded from", commit)


if __name__ == "__main__":
    main()
