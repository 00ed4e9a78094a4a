"""Fixtures of the "-v" image tool (tests/golden/image/, made by the real reference: tests/golden/make_image_golden.py).

The FASTA inputs are not stored: the tool uses the records' names and lengths only, so both the generator and the tests write
them from the manifest with the same fixed letters."""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
IMAGE_GOLDEN = os.path.join(HERE, "golden", "image")
RANDOM_CASES = os.path.join(IMAGE_GOLDEN, "random_cases.json")


def manifest():
    return json.load(open(os.path.join(IMAGE_GOLDEN, "manifest.json")))


def write_fasta(path, records):
    """records: [(name, length)]; the letters are a fixed pattern, 70 per line"""
    unit = "ACGTTGCAAGCT" * 6
    with open(path, "w") as f:
        for name, n in records:
            f.write(">%s\n" % name)
            body = (unit * (n // len(unit) + 1))[:n]
            f.write("".join(body[i:i + 70] + "\n" for i in range(0, n, 70)))


def write_inputs(case, entry, where):
    write_fasta(os.path.join(where, "ref.fa"), [tuple(r) for r in entry["reference"]])
    write_fasta(os.path.join(where, "q.fa"), [tuple(q) for q in entry["queries"]])
    with open(os.path.join(IMAGE_GOLDEN, case, "mems.txt"), "rb") as f, open(os.path.join(where, "mems.txt"), "wb") as g:
        g.write(f.read())


def write_random_case(where, seed):
    """ref.fa, q.fa and mems.txt of seeded random case `seed` (tests/test_image_tool.py; the reference's answers to them are
    RANDOM_CASES): 1 to 20 queries shorter and longer than the reference, odd names, few / diagonal / scattered / per-column
    MEMs, names the tool must refuse"""
    rng = random.Random(1000 + seed)
    rn = rng.choice([300, 5000, 123456, 400000, 2500])
    queries = []
    for k in range(rng.choice([1, 2, 3, 5, 9, 20])):
        ql = rng.choice([50, 400, rn // 2, rn, rn * 2 if rn < 200000 else rn // 3, 1234])
        name = rng.choice(["q%d" % k, "read_%d some description here that is long" % k, "x" * rng.randint(1, 300) + str(k),
                           "Reverse%d" % k, "we|rd~{}[]%d" % k, "tab\tname%d" % k])
        queries.append((name, ql))
    write_fasta(os.path.join(where, "ref.fa"), [(rng.choice(["ref", "gi|123|some reference, complete genome", "R" * 200]), rn)])
    write_fasta(os.path.join(where, "q.fa"), queries)
    mode = rng.choice(["scatter", "diag", "few", "noise"])
    with open(os.path.join(where, "mems.txt"), "w") as f:
        for name, ql in queries:
            for strand in (0, 1):
                f.write(">%s%s\n" % (name, " Reverse" if strand else ""))
                if mode == "noise":
                    step = max(1, ql // 1000)
                    for qp in range(1, ql + 1, step):
                        ln = max(1, min(rng.randint(1, step), ql - qp + 1, rn))
                        f.write("%d\t%d\t%d\n" % (rng.randint(1, rn - ln + 1), qp, ln))
                    continue
                for _ in range(rng.randint(0, 5) if mode == "few" else rng.randint(0, 400)):
                    ln = max(1, min(rng.randint(1, max(1, min(ql, rn) // rng.choice([1, 3, 10, 100]))), ql, rn))
                    qp = rng.randint(1, ql - ln + 1)
                    rp = min(max(1, qp + rng.randint(-5, 5)), rn - ln + 1) if mode == "diag" else rng.randint(1, rn - ln + 1)
                    f.write("%d\t%d\t%d\n" % (rp, qp, ln))
