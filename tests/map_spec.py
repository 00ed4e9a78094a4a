"""-paf on the checker side: one mapping per read with a mapping quality, straight from the definition of DESIGN.md 4.15, and
the PAF lines.  Builds on chain_spec (the best chain and its score) and aln_spec (the segments of a block); restates neither.

For one read of n letters its strand blocks are those of -mem in block order (forward; forward then reverse under -b):

  chains     per block b with rows R_b: (K_b, c_b) = chain_spec's best chain and score; R'_b = R_b without the rows of K_b, in
             the same order; c'_b = chain_spec's score of R'_b (0 when it is empty)
  primary    the block with the largest c_b, the first in block order on a tie; s1 = its score; s1 == 0: unmapped (no segments,
             strand 0, mapq 0, s2 0)
  s2         max(c'_primary, c_other)
  mapq       (60 * (s1 - s2)) // s1
  segments   aln_spec's segments of the primary block; the other block is not aligned
  PAF        a line per segment: name, n, qs, qe, strand, record, record length, ts, te, letters under =, all operation
             lengths, mapq, NM:i:, s1:i:, s2:i:, cg:Z: -- qs = query_pos on the forward strand, n - query_pos - query_len on the
             reverse strand; ts local to the record that holds the segment's first reference letter

strand: 0 unmapped, 1 forward, 2 reverse.  Python integers: no overflow."""
import numpy as np

import aln_spec
import chain_spec
import ext_spec
import mum_spec


def block_scores(rows, G: int = chain_spec.DEFAULT_GAP):
    """(c_b, c'_b) of one block."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    windowed = len(rows) > 200
    keep, c = chain_spec.block_chain(rows, G, windowed=windowed)
    rest = rows[~keep]
    return c, (chain_spec.block_chain(rest, G, windowed=windowed)[1] if len(rest) else 0)


def read_map(blocks, read, T, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
             E: int = aln_spec.DEFAULT_EDITS):
    """blocks: the read's one or two row arrays in block order; read: its letters as given.  Returns (strand, mapq, s1, s2,
    segments as aln_spec.block_aln gives them)."""
    sc = [block_scores(r, G) for r in blocks]
    prim = max(range(len(blocks)), key=lambda b: (sc[b][0], -b))
    s1 = sc[prim][0]
    if s1 == 0:
        return 0, 0, 0, 0, []
    s2 = max([sc[prim][1]] + [sc[b][0] for b in range(len(blocks)) if b != prim])
    rec = np.frombuffer(ext_spec._letters(read), dtype=np.uint8)
    Q = bytes(ext_spec.revcomp(rec)) if prim else bytes(rec)
    return 1 + prim, (60 * (s1 - s2)) // s1, s1, s2, aln_spec.block_aln(blocks[prim], Q, T, G, P, X, E)


def filter_reads(mem, boff, ref, queries, offsets, both: bool, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY,
                 X: int = ext_spec.DEFAULT_XDROP, E: int = aln_spec.DEFAULT_EDITS):
    """The -paf result of a -mem result as the engine returns it: a read_map tuple per read (pack() gives the arrays)."""
    tri = ext_spec._tri(mem)
    boff = np.asarray(boff, dtype=np.int64)
    T = ext_spec._letters(ref)
    q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    strands = 2 if both else 1
    assert len(boff) - 1 == (len(off) - 1) * strands
    out = []
    for r in range(len(off) - 1):
        blocks = [tri[boff[r * strands + s]:boff[r * strands + s + 1]] for s in range(strands)]
        out.append(read_map(blocks, q[off[r]:off[r + 1]], T, G, P, X, E))
    return out


def pack(reads):
    """read_map tuples -> what the engine returns: (segments (n, 5) int64, read offsets, ops uint32, op offsets, (n, 4) int64
    of strand, mapq, s1, s2)."""
    segs, roff, ops, ooff = aln_spec.pack([r[4] for r in reads])
    return segs, roff, ops, ooff, np.array([r[:4] for r in reads], dtype=np.int64).reshape(-1, 4)


# ---- PAF ---------------------------------------------------------------------------------------------------------------------

def cut_name(name: bytes) -> bytes:
    for k, c in enumerate(name):
        if c in b" \t":
            return name[:k]
    return name


def paf_lines(name: bytes, n: int, result, ref) -> bytes:
    """The PAF lines of one read.  ref: hostlib.Loaded of the merged reference (names, sizes, merged_start)."""
    strand, mapq, s1, s2, segl = result
    out = []
    starts = ref.merged_start
    for (p, q, rlen, qlen, ed, rl) in segl:
        r = max(i for i in range(len(starts)) if starts[i] <= p) if ref.s.num > 1 else 0
        ts = p - (starts[r] if ref.s.num > 1 else 0)
        qs = q if strand == 1 else n - q - qlen
        f = [cut_name(name), b"%d" % n, b"%d" % qs, b"%d" % (qs + qlen), b"+" if strand == 1 else b"-", cut_name(ref.names[r]),
             b"%d" % ref.sizes[r], b"%d" % ts, b"%d" % (ts + rlen), b"%d" % sum(k for c, k in rl if c == "="),
             b"%d" % sum(k for _, k in rl), b"%d" % mapq, b"NM:i:%d" % ed, b"s1:i:%d" % s1, b"s2:i:%d" % s2,
             b"cg:Z:" + aln_spec.cigar_string(rl).encode()]
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def paf_file(reads, names, lengths, ref) -> bytes:
    return b"".join(paf_lines(names[i], int(lengths[i]), r, ref) for i, r in enumerate(reads))


def golden_map(case, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
               E: int = aln_spec.DEFAULT_EDITS):
    """-paf of the file the real reference wrote for the -mem case: (read_map tuples, per-read row blocks, reference, queries,
    options)."""
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    blocks = mum_spec.parse_mems_file(open(exp_mems, "rb").read(), ref)
    strands = 2 if "-b" in opts else 1
    assert len(blocks) == qs.n * strands
    chars = np.frombuffer(qs.chars, dtype=np.uint8)
    T = ext_spec._letters(ref.chars)
    out, rows = [], []
    for i in range(qs.n):
        bl = [blocks[i * strands + s][1].astype(np.int64) for s in range(strands)]
        rows.append(bl)
        out.append(read_map(bl, chars[qs.offsets[i]:qs.offsets[i + 1]], T, G, P, X, E))
    return out, rows, ref, qs, opts


def golden_paf_file(case, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
                    E: int = aln_spec.DEFAULT_EDITS) -> bytes:
    reads, _, ref, qs, _ = golden_map(case, G, P, X, E)
    return paf_file(reads, qs.names, qs.sizes, ref)


# ---- known answers that do not go through the definition ---------------------------------------------------------------------

def unique_reads(seed: int, count: int = 200, ref_len: int = 40000, read_len: int = 200, sub_rate: float = 0.02):
    """Reads of read_len letters from both strands of a uniform random reference over A,C,G,T, each letter substituted with
    probability sub_rate.  Returns (reference, reads, offsets, [(start in the reference, strand 1 or 2)])."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=ref_len)
    reads, truth = [], []
    for k in range(count):
        a = int(rng.integers(0, ref_len - read_len))
        r = ref[a:a + read_len].copy()
        for x in np.nonzero(rng.random(read_len) < sub_rate)[0]:
            r[x] = rng.choice(acgt[acgt != r[x]])
        rev = bool(rng.integers(0, 2))
        reads.append(ext_spec.revcomp(r) if rev else r)
        truth.append((a, 2 if rev else 1))
    off = (np.arange(count + 1, dtype=np.uint64) * np.uint64(read_len))
    return ref, np.concatenate(reads), off, truth


def duplicated_reads(seed: int, count: int = 60, ref_len: int = 20000, copy_len: int = 1500, read_len: int = 150):
    """A random reference in which [2000, 2000 + copy_len) is copied verbatim to [12000, 12000 + copy_len), and exact reads
    that lie wholly inside the first copy (forward strand).  Returns (reference, reads, offsets)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=ref_len)
    ref[12000:12000 + copy_len] = ref[2000:2000 + copy_len]
    reads = []
    for k in range(count):
        a = 2000 + int(rng.integers(1, copy_len - read_len - 1))
        reads.append(ref[a:a + read_len].copy())
    off = (np.arange(count + 1, dtype=np.uint64) * np.uint64(read_len))
    return ref, np.concatenate(reads), off
