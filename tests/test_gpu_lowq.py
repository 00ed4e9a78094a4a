"""The low-quality mask on the MI355X: slamem_pileup_add_masked_device, k_lowq_pack, a stream's submit_masked and
slaMEM-hip -bq, every table compared for exact equality with tests/lowq_spec.py applied to map_spec.filter_reads of the same
engine's -mem list.  One reference of 4 kbp and one batch, mapped by the spec once: reads that are copies of the reference with
planted substitutions, so that their = runs are known -- a run of each length 1, 63, 64, 65, 128, 129 whose first letter sits at
each bit offset 0 .. 63 of a mask word --, reverse-strand reads of every length up to 130, a read with an insertion, one with a
deletion, one over the text's N, and segments of 33 and of more than 64 operations.  The masks are made from the spec's own runs."""
import os
import subprocess

import numpy as np
import pytest

import ext_spec
import lowq_spec
import map_spec
import pile_spec
import prims
from test_gpu_aln import batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MIN_LEN = 14
RUN_LENGTHS = (1, 63, 64, 65, 128, 129)
N_AT = 2000  # the text's one N


def other(letter, rng):
    return rng.choice(ACGT[ACGT != (letter & 0xDF)])


def make_batch():
    rng = np.random.default_rng(20)
    ref = rng.choice(ACGT, size=4096).astype(np.uint8)
    ref[N_AT] = ord("N")
    reads = []

    def copy(a, n, subs=()):
        r = ref[a:a + n].copy()
        for x in subs:
            r[x] = other(r[x], rng)
        return r
    # A: 24 matching letters, a substitution, a run of k, a substitution, then matching letters up to a length of 1 modulo 64 --
    # the batch's offsets step through every residue, so the run of k (its first letter is letter 25) starts at every bit offset
    first_a = len(reads)
    for j in range(64):
        k = RUN_LENGTHS[j % 6]
        n = 24 + 1 + k + 1 + 24
        n += (1 - n) % 64
        a = 100 + 37 * j
        if a <= N_AT < a + n:  # (not over the text's N: group C has that)
            a = N_AT + 1 + j
        reads.append(copy(a, n, (24, 25 + k)))
    # B: the reverse strand, every length from 1 to 130 (those below the minimum match length stay unmapped and only shift the
    # offsets); every third one with a substitution
    first_b = len(reads)
    for n in range(1, 131):
        a = 2100 + 13 * n
        reads.append(ext_spec.revcomp(copy(a, n, (n // 2,) if n % 3 == 0 and n > 40 else ())))
    # C: an insertion of three letters, a deletion of three rows, the text's N inside an anchor, on both strands
    first_c = len(reads)
    r = copy(300, 120)
    reads.append(np.concatenate([r[:60], other(r[60], rng).repeat(3), r[60:]]).astype(np.uint8))
    r = copy(700, 123)
    reads.append(np.concatenate([r[:60], r[63:]]))
    reads.append(copy(N_AT - 50, 130, (20,)))
    reads.append(ext_spec.revcomp(copy(N_AT - 70, 131, (100,))))
    reads.append(ext_spec.revcomp(reads[first_c].copy()))
    reads.append(ext_spec.revcomp(reads[first_c + 1].copy()))
    # D: segments of 33 and of 81 operations (a substitution every 20 letters): the wave kernel, its second trip included
    first_d = len(reads)
    reads.append(copy(1000, 16 * 20 + 19, range(19, 16 * 20, 20)))
    reads.append(copy(2200, 40 * 20 + 19, range(19, 40 * 20, 20)))
    reads.append(ext_spec.revcomp(copy(2300, 40 * 20 + 19, range(19, 40 * 20, 20))))
    reads.append(copy(3900, 67))  # the last read ends in the buffer's last word
    q, off = batch(reads)
    return ref, q, off, dict(a=first_a, b=first_b, c=first_c, d=first_d)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


@pytest.fixture(scope="module")
def world(eng):
    """The index, the batch and what the spec maps it to -- computed once, read by every test, changed by none."""
    ref, q, off, first = make_batch()
    idx = eng.Index.build(ref)
    mem, mem_boff = idx.find_mems(q, off, MIN_LEN, True)
    res = map_spec.filter_reads(mem, mem_boff, ref, q, off, True)
    yield dict(ref=ref, q=q, off=off, first=first, idx=idx, res=res, n=len(ref), total=int(off[-1]))
    idx.close()


def runs(w, kinds="="):
    """(read, strand, first global letter index of the run as given ... ) per operation of the kinds: (r, strand, p, q, k, lo, hi)
    with [lo, hi) the global indices of its letters in the buffer (on strand 2 the mirrored range)."""
    out = []
    for r, (strand, _mapq, _s1, _s2, segl) in enumerate(w["res"]):
        if strand == 0:
            continue
        a, b = int(w["off"][r]), int(w["off"][r + 1])
        for (p, qq, _rl, _ql, _ed, ops) in segl:
            p, qq = int(p), int(qq)
            for c, k in ops:
                k = int(k)
                if c in kinds:
                    lo, hi = (a + qq, a + qq + k) if strand == 1 else (b - qq - k, b - qq)
                    out.append((r, strand, p, qq, k, lo, hi))
                if c in "=XD":
                    p += k
                if c in "=XI":
                    qq += k
    return out


def same(got, want):
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.nonzero((got.astype(np.int64) != want).any(axis=1))[0]
    assert len(bad) == 0, "rows %s: got %s, want %s" % (bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())


def piled(eng, w, mask, q=None, off=None, pile=None, **kw):
    """The table after one add of the batch with `mask` (bits per letter, words, a tensor, or None)."""
    p = eng.Pileup(w["idx"], **kw) if pile is None else pile
    if mask is not None and not hasattr(mask, "data_ptr") and np.asarray(mask).dtype != np.uint64:
        mask = lowq_spec.from_bits(mask)
    p.add(w["q"] if q is None else q, w["off"] if off is None else off, MIN_LEN, True, lowq=mask)
    if pile is not None:
        return None
    t = p.counts()
    p.close()
    return t


def want_table(w, bits):
    return lowq_spec.pile(w["res"], w["q"], w["off"], w["n"], None if bits is None else lowq_spec.from_bits(bits))


def test_the_batch_is_what_it_claims(world):
    w = world
    res, first = w["res"], w["first"]
    eq = runs(w, "=")
    # group A: every read mapped forward as planned, its run of k between two X at letters 24 and 25 + k
    for j in range(64):
        r, k = first["a"] + j, RUN_LENGTHS[j % 6]
        assert res[r][0] == 1 and int(w["off"][r]) % 64 == j
        mine = [(q, kk) for (rr, _s, _p, q, kk, _lo, _hi) in eq if rr == r]
        assert (25, k) in mine, (j, mine)
    starts = {(lo % 64, k) for (r, _s, _p, q, k, lo, _hi) in eq if first["a"] <= r < first["b"] and q == 25}
    assert {s for s, _ in starts} == set(range(64)) and {k for _, k in starts} == set(RUN_LENGTHS)
    # group B: lengths from the minimum match length on are mapped to strand 2
    assert all(res[first["b"] + n - 1][0] == (2 if n >= MIN_LEN else 0) for n in range(1, 131))
    # group C: an I, a D, and an = run over the text's N on either strand
    ops = lambda r: [c for seg in res[r][4] for c, _ in seg[5]]
    assert "I" in ops(first["c"]) and "D" in ops(first["c"] + 1) and "I" in ops(first["c"] + 4) and "D" in ops(first["c"] + 5)
    assert res[first["c"] + 4][0] == 2 and res[first["c"] + 5][0] == 2
    over_n = {s for (r, s, p, _q, k, _lo, _hi) in eq if p <= N_AT < p + k}
    assert over_n == {1, 2}
    # group D: one segment of 33 operations, two of 81
    assert [len(seg[5]) for seg in res[first["d"]][4]] == [33]
    assert [len(seg[5]) for seg in res[first["d"] + 1][4]] == [81] and [len(seg[5]) for seg in res[first["d"] + 2][4]] == [81]
    assert res[first["d"] + 2][0] == 2
    # reads share words, and the last one ends in the last word
    assert any(int(o) % 64 for o in w["off"][1:-1]) and w["total"] % 64 != 0
    assert len(runs(w, "X")) > 150


def masks_of(w):
    """name -> bits per letter, made from the spec's runs"""
    total, off = w["total"], w["off"]
    eq, xs = runs(w, "="), runs(w, "X")
    rng = np.random.default_rng(6)
    m = {}
    z = lambda: np.zeros(total, dtype=np.uint8)
    given_first = lambda e: e[5] if e[1] == 1 else e[6] - 1   # the global index of the run's first letter in the scanned strand
    given_last = lambda e: e[6] - 1 if e[1] == 1 else e[5]
    b = z(); b[[given_first(e) for e in eq]] = 1; m["first_letter_of_every_run"] = b
    b = z(); b[[given_last(e) for e in eq]] = 1; m["last_letter_of_every_run"] = b
    b = z(); b[[given_first(e) for e in eq] + [given_last(e) for e in eq]] = 1; m["both_ends_of_every_run"] = b
    edges = np.arange(64, total, 64)
    b = z(); b[edges - 1] = 1; m["last_bit_of_every_word"] = b
    b = z(); b[edges] = 1; m["first_bit_of_every_word"] = b
    b = z(); b[edges - 1] = 1; b[edges] = 1; m["both_sides_of_every_word_boundary"] = b
    b = z()
    for e in eq:
        if e[4] >= 6:
            b[e[5] + 3] = b[e[5] + 4] = 1
    m["two_adjacent_bits"] = b
    b = z(); b[[e[5] for e in xs]] = 1; m["every_x_letter"] = b
    b = z(); b[[e[5] for e in xs[::2]]] = 1; m["every_other_x_letter"] = b
    m["all"] = np.ones(total, dtype=np.uint8)
    b = z()
    for r in range(0, len(off) - 1, 2):
        b[int(off[r]):int(off[r + 1])] = 1
    m["all_ones_reads_beside_all_zero_reads"] = b
    m["the_other_reads"] = 1 - b
    # one bit per read: its first given letter, its last, its middle (the reverse-strand reads of every length among them)
    nq = len(off) - 1
    lens = (off[1:] - off[:-1]).astype(np.int64)
    have = lens > 0
    b = z(); b[off[:-1][have].astype(np.int64)] = 1; m["first_letter_of_every_read"] = b
    b = z(); b[(off[1:][have] - 1).astype(np.int64)] = 1; m["last_letter_of_every_read"] = b
    b = z(); b[(off[:-1][have] + lens[have] // 2).astype(np.int64)] = 1; m["middle_letter_of_every_read"] = b
    # around the N, the I and the D
    b = z()
    for (r, s, p, q, k, lo, hi) in eq:
        if p <= N_AT < p + k:
            j = lo + (N_AT - p) if s == 1 else hi - 1 - (N_AT - p)
            b[[j - 2, j - 1, j + 1, j + 3]] = 1
    m["both_sides_of_the_n"] = b
    b = z()
    for (r, s, p, q, k, lo, hi) in runs(w, "I"):
        b[lo:hi] = 1
    m["under_the_insertions"] = b
    m["random_2_percent"] = (rng.random(total) < 0.02).astype(np.uint8)
    m["random_half"] = (rng.random(total) < 0.5).astype(np.uint8)
    assert nq > 0 and all(v.shape == (total,) for v in m.values())
    return m


def test_masked_add_equals_the_spec(eng, world):
    w = world
    plain = piled(eng, w, None)
    same(plain, pile_spec.pile(w["res"], w["q"], w["off"], w["n"]))
    masks = masks_of(w)
    changed = 0
    for name, bits in masks.items():
        want = want_table(w, bits)
        got = piled(eng, w, bits)
        try:
            same(got, want)
        except AssertionError as e:
            raise AssertionError("mask %s: %s" % (name, e))
        changed += int((want != plain.astype(np.int64)).any())
        # D and I are as without a mask
        assert np.array_equal(got[:, 4:], plain[:, 4:]), name
    assert changed >= len(masks) - 1  # (only the bits under the insertions change nothing)
    assert np.array_equal(piled(eng, w, masks["under_the_insertions"]), plain)
    everything = piled(eng, w, masks["all"])
    assert not everything[:, :4].any() and everything[:, 4:].any()  # all bits set: the reads contribute only D and I


def test_no_bit_and_no_mask_are_the_existing_add(eng, world):
    import torch
    from slamem_amd import capi
    w = world
    plain = piled(eng, w, None)
    assert np.array_equal(piled(eng, w, np.zeros(w["total"], dtype=np.uint8)), plain)
    # lowq=None is the existing entry point, a mask without a set bit the masked kernels: the same table bit for bit
    idx, L = w["idx"], capi.lib()
    p = eng.Pileup(idx)
    p.add(w["q"], w["off"], MIN_LEN, True, lowq=torch.zeros((w["total"] + 63) // 64, dtype=torch.int64, device=idx.device))
    assert np.array_equal(p.counts(), plain)
    p.close()
    qd = torch.zeros(64, dtype=torch.uint8, device=idx.device)
    dummy = qd.data_ptr()
    assert L.slamem_pileup_add_masked_device(None, dummy, dummy, 0, dummy, dummy, dummy, dummy, dummy, 0, None, None) == capi.SLAMEM_ERR_ARG
    p = eng.Pileup(idx)
    assert L.slamem_pileup_add_masked_device(p._h, dummy, dummy, 0, dummy, dummy, dummy, dummy, dummy, 61, dummy, None) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_add_masked_device(p._h, dummy, dummy, 0, dummy, dummy, dummy, dummy, dummy, 0, None, None) == capi.SLAMEM_OK
    assert not p.counts().any()
    with pytest.raises(ValueError):
        p.add(w["q"], w["off"], MIN_LEN, True, lowq=np.zeros(1, dtype=np.uint64))  # too few words
    with pytest.raises(ValueError):
        p.add(w["q"], w["off"], MIN_LEN, True, lowq=np.zeros(w["total"], dtype=np.uint8))  # not words
    p.close()


def test_guarded_mask_of_exactly_the_words(eng, world):
    """The mask in an allocation of exactly (total + 63) / 64 words between two guards whose bytes are all 0xA5: the last read
    ends in the last word, and the table is the spec's -- a window that took a word from behind the mask would have seen set bits."""
    import torch
    w = world
    bits = masks_of(w)["random_2_percent"]
    words = lowq_spec.from_bits(bits)
    assert len(words) == (w["total"] + 63) // 64 and w["total"] % 64 != 0
    g = prims.Guarded.of(words)
    t = g.buf[prims.GUARD:prims.GUARD + g.nbytes].view(torch.int64)
    assert t.data_ptr() == g.ptr
    same(piled(eng, w, t), want_table(w, bits))
    assert g.guards_intact() and np.array_equal(g.payload(np.uint64), words)
    # the last read alone, all of its letters low, in front of the rear guard
    bits = np.zeros(w["total"], dtype=np.uint8)
    bits[int(w["off"][-2]):] = 1
    g = prims.Guarded.of(lowq_spec.from_bits(bits))
    same(piled(eng, w, g.buf[prims.GUARD:prims.GUARD + g.nbytes].view(torch.int64)), want_table(w, bits))
    assert g.guards_intact()


def test_batches_in_either_order_and_events(eng, world):
    w = world
    bits = masks_of(w)["random_half"]
    want = want_table(w, bits)
    nq = len(w["off"]) - 1
    h = nq // 2 + 1
    cut = int(w["off"][h])
    assert cut % 64 != 0  # (the second half's mask is the first one's shifted by a part of a word: packed anew)
    parts = [(w["q"][:cut], w["off"][:h + 1].copy(), bits[:cut]), (w["q"][cut:], (w["off"][h:] - w["off"][h]).astype(np.uint64), bits[cut:])]
    for order in ((0, 1), (1, 0)):
        p = eng.Pileup(w["idx"])
        for k in order:
            piled(eng, w, parts[k][2], parts[k][0], parts[k][1], pile=p)
        same(p.counts(), want)
        p.close()
    # events=True: the indel events are those of the unmasked add, the table is the masked one
    a, b = eng.Pileup(w["idx"], events=True), eng.Pileup(w["idx"], events=True)
    piled(eng, w, None, pile=a)
    piled(eng, w, masks_of(w)["all"], pile=b)
    ea, eb = a.events(), b.events()
    assert len(ea[0]) == 2 and int(ea[0]['fwd'].sum()) == 2 and int(ea[0]['rev'].sum()) == 2 and np.array_equal(ea[0], eb[0]) and ea[1] == eb[1]
    assert not b.counts()[:, :4].any() and np.array_equal(b.counts()[:, 4:], a.counts()[:, 4:])
    a.close()
    b.close()


def test_stream_submit_masked_equals_add(eng, world):
    from slamem_amd import capi
    w = world
    bits = masks_of(w)["random_half"]
    words = lowq_spec.from_bits(bits)
    want = want_table(w, bits)
    nq = len(w["off"]) - 1
    per = (nq + 2) // 3
    wins = [w["off"][b * per: min(nq, (b + 1) * per) + 1].copy() for b in range(3)]
    assert all(int(x[0]) % 64 for x in wins[1:])  # windows of the one offsets array: offsets[0] != 0, and inside a word
    for slots in (2, 4):
        p = eng.Pileup(w["idx"])
        st = eng.Stream(w["idx"], slots, 1 << 16, per, True, pile=p)
        done = 0
        for b in range(3):
            st.submit_masked(w["q"], words, wins[b], MIN_LEN)
            if b - done + 1 >= slots - 1:
                st.next(); done += 1
        while done < 3:
            st.next(); done += 1
        st.close()
        same(p.counts(), want)
        p.close()
    # submit and submit_masked(None) on such a stream are the unmasked ones; a small first reservation grows (the batch is piled once)
    p = eng.Pileup(w["idx"])
    st = eng.Stream(w["idx"], 2, 64, 2, True, pile=p)
    st.submit(w["q"], wins[0], MIN_LEN); st.next()
    st.submit_masked(w["q"], None, wins[1], MIN_LEN); st.next()
    st.submit_masked(w["q"], words, wins[2], MIN_LEN); st.next()
    st.close()
    cut = int(wins[2][0])
    mixed = bits.copy(); mixed[:cut] = 0
    same(p.counts(), want_table(w, mixed))
    p.close()
    # another match type: SLAMEM_ERR_ARG
    for kw in (dict(), dict(paf=True)):
        st = eng.Stream(w["idx"], 2, 1 << 16, per, True, **kw)
        with pytest.raises(capi.SlamemError) as e:
            st.submit_masked(w["q"], words, wins[0], MIN_LEN)
        assert e.value.code == capi.SLAMEM_ERR_ARG and "match type 8" in str(e.value)
        st.close()


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 4097])
def test_pack_lowq_on_the_device(eng, total):
    import torch
    from slamem_amd import capi
    rng = np.random.default_rng(total + 1)
    quals = rng.integers(0, 256, size=total, dtype=np.uint8)
    for min_bq, phred in ((0, 33), (1, 33), (20, 33), (93, 33), (20, 64), (93, 0)):
        want = lowq_spec.pack(quals, min_bq, phred)
        assert np.array_equal(eng.pack_lowq(quals, min_bq, phred), want)
        got = eng.pack_lowq(quals, min_bq, phred, device=True)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy().view(np.uint64), want)
    # between guards: exactly (total + 63) / 64 words are written
    qd = prims.Guarded.of(quals) if total else prims.Guarded(0)
    out = prims.Guarded(8 * ((total + 63) // 64))
    L = capi.lib()
    assert L.slamem_pack_lowq_device(qd.ptr, total, 20, 33, out.ptr, None) == capi.SLAMEM_OK
    torch.cuda.synchronize()
    assert out.guards_intact() and qd.guards_intact() and np.array_equal(out.payload(np.uint64), lowq_spec.pack(quals, 20))
    assert L.slamem_pack_lowq_device(qd.ptr, total, 94, 33, out.ptr, None) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pack_lowq_device(qd.ptr, total, 20, 127, out.ptr, None) == capi.SLAMEM_ERR_ARG
    with pytest.raises(capi.SlamemError):
        eng.pack_lowq(quals, 94)


# ---- the executable ------------------------------------------------------------------------------------------------------------

def test_cli_bq_on_a_fastq_file(eng, world, tmp_path):
    """slaMEM-hip -b -l 14 -pile -bq 20 ref.fa reads.fq: byte for byte the file of the spec's masked table; with -bq 0, and with the
    same reads as FASTA (with and without -bq 20), the file of the plain table."""
    import hostlib
    w = world
    rng = np.random.default_rng(8)
    nq = len(w["off"]) - 1
    quals = rng.integers(33 + 20, 33 + 42, size=w["total"], dtype=np.uint8)
    low = rng.random(w["total"]) < 0.1
    for r in range(nq):  # the Illumina shape as well: the last letters of every read
        low[max(int(w["off"][r]), int(w["off"][r + 1]) - 3):int(w["off"][r + 1])] = True
    quals[low] = rng.integers(33, 33 + 20, size=int(low.sum()), dtype=np.uint8)
    reads = [(b"read%d x" % r, bytes(w["q"][int(w["off"][r]):int(w["off"][r + 1])]), bytes(quals[int(w["off"][r]):int(w["off"][r + 1])]))
             for r in range(nq)]
    ref_fa, q_fq, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), str(tmp_path / "reads.fa")
    open(ref_fa, "wb").write(b">chr one\n" + bytes(w["ref"]) + b"\n")
    open(q_fq, "wb").write(lowq_spec.write_fastq(reads))
    open(q_fa, "wb").write(b"".join(b">" + n + b"\n" + l + b"\n" for n, l, _ in reads))
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(w["ref"])
    assert np.array_equal(lowq_spec.pack(quals, 20), lowq_spec.from_bits(low))
    masked = pile_spec.pile_file(want_table(w, low), loaded)
    plain = pile_spec.pile_file(want_table(w, None), loaded)
    assert masked != plain and masked.count(b"\n") > 2000
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")

    def run(*args):
        out = str(tmp_path / "out.txt")
        r = subprocess.run([EXE, "-b", "-l", str(MIN_LEN), "-pile", "-o", out] + list(args), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        return open(out, "rb").read(), r
    got, r = run("-bq", "20", ref_fa, q_fq)
    assert got == masked and b"; minimum mapping quality = 0 ; minimum base quality = 20\n" in r.stdout and b"-bq" not in r.stderr
    got, r = run("-bq", "0", ref_fa, q_fq)
    assert got == plain and b"; minimum base quality = 0\n" in r.stdout
    got, r = run(ref_fa, q_fa)
    assert got == plain and b"base quality" not in r.stdout
    got, r = run("-bq", "20", ref_fa, q_fa)
    assert got == plain and r.stderr.count(b"option -bq 20 has no effect on FASTA queries") == 1
    # the loader thread beside the search, pieces of the smallest size, two logical GPUs
    env.update(SLAMEM_OVERLAP_MB="0", SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1")
    got2, r = run("-bq", "20", ref_fa, q_fq)
    assert got2 == masked
