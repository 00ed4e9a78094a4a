"""A stream's slots as their buffers grow (stream.hip), in the modes whose buffers `test_stream_slots_grow_with_the_
batches` does not reach: the -ext column, the -aln segments and operations, -paf's read records and the MD arrays, -pile's
low-quality mask, the packed planes.  A stream of 3 slots reserved for 4 records of 1 kB takes batches of 3, 0, 7, 50, 240, 600 and
300 reads one after the other, so that every slot is used again at another size.  The last batch is cut from a region of the text
that is one 13-letter unit forty times over: a read has some thirty MEMs there, the batch's -mem list is several times the first
guess of a slot's room (letters / 32 + strand blocks + 1024), and the download stage has to run it again with more room.  Every
batch is compared, array for array, with the one-shot device call of its mode on the same window (Index.find_exts, find_alns,
map_reads, Pileup.add, find_mems), which their own tests hold to the specs."""
import numpy as np
import pytest

from test_gpu_parity import make_queries, pack, rand_text

pytestmark = pytest.mark.gpu

MIN_LEN = 12
BOUNDS = [0, 3, 3, 10, 60, 300, 900, 1200]  # (an empty batch: 3..3)
DENSE = len(BOUNDS) - 2                     # the batch cut from the repeat: behind the sparse ones, so that the densest batch
                                            # seen (which sizes a slot's first room) is a sparse one when it comes
DENSE_FACTOR = 2.0                          # its -mem rows against the first guess of the room
UNIT, COPIES, REGION = 13, 40, 40_000


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (there is no CPU path)")
    from slamem_amd import engine
    return engine


def make_world(rng):
    """(text, reads, offsets): 80 kbp with a repeat of UNIT x COPIES letters at REGION, 1200 reads of 1 .. 200 letters with empty
    records among them; the last 300 are 100-letter windows of the repeat, every second one with a few substitutions."""
    t = np.frombuffer(rand_text(rng, 80_000, "ACGT", 30, max_rep=400), dtype=np.uint8).copy()
    t[REGION:REGION + UNIT * COPIES] = np.tile(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=UNIT), COPIES)
    text = t.tobytes()
    qs = make_queries(rng, text, BOUNDS[DENSE], "ACGT", maxlen=200)
    for k in (1, 5, 650):
        qs[k] = b""
    for k in range(BOUNDS[DENSE + 1] - BOUNDS[DENSE]):
        a = REGION + int(rng.integers(0, UNIT * COPIES - 100 + 1))
        r = t[a:a + 100].copy()
        if k % 2:
            mut = rng.random(100) < 0.02
            r[mut] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(mut.sum()))
        qs.append(r.tobytes())
    q, off = pack(qs)
    return text, np.array(q), off


@pytest.fixture(scope="module")
def world(eng):
    text, q, off = make_world(np.random.default_rng(909))
    idx = eng.Index.build(text)
    w = off[BOUNDS[DENSE]: BOUNDS[DENSE + 1] + 1]
    rows, _ = idx.find_mems(q[int(w[0]): int(w[-1])], w - w[0], MIN_LEN, True)
    yield {"idx": idx, "q": q, "off": off, "dense_rows": len(rows)}
    idx.close()


def windows(w):
    """Per batch: its number, the window of the offsets (into the one array of letters), and letters and offsets as a one-shot
    call takes them (from 0)."""
    for b in range(len(BOUNDS) - 1):
        o = w["off"][BOUNDS[b]: BOUNDS[b + 1] + 1]
        yield b, o, w["q"][int(o[0]): int(o[-1])], o - o[0]


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def stream_of(eng, w, **mode):
    return eng.Stream(w["idx"], 3, 1024, 4, True, **mode)


def test_the_dense_batch_is_far_above_a_slots_first_room(world):
    """What makes the cases below run the download stage's capacity retry: the last batch's -mem list against the first guess
    for a slot that holds it.  The oracle counts 18,747 rows on the CPU for these 300 reads of 30,000 letters; the guess is 2,561,
    and the densest batch in front of it has 0.041 rows a letter, which sizes a slot for 2,580."""
    o = world["off"][BOUNDS[DENSE]: BOUNDS[DENSE + 1] + 1]
    chars, blocks = int(o[-1] - o[0]), 2 * (len(o) - 1)
    guess = chars // 32 + blocks + 1024
    print(f"dense batch: {world['dense_rows']} -mem rows, first guess {guess}")
    assert world["dense_rows"] >= DENSE_FACTOR * guess, "input no longer dense"


def test_ext_rows_and_mismatches(eng, world):
    st = stream_of(eng, world, ext=True)
    for b, o, sub, rel in windows(world):
        st.submit(world["q"], o, MIN_LEN)
        rows, boff, _ = st.next()
        mm = st.mismatches()
        want = world["idx"].find_exts(sub, rel, MIN_LEN, True)
        for k, got in enumerate((rows, boff, mm)):
            same(got, want[k], (b, k))
    st.close()


def test_aln_segments_and_operations(eng, world):
    st = stream_of(eng, world, aln=True)
    for b, o, sub, rel in windows(world):
        st.submit(world["q"], o, MIN_LEN)
        segs, boff, _ = st.next()
        want = world["idx"].find_alns(sub, rel, MIN_LEN, True)
        for k, got in enumerate((segs, boff) + st.alns()):
            same(got, want[k], (b, k))
    st.close()


def test_paf_reads_and_md(eng, world):
    st = stream_of(eng, world, paf=True, md=True)
    for b, o, sub, rel in windows(world):
        st.submit(world["q"], o, MIN_LEN)
        segs, roff, _ = st.next()
        want = world["idx"].map_reads(sub, rel, MIN_LEN, True, md=True)
        assert len(want) == 9
        for k, got in enumerate((segs, roff) + st.alns() + (st.maps(),) + st.mds()):
            same(got, want[k], (b, k))
    st.close()


def test_pile_with_a_mask_on_every_second_batch(eng, world):
    rng = np.random.default_rng(910)
    q = world["q"]
    bits = (rng.random(len(q)) < 0.3).astype(np.uint8)

    def words(x):
        return np.packbits(np.concatenate([x, np.zeros(-len(x) % 64, dtype=np.uint8)]), bitorder="little").view(np.uint64).copy()

    mask = words(bits)
    got, want = eng.Pileup(world["idx"]), eng.Pileup(world["idx"])
    st = stream_of(eng, world, pile=got)
    for b, o, sub, rel in windows(world):
        if b % 2:
            st.submit_masked(q, mask, o, MIN_LEN)
        else:
            st.submit(q, o, MIN_LEN)
        st.next()
        recs = want.add(sub, rel, MIN_LEN, True, lowq=words(bits[int(o[0]): int(o[-1])]) if b % 2 else None)
        same(st.maps(), recs, b)
    st.close()
    same(got.counts(), want.counts(), "table")
    assert got.counts().any()
    got.close()
    want.close()


def test_packed_planes(eng, world):
    st = stream_of(eng, world)
    keep = []
    for b, o, sub, rel in windows(world):
        units = int(((np.diff(o) + 63) // 64).sum())
        pl = eng.PinnedBuffer(units * 16 + 64)
        keep.append(pl)
        assert eng.pack_reads(world["q"], o, pl.array, None, threads=2) == units  # (no letter but A, C, G, T)
        st.submit_packed(pl.array, None, o, MIN_LEN, units=units if b % 2 else 0)
        rows, boff, _ = st.next()
        want = world["idx"].find_mems(sub, rel, MIN_LEN, True)
        same(rows, want[0], (b, "rows"))
        same(boff, want[1], (b, "offsets"))
    st.close()
    for pl in keep:
        pl.close()


def test_an_empty_first_batch_gives_empty_arrays(eng, world):
    """A slot's first batch has no read: total 0, and every getter still hands out memory an empty array can be formed on."""
    from slamem_amd.engine import ALN_DTYPE, MAP_DTYPE
    none = world["off"][:1]
    for mode in (dict(aln=True), dict(paf=True, md=True)):
        st = stream_of(eng, world, **mode)
        st.submit(world["q"], none, MIN_LEN)
        segs, boff, _ = st.next()
        assert segs.dtype == ALN_DTYPE and len(segs) == 0
        same(boff, np.zeros(1, dtype=np.uint64), "offsets")
        ops, ooff = st.alns()
        same(ops, np.zeros(0, dtype=np.uint32), "ops")
        same(ooff, np.zeros(1, dtype=np.uint64), "op offsets")
        if "paf" in mode:
            assert st.maps().dtype == MAP_DTYPE and len(st.maps()) == 0
            md, moff, seg_eq, primary = st.mds()
            same(md, np.zeros(0, dtype=np.uint32), "md")
            same(moff, np.zeros(1, dtype=np.uint64), "md offsets")
            same(seg_eq, np.zeros(0, dtype=np.uint32), "seg_eq")
            same(primary, np.zeros(0, dtype=np.uint32), "primary")
        st.close()
