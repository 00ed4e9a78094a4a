"""Python view of the MEM engine: thin wrappers over the C ABI (include/slamem_hip.h).

torch is used for what the task calls plumbing only: device memory (tensors own the HBM buffers handed
to the C ABI as raw pointers), streams and torch.distributed.  All compute happens in libslamem_hip.so.

Method names mirror the reference's own interface for this path (bwtindex.h / lcparray.h as used by
GetMatches, slamem.c:37-218), in batched form.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import capi

MEM_DTYPE = np.dtype([("ref_pos", "<u4"), ("query_pos", "<u4"), ("length", "<u4")])
ALN_DTYPE = np.dtype([("ref_pos", "<u4"), ("query_pos", "<u4"), ("ref_len", "<u4"), ("query_len", "<u4"), ("edits", "<u4")])
MAP_DTYPE = np.dtype([("strand", "u1"), ("mapq", "u1"), ("s1", "<u4"), ("s2", "<u4")])  # strand: 0 unmapped, 1 forward, 2 reverse
_MAP_ABI = np.dtype([("s1", "<u4"), ("s2", "<u4"), ("strand", "u1"), ("mapq", "u1"), ("reserved", "u1", (2,))])  # slamem_map
EDITS_DEFAULT = 0xFFFFFFFF  # SLAMEM_ALN_EDITS_DEFAULT: "the default 31" in the C ABI (0 is a value of its own)
CIGAR_OPS = {7: "=", 8: "X", 1: "I", 2: "D"}  # BAM's codes; an operation is length << 4 | code
SITES_NONZERO, SITES_VARIANT = 0, 1  # the rules of Pileup.sites (SLAMEM_SITES_*)
# slamem_event: kind 0 a deletion of len rows from pos, 1 an insertion of len letters in front of pos
EVENT_DTYPE = np.dtype([("pos", "<u8"), ("letters", "<u8"), ("fwd", "<u4"), ("rev", "<u4"), ("kind", "u1"), ("len", "u1"), ("pad", "u1", (6,))])
SAM_LANE_OPS = 32  # -sam: the MD entries of a segment of up to this many operations are written by one lane, of a longer one by a wave (sam_filter.hip)
MD_CLOSE = 8  # the closing entry of a segment: m << 4 | 8
PILE_LANE_OPS = 32  # -pile: a segment of up to this many operations is walked by one lane, a longer one by a wave (pile_filter.hip)
# slamem_junction: kind 0 a deletion of len rows from pos, 1 an insertion of len letters in front of pos
JUNCTION_DTYPE = np.dtype([("pos", "<u8"), ("len", "<u4"), ("fwd", "<u4"), ("rev", "<u4"), ("kind", "u1"), ("pad", "u1", (3,))])
# slamem_genotype: a <= b letter columns (SNV) or allele numbers 0 / 1 (event); scores in milli-Phred
GENOTYPE_DTYPE = np.dtype([("qual", "<u4"), ("gq", "<u4"), ("a", "u1"), ("b", "u1"), ("ploidy", "u1"), ("ref", "u1"), ("pl", "<u4", (10,)),
                           ("pad", "u1", (4,))])


def gt_costs(q: int) -> tuple[int, int, int]:
    """(M, H, E): what one observed letter costs a genotype that is homozygous for it, heterozygous with it, or does not hold it,
    in milli-Phred, at a constant error rate of Phred q (1 to 93).  Host arithmetic, the same operations in the
    same order as slamem_gt_costs; q = 20 gives (44, 3039, 24771)."""
    import math
    q = int(q)
    if not 1 <= q <= 93:
        raise ValueError("the error rate is 1 to 93 Phred")
    e = math.pow(10.0, -float(q) / 10.0)
    hom = 1.0 - e
    het = hom / 2.0 + e / 6.0
    third = e / 3.0
    return tuple(int(math.floor(-10000.0 * math.log10(x) + 0.5)) for x in (hom, het, third))


WQ_COSTS = (0, 3010, 4771)  # -wq: M, H = round(10000 log10 2), E = round(10000 log10 3); a letter's own quality comes on top of E


def fisher_strand(t) -> float:
    """slamem_fisher_strand: FS of -sb, the Phred-scaled two-sided Fisher exact test of the strand table
    t = (reference forward, reference reverse, alternative forward, alternative reverse), four counts below 2^32.  Host
    arithmetic in doubles; tables of a sum above 400 are scaled to 200 first (fisher_strand_table shows the scaled table).
    (10, 10, 10, 10) gives 0.0 and the VCF prints the value with three decimals."""
    return float(capi.lib().slamem_fisher_strand(_strand_table(t)))


def fisher_strand_table(t) -> tuple[int, int, int, int]:
    """The table fisher_strand tests: t itself up to a sum of 400, else every cell * 200 // sum."""
    out = (C.c_uint32 * 4)()
    capi.lib().slamem_fisher_strand_table(_strand_table(t), out)
    return tuple(int(v) for v in out)


def _strand_table(t):
    t = [int(v) for v in t]
    if len(t) != 4 or not all(0 <= v < 2 ** 32 for v in t):
        raise ValueError("a strand table is four counts below 2^32")
    return (C.c_uint32 * 4)(*t)


def _gt_params(ploidy, err_q, het_q, min_depth, min_qual, costs=None) -> capi.GtParams:
    M, H, E = gt_costs(err_q) if costs is None else (int(v) for v in costs)
    if not 0 <= int(het_q) <= 999:
        raise ValueError("het_q is 0 to 999 Phred")
    vals = (int(ploidy), M, H, E, 1000 * int(het_q), int(min_depth), int(min_qual))
    if not all(0 <= v < 2 ** 32 for v in vals):
        raise ValueError("the genotype parameters are unsigned 32-bit numbers")
    return capi.GtParams(*vals)


def _map_records(raw: np.ndarray) -> np.ndarray:
    """slamem_map records (bytes) -> MAP_DTYPE"""
    a = raw.view(_MAP_ABI).reshape(-1)
    out = np.zeros(a.shape[0], dtype=MAP_DTYPE)
    for k in ("strand", "mapq", "s1", "s2"):
        out[k] = a[k]
    return out


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def _stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_gpu(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("slamem_amd runs on an MI355X only (device must be cuda:N); there is no CPU path")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: slamem_amd has no CPU fallback")
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


class Index:
    """FM-index + parent-interval structure resident in HBM.

    ``Index.build`` replaces ``FMI_BuildIndex`` + ``BuildSampledLCPArray`` (slamem.c:73-74);
    ``close`` replaces ``FMI_FreeIndex`` + ``FreeSampledSuffixArray`` (slamem.c:208-209).
    """

    def __init__(self, handle: int, device: torch.device, keepalive=None):
        self._h = C.c_void_p(handle)
        self.device = device
        self._keepalive = keepalive  # arena tensor when attached
        info = capi.IndexInfo()
        capi.check(capi.lib().slamem_index_get_info(self._h, C.byref(info)))
        self.info = info
        self.n = int(info.text_length)

    # ---- construction -------------------------------------------------------------------------
    @classmethod
    def build(cls, text, device="cuda:0", layout: int = capi.LAYOUT_AUTO) -> "Index":
        """text: bytes / numpy uint8 / torch uint8 tensor (host or device) of A,C,G,T,N.  layout: capi.LAYOUT_AUTO (full
        when its build peak fits the free HBM, else compact), LAYOUT_FULL or LAYOUT_COMPACT (include/slamem_hip.h)."""
        dev = _require_gpu(device)
        L = capi.lib()
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        if isinstance(text, np.ndarray):
            text = torch.from_numpy(np.array(text, dtype=np.uint8, copy=True))
        if text.device != dev:
            text = text.to(dev)
        text = text.contiguous()
        n = text.numel()
        h = C.c_void_p()
        with torch.cuda.device(dev):
            stream = _stream_handle(dev)
            capi.check(L.slamem_index_build_device_layout(_ptr(text), n, dev.index, stream, int(layout), C.byref(h)))
        return cls(h.value, dev)

    @classmethod
    def attach(cls, arena: torch.Tensor) -> "Index":
        """Borrow an arena that was broadcast from a peer GPU (uint8 tensor on this device)."""
        dev = _require_gpu(arena.device)
        h = C.c_void_p()
        capi.check(capi.lib().slamem_index_attach(_ptr(arena), arena.numel(), dev.index, C.byref(h)))
        return cls(h.value, dev, keepalive=arena)

    @classmethod
    def load(cls, path: str, device="cuda:0") -> "Index":
        dev = _require_gpu(device)
        h = C.c_void_p()
        capi.check(capi.lib().slamem_index_load(path.encode(), dev.index, C.byref(h)))
        return cls(h.value, dev)

    def save(self, path: str) -> None:
        capi.check(capi.lib().slamem_index_save(self._h, path.encode()))

    def export_arena(self) -> torch.Tensor:
        """A torch-owned copy of the arena (what rank 0 hands to torch.distributed.broadcast)."""
        out = torch.empty(int(self.info.arena_bytes), dtype=torch.uint8, device=self.device)
        capi.check(capi.lib().slamem_index_export(self._h, _ptr(out), out.numel(), _stream_handle(self.device)))
        return out

    def arena_view(self) -> torch.Tensor:
        """Zero-copy uint8 tensor over the index arena (slamem_index_arena): what rank 0 hands to the broadcast, so the
        index is never held twice.  Valid while this Index is alive."""
        ptr, nbytes = C.c_void_p(), C.c_uint64()
        capi.check(capi.lib().slamem_index_arena(self._h, C.byref(ptr), C.byref(nbytes)))

        class _Arena:  # the CUDA array interface torch.as_tensor understands (HIP pointers on ROCm builds)
            __cuda_array_interface__ = {"shape": (int(nbytes.value),), "typestr": "|u1", "data": (int(ptr.value), False),
                                        "version": 2, "strides": None}
        holder = _Arena()
        t = torch.as_tensor(holder, device=self.device)
        assert t.data_ptr() == ptr.value and t.numel() == nbytes.value, "arena view must alias the arena"
        t._slamem_keepalive = (holder, self)
        return t

    def close(self) -> None:
        h, self._h = self._h, None
        if h:
            capi.lib().slamem_index_free(h)
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- FMI_GetBWTSize (bwtindex.c:263) ---------------------------------------------------------
    def bwt_size(self) -> int:
        return self.n + 1

    # ---- structure-level parity -----------------------------------------------------------------------
    def download(self, which: int) -> np.ndarray:
        n = self.n
        shape, dt = {capi.ARRAY_SA: (n + 1, np.uint32), capi.ARRAY_BWT: (n + 1, np.uint8),
                     capi.ARRAY_LCP: (n + 2, np.int32), capi.ARRAY_PSV: (n + 2, np.uint32),
                     capi.ARRAY_NSV: (n + 2, np.uint32)}[which]
        out = np.empty(shape, dtype=dt)
        capi.check(capi.lib().slamem_index_download(self._h, which, out.ctypes.data, shape))
        return out

    def sampled_lcp_stats(self) -> dict:
        """What BuildSampledLCPArray would report for this text (lcparray.c:709-711, 999-1000)."""
        st = capi.SslcpStats()
        capi.check(capi.lib().slamem_index_sampled_lcp_stats(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in capi.SslcpStats._fields_ if k != "pad"}

    # ---- fine-grained operations, batched ------------------------------------------------------------
    def follow_letter(self, letters: bytes, top, bottom):
        """FMI_FollowLetter (bwtindex.c:359) for arrays of (letter, top, bottom) -> (size, top, bottom)."""
        dev = self.device
        cnt = len(letters)
        lt = torch.from_numpy(np.frombuffer(bytes(letters), dtype=np.uint8).copy()).to(dev)
        t = torch.as_tensor(np.asarray(top, dtype=np.uint32).view(np.int32)).to(dev)
        b = torch.as_tensor(np.asarray(bottom, dtype=np.uint32).view(np.int32)).to(dev)
        s = torch.zeros(cnt, dtype=torch.int32, device=dev)
        capi.check(capi.lib().slamem_follow_letter_batch(self._h, _ptr(lt), _ptr(t), _ptr(b), _ptr(s), cnt,
                                                         _stream_handle(dev)))
        torch.cuda.synchronize(dev)
        f = lambda x: x.cpu().numpy().view(np.uint32)
        return f(s), f(t), f(b)

    def enclosing_interval(self, top, bottom):
        """GetEnclosingLCPInterval (lcparray.c:330) -> (depth, top, bottom)."""
        dev = self.device
        t = torch.as_tensor(np.asarray(top, dtype=np.uint32).view(np.int32)).to(dev)
        b = torch.as_tensor(np.asarray(bottom, dtype=np.uint32).view(np.int32)).to(dev)
        d = torch.zeros(t.numel(), dtype=torch.int32, device=dev)
        capi.check(capi.lib().slamem_enclosing_interval_batch(self._h, _ptr(t), _ptr(b), _ptr(d), t.numel(),
                                                              _stream_handle(dev)))
        torch.cuda.synchronize(dev)
        return d.cpu().numpy(), t.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)

    def position_in_text(self, rows):
        """FMI_PositionInText (bwtindex.c:402)."""
        dev = self.device
        r = torch.as_tensor(np.asarray(rows, dtype=np.uint32).view(np.int32)).to(dev)
        o = torch.zeros(r.numel(), dtype=torch.int32, device=dev)
        capi.check(capi.lib().slamem_position_in_text_batch(self._h, _ptr(r), _ptr(o), r.numel(), _stream_handle(dev)))
        torch.cuda.synchronize(dev)
        return o.cpu().numpy().view(np.uint32)

    def char_at_bwt_pos(self, rows) -> bytes:
        """FMI_GetCharAtBWTPos (bwtindex.c:304)."""
        dev = self.device
        r = torch.as_tensor(np.asarray(rows, dtype=np.uint32).view(np.int32)).to(dev)
        o = torch.zeros(r.numel(), dtype=torch.uint8, device=dev)
        capi.check(capi.lib().slamem_char_at_bwt_pos_batch(self._h, _ptr(r), _ptr(o), r.numel(), _stream_handle(dev)))
        torch.cuda.synchronize(dev)
        return o.cpu().numpy().tobytes()

    # ---- GetMatches (slamem.c:90-207) for a batch ---------------------------------------------------------
    def matcher(self, num_queries: int, both_strands: bool, mems_capacity: int, query_bytes: int,
                mam: bool = False, mum: bool = False, smem: bool = False, max_occ: int = 0, chain: bool = False,
                max_gap: int = 0, ext: bool = False, penalty: int = 0, xdrop=None) -> "Matcher":
        return Matcher(self, num_queries, both_strands, mems_capacity, query_bytes, mam, mum, smem, max_occ, chain, max_gap,
                       ext, penalty, xdrop)

    def find_mems(self, queries, offsets, min_len: int = 20, both_strands: bool = False, mam: bool = False,
                  mum: bool = False, smem: bool = False, max_occ: int = 0, chain: bool = False, max_gap: int = 0,
                  ext: bool = False, penalty: int = 0, xdrop=None):
        """Convenience: host arrays in, (mems structured array, block_offsets) out.  mam=True: -mam mode
        (slamem_find_mams_device; slamem.c:131,657).  mum=True: -mum mode, the MEMs no other MEM of their strand
        block contains in either coordinate (slamem_find_mums_device).  smem=True: -smem mode, the MEMs whose query
        interval no other MEM of their strand block strictly contains; max_occ > 0 also drops the intervals that more than
        max_occ MEMs of the block share (slamem_find_smems_device).  chain=True: -chain mode, the MEMs of each strand
        block's best collinear chain; max_gap: the maximum gap, 0 for the default 5000 (slamem_find_chains_device;
        find_chains also returns the scores).  ext=True: -ext mode, every MEM extended through mismatches on its diagonal;
        penalty: the mismatch penalty, 0 for the default 4; xdrop: the drop, None for the default 20
        (slamem_find_exts_device; find_exts also returns the mismatches)."""
        mems, boff, _ = self._find(queries, offsets, min_len, both_strands, mam, mum, smem, max_occ, chain, max_gap, ext, penalty,
                                   xdrop)
        return mems, boff

    def find_chains(self, queries, offsets, min_len: int = 20, both_strands: bool = False, max_gap: int = 0):
        """-chain mode: (mems, block_offsets, scores) -- the MEMs of each strand block's best collinear chain in the -mem
        order, and a uint32 score per strand block (0 for an empty block).  DESIGN.md 4.12 has the definition."""
        return self._find(queries, offsets, min_len, both_strands, False, False, False, 0, True, max_gap)

    def find_exts(self, queries, offsets, min_len: int = 20, both_strands: bool = False, penalty: int = 0, xdrop=None):
        """-ext mode: (rows, block_offsets, mismatches) -- every MEM of a strand block extended on its diagonal by the X-drop
        rule of DESIGN.md 4.13 (a match +1, a mismatch -penalty, default 4; drop xdrop, default 20), rows that extend to the
        same segment once, and a uint32 of mismatches per row."""
        return self._find(queries, offsets, min_len, both_strands, False, False, False, 0, False, 0, True, penalty, xdrop)

    def find_alns(self, queries, offsets, min_len: int = 20, both_strands: bool = False, max_gap: int = 0, penalty: int = 0,
                  xdrop=None, max_edits=None, capacities=None, gap_costs=None, end_band: int = 0):
        """-aln mode: (segments, block_offsets, ops, op_offsets) -- per strand block the gapped alignment built on its best
        chain.  segments: a structured array (ref_pos, query_pos, ref_len, query_len, edits), the segments
        of a block with the query start descending; block_offsets: per strand block; ops: uint32 CIGAR operations, length << 4
        | code with BAM's codes (CIGAR_OPS), left to right in the scanned strand; op_offsets: per segment.  max_gap, penalty
        and xdrop as for find_chains and find_exts; max_edits: the most edits in one gap (None: 31; at most 127).
        gap_costs=(x, o, e): the gaps are closed at gap-affine cost (aln_word); None: unit cost.
        end_band=Z (1 to 31, with gap_costs): each of a block's two outer ends may hold indels of at most Z letters
        of net diagonal drift -- the gapped X-drop attempt where it scores more than the ungapped side; 0: ungapped ends.
        capacities: (mems, segments, operations) to run with exactly that room (slamem.capi.SlamemError with
        SLAMEM_ERR_CAPACITY and .totals = what is needed when it is too small); None: grow until the batch fits."""
        return self._aln_like(queries, offsets, min_len, both_strands, max_gap, penalty, xdrop, aln_word(max_edits, gap_costs), capacities,
                              False, end_band=_end_band(end_band, gap_costs))

    def map_reads(self, queries, offsets, min_len: int = 20, both_strands: bool = False, max_gap: int = 0, penalty: int = 0,
                  xdrop=None, max_edits=None, capacities=None, md: bool = False, gap_costs=None, end_band: int = 0):
        """-paf mode: (segments, read_offsets, ops, op_offsets, reads) -- one mapping per read.  Per read the
        strand block whose best chain scores highest is the primary one (the forward block on a tie) and only that block is
        aligned, as find_alns aligns it; segments, ops and op_offsets are as find_alns returns them, in the coordinates of the
        scanned strand; read_offsets: the segments' offsets per READ (len(offsets) entries); reads: a structured array (strand,
        mapq, s1, s2) per read -- strand 0 unmapped, 1 forward, 2 reverse; s1 the primary chain's score, s2 the best competing
        chain's; mapq = 60 * (s1 - s2) // s1.  The other arguments as for find_alns.  md=True appends (md, md_offsets, seg_eq,
        primary), what SAM needs (slamem_maps_md_device over the batch as it lies on the device): the MD entries of
        all segments, uint32 `m << 4 | d << 2 | c` and a closing `m << 4 | 8` per segment (md_text makes the tag of one segment's),
        their offsets per segment, the letters under = per segment, and per read the index of its primary segment within the
        read's range (0xFFFFFFFF: the read has no segment)."""
        return self._aln_like(queries, offsets, min_len, both_strands, max_gap, penalty, xdrop, aln_word(max_edits, gap_costs), capacities,
                              True, md=md, end_band=_end_band(end_band, gap_costs))

    def _md_pass(self, segs, nseg, roff, num, ops, ooff, cap):
        """slamem_maps_md_device over a mapped batch as it lies on the device, with room for cap entries: (md, md_offsets, seg_eq,
        primary) as numpy arrays."""
        dev = self.device
        L = capi.lib()
        need = C.c_uint64()
        capi.check(L.slamem_maps_md_workspace_bytes(nseg, num, C.byref(need)))
        ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
        md = torch.empty(cap + 1, dtype=torch.int32, device=dev)
        moff = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
        seq = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
        prim = torch.empty(num + 1, dtype=torch.int32, device=dev)
        total = C.c_uint64()
        with torch.cuda.device(dev):
            torch.cuda.current_stream(dev).synchronize()
            capi.check(L.slamem_maps_md_device(self._h, _ptr(segs), nseg, _ptr(roff), num, _ptr(ops), _ptr(ooff), _ptr(md), cap,
                                               _ptr(moff), _ptr(seq), _ptr(prim), _ptr(ws), need.value, None, C.byref(total)))
            torch.cuda.synchronize(dev)
        n = int(total.value)
        return (md[:n].cpu().numpy().view(np.uint32), moff.cpu().numpy().view(np.uint64), seq[:nseg].cpu().numpy().view(np.uint32),
                prim[:num].cpu().numpy().view(np.uint32))

    def _aln_like(self, queries, offsets, min_len, both_strands, max_gap, penalty, xdrop, max_edits, capacities, mapping,
                  pile=None, md=False, end_band=0):
        """pile: (Pileup, min_mapq) -- the batch's mappings are added to the accumulator on the device and only the read records
        come back (Pileup.add)."""
        dev = self.device
        q = np.ascontiguousarray(np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray))
                                 else queries, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        num = offsets.shape[0] - 1
        nb = num * (2 if both_strands else 1)
        qbytes = int(offsets[-1]) if num else 0
        qd = torch.zeros((q.shape[0] + 15) // 8 * 8, dtype=torch.uint8, device=dev)
        if q.shape[0]:
            qd[: q.shape[0]] = torch.from_numpy(q if q.flags.writeable else q.copy()).to(dev)
        od = torch.from_numpy(offsets.view(np.int64)).to(dev)
        edits = EDITS_DEFAULT if max_edits is None else int(max_edits)
        cap, scap, ocap = capacities if capacities is not None else (max(1024, q.shape[0] // 8 + 4 * num), nb + 1024, 4 * nb + 4096)
        L = capi.lib()
        boff = torch.zeros((num if mapping else nb) + 1, dtype=torch.int64, device=dev)
        recs = torch.zeros((num + 1) * 12, dtype=torch.uint8, device=dev) if mapping else None
        ws_bytes = L.slamem_find_maps_workspace_bytes_gext if mapping else L.slamem_find_alns_workspace_bytes_gext
        while True:
            need = C.c_uint64()
            capi.check(ws_bytes(num, int(both_strands), qbytes, cap, ocap, edits, int(end_band), C.byref(need)))
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            segs = torch.zeros((scap + 1) * 5, dtype=torch.int32, device=dev)
            ops = torch.zeros(ocap + 1, dtype=torch.int32, device=dev)
            ooff = torch.zeros(scap + 2, dtype=torch.int64, device=dev)
            totals = (C.c_uint64 * 3)()
            with torch.cuda.device(dev):
                torch.cuda.current_stream(dev).synchronize()
                if mapping:
                    rc = L.slamem_find_maps_device_gext(self._h, _ptr(qd), _ptr(od), num, qbytes, int(min_len), int(both_strands),
                                                   int(max_gap), int(penalty), _xdrop_arg(xdrop), edits, int(end_band), cap, _ptr(segs), scap,
                                                   _ptr(boff), _ptr(ops), ocap, _ptr(ooff), _ptr(recs), _ptr(ws), need.value, None,
                                                   totals)
                else:
                    rc = L.slamem_find_alns_device_gext(self._h, _ptr(qd), _ptr(od), num, qbytes, int(min_len), int(both_strands),
                                                   int(max_gap), int(penalty), _xdrop_arg(xdrop), edits, int(end_band), cap, _ptr(segs), scap,
                                                   _ptr(boff), _ptr(ops), ocap, _ptr(ooff), _ptr(ws), need.value, None, totals)
            if rc == capi.SLAMEM_ERR_CAPACITY and capacities is None:
                cap, scap, ocap = max(cap, int(totals[0])), max(scap, int(totals[1])), max(ocap, int(totals[2]))
                continue
            if rc != capi.SLAMEM_OK:
                err = capi.SlamemError(rc, L.slamem_last_error_message().decode(errors="replace"))
                err.totals = tuple(int(t) for t in totals)
                raise err
            break
        if pile is not None:
            pile[0]._add_device(qd, od, num, segs, boff, ops, ooff, recs, pile[1], pile[2] if len(pile) > 2 else None,
                                bool(len(pile) > 3 and pile[3]), pile[4] if len(pile) > 4 else None)
            return _map_records(recs[: num * 12].cpu().numpy())
        nseg, nops = int(totals[1]), int(totals[2])
        extra = ()
        if md:
            edits = int(segs[: nseg * 5].view(-1, 5)[:, 4].to(torch.int64).sum().item()) if nseg else 0
            extra = self._md_pass(segs, nseg, boff, num, ops, ooff, edits + nseg)
        out = segs[: nseg * 5].cpu().numpy().view(np.uint32).reshape(-1, 5).copy().view(ALN_DTYPE).reshape(-1)
        res = (out, boff.cpu().numpy().view(np.uint64), ops[:nops].cpu().numpy().view(np.uint32),
               ooff[: nseg + 1].cpu().numpy().view(np.uint64))
        return res + (_map_records(recs[: num * 12].cpu().numpy()),) + extra if mapping else res

    def _find(self, queries, offsets, min_len, both_strands, mam, mum, smem, max_occ, chain, max_gap, ext=False, penalty=0,
              xdrop=None):
        _match_type(mam, mum, smem, max_occ, chain, max_gap, ext, penalty, xdrop)
        dev = self.device
        q = np.ascontiguousarray(np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray))
                                 else queries, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        num = offsets.shape[0] - 1
        qd = torch.zeros((q.shape[0] + 15) // 8 * 8, dtype=torch.uint8, device=dev)
        if q.shape[0]:
            qd[: q.shape[0]] = torch.from_numpy(q if q.flags.writeable else q.copy()).to(dev)
        od = torch.from_numpy(offsets.view(np.int64)).to(dev)
        cap = max(1024, q.shape[0] // 8 + 4 * num)
        while True:
            m = self.matcher(num, both_strands, cap, int(offsets[-1]) if num else 0, mam, mum, smem, max_occ, chain, max_gap,
                             ext, penalty, xdrop)
            try:
                total = m.run(qd, od, min_len)
                break
            except capi.SlamemError as e:
                if e.code != capi.SLAMEM_ERR_CAPACITY:
                    raise
                cap = int(m.last_total)
        mems = m.mems[:total].cpu().numpy().view(np.uint32).reshape(-1, 3)
        out = np.empty(total, dtype=MEM_DTYPE)
        out["ref_pos"], out["query_pos"], out["length"] = mems[:, 0], mems[:, 1], mems[:, 2]
        scores = m.scores.cpu().numpy().view(np.uint32) if m.chain else None
        if m.ext:  # (the third value of -ext: a uint32 per row)
            scores = m.mismatches[:total].cpu().numpy().view(np.uint32)
        return out, m.block_offsets.cpu().numpy().view(np.uint64), scores


XDROP_DEFAULT = 0xFFFFFFFF  # SLAMEM_EXT_XDROP_DEFAULT: "the default drop" in the C ABI (0 is a drop of its own)


def aln_word(max_edits=None, gap_costs=None):
    """The max_edits word of the C ABI (SLAMEM_ALN_AFFINE).  gap_costs=None: max_edits as it is given (unit
    cost).  gap_costs=(x, o, e): the cost of a mismatch (1 to 31), of a gap opened (0 to 63) and of a gap letter (1 to 31) in the
    upper 24 bits, above max_edits (None: 31); a gap then closes when its cost is at most o + e * max_edits (at most 512)."""
    if gap_costs is None:
        return max_edits
    x, o, e = (int(v) for v in gap_costs)
    E = 31 if max_edits is None else int(max_edits)
    if not (0 <= E <= 127 and 1 <= x <= 31 and 0 <= o <= 63 and 1 <= e <= 31):
        raise ValueError("gap_costs=(x, o, e) needs 1 <= x <= 31, 0 <= o <= 63, 1 <= e <= 31, and max_edits in [0, 127]")
    if o + e * E > 512:
        raise ValueError(f"gap_costs: the bound on a gap's cost, o + e * max_edits = {o + e * E}, is above 512")
    return E | x << 8 | o << 16 | e << 24


def _end_band(end_band, gap_costs) -> int:
    """end_band= checked: 0 to 31, and a band other than 0 needs gap_costs."""
    z = int(end_band)
    if not 0 <= z <= 31:
        raise ValueError("end_band must be in [0, 31]")
    if z and gap_costs is None:
        raise ValueError("end_band is the band of the gapped outer ends: it needs gap_costs=(x, o, e)")
    return z


def _xdrop_arg(xdrop) -> int:
    return XDROP_DEFAULT if xdrop is None else int(xdrop)


def _match_type(mam: bool, mum: bool, smem: bool = False, max_occ: int = 0, chain: bool = False, max_gap: int = 0,
                ext: bool = False, penalty: int = 0, xdrop=None) -> int:
    """The C ABI's match type: 0 -mem, 1 -mam, 2 -mum, 3 -smem, 4 -chain, 5 -ext.  The reference has one matchType
    (slamem.c:35): not two.  max_occ (the occurrence cap, 0: none) only with smem; max_gap (the maximum gap, 0: the default) only
    with chain; penalty (0: the default) and xdrop (None: the default) only with ext."""
    if ext and (mam or mum or smem or chain):
        raise ValueError("ext excludes mam, mum, smem and chain: one match type per search")
    if ext and (max_occ or max_gap):
        raise ValueError("max_occ and max_gap belong to smem and chain: not with ext")
    if (penalty or xdrop is not None) and not ext:
        raise ValueError("penalty and xdrop are the parameters of ext: they need ext=True")
    if not 0 <= int(penalty) < 2 ** 32:
        raise ValueError("penalty must be in [0, 2^32) (0: the default)")
    if xdrop is not None and not 0 <= int(xdrop) < 2 ** 32 - 1:
        raise ValueError("xdrop must be in [0, 2^32 - 1) (None: the default)")
    if ext:
        return 5
    if int(bool(mam)) + int(bool(mum)) + int(bool(smem)) > 1:
        raise ValueError("mam, mum and smem exclude each other: one match type per search")
    if chain and (mam or mum or smem):
        raise ValueError("chain excludes mam, mum and smem: one match type per search")
    if max_occ and chain:
        raise ValueError("max_occ is the occurrence cap of smem: not with chain")
    if max_gap and not chain:
        raise ValueError("max_gap is the maximum gap of chain: it needs chain=True")
    if not 0 <= int(max_gap) < 2 ** 31:
        raise ValueError("max_gap must be in [0, 2^31)")
    if max_occ and not smem:
        raise ValueError("max_occ is the occurrence cap of smem: it needs smem=True")
    if not 0 <= int(max_occ) < 2 ** 32:
        raise ValueError("max_occ must be in [0, 2^32)")
    return 4 if chain else (3 if smem else (2 if mum else (1 if mam else 0)))


class Pileup:
    """slamem_pileup_*: the per-base pileup of the read mappings, accumulated on the GPU (-pile).  A table of
    index.n rows of six uint32 counters A, C, G, T, D, I: per reference position the letters the mapped reads show there, how many
    delete it, and how many insert in front of it.  It is the sum over every batch added since creation or the last reset(),
    whatever the split into batches and their order.  28 bytes of HBM per text letter.  events=True: every add also records the
    reads' insertions and deletions as left-normalised events in a hash table of event_slots slots (a power of two of at least
    64; 0: the default) -- see events().  dedup=True: the accumulator gets the duplicate filter of DESIGN.md 4.23, a table of
    dedup_slots slots (a power of two of at least 64; 0: the default), and add(..., dedup=True) piles one read per (strand,
    unclipped 5' position): the first in the order of the adds, then of the batch.  With it the table depends on the order of the
    adds: addition no longer commutes across them.  strands=True (-sb): the accumulator owns a second one, `forward`,
    which receives exactly what the reads of strand 1 contribute, in the same kernels; 28 more bytes per text letter.  The reverse
    strand's rows are counts() - forward.counts().  quals=True (-wq): the accumulator owns a second one, `quality`,
    whose A C G T columns hold the sum of the base qualities of the letters that the same columns of counts() count; every add
    then needs quals=, and genotypes(weighted=True) scores each letter by its own quality; 28 more bytes per text letter.
    junctions=True (-sv): every add also records the long deletions and insertions between two segments of one read
    in a hash table of junction_slots slots (a power of two of at least 64; 0: the default), a split between the two segments
    having at most junction_max_mis (0 to 64) mismatches -- see junctions()."""

    def __init__(self, index: Index, events: bool = False, event_slots: int = 0, dedup: bool = False, dedup_slots: int = 0,
                 strands: bool = False, quals: bool = False, junctions: bool = False, junction_slots: int = 0, junction_max_mis: int = 3):
        self.index = index
        self._h = C.c_void_p()
        self._owner = None  # (a forward or quality view: the Pileup that owns the handle)
        self.forward = None
        self.quality = None
        if event_slots and not events:
            raise ValueError("event_slots is the size of the event table: it needs events=True")
        if dedup_slots and not dedup:
            raise ValueError("dedup_slots is the size of the duplicate filter's table: it needs dedup=True")
        if junction_slots and not junctions:
            raise ValueError("junction_slots is the size of the junction table: it needs junctions=True")
        if not 0 <= int(junction_max_mis) <= 64:
            raise ValueError("junction_max_mis must be in [0, 64]")
        capi.check(capi.lib().slamem_pileup_create(index._h, C.byref(self._h)))
        for on, enable, slots in ((events, capi.lib().slamem_pileup_enable_events, (event_slots,)),
                                  (dedup, capi.lib().slamem_pileup_enable_dedup, (dedup_slots,)),
                                  (junctions, capi.lib().slamem_pileup_enable_junctions, (junction_slots, junction_max_mis))):
            if not on:
                continue
            rc = enable(self._h, *(int(v) for v in slots))
            if rc != capi.SLAMEM_OK:
                h, self._h = self._h, None
                try:
                    capi.check(rc)
                finally:
                    capi.lib().slamem_pileup_free(h)
        self.dedup = bool(dedup)
        self.last_add_ms = 0.0  # device time of the last add's own kernels (the mapping in front of them not counted)
        if strands:
            self.enable_strands()
        if quals:
            self.enable_quals()

    def _view(self, h) -> "Pileup":
        view = Pileup.__new__(Pileup)
        view.index, view._h, view._owner, view.forward, view.quality, view.dedup, view.last_add_ms = self.index, h, self, None, None, False, 0.0
        return view

    def enable_quals(self) -> None:
        """slamem_pileup_enable_quals: from here on `quality` is the accumulator of the quality sums, a Pileup that does not own its
        handle: counts(), rows_at() and add_counts() are the read-outs with a meaning on it; add, reset and close are its owner's.
        Only on an empty accumulator (just made, or reset); a second call changes nothing."""
        capi.check(capi.lib().slamem_pileup_enable_quals(self._h))
        if self.quality is None:
            h = C.c_void_p()
            capi.check(capi.lib().slamem_pileup_quality(self._h, C.byref(h)))
            self.quality = self._view(h)

    def enable_strands(self) -> None:
        """slamem_pileup_enable_strands: from here on `forward` is the accumulator of the strand-1 reads, a Pileup that does not
        own its handle: every read-out and add_counts work on it; add, reset and close are its owner's.  Only on an empty
        accumulator (just made, or reset); a second call changes nothing."""
        capi.check(capi.lib().slamem_pileup_enable_strands(self._h))
        if self.forward is None:
            h = C.c_void_p()
            capi.check(capi.lib().slamem_pileup_forward(self._h, C.byref(h)))
            self.forward = self._view(h)

    def add(self, queries, offsets, min_len: int = 20, both_strands: bool = False, max_gap: int = 0, penalty: int = 0,
            xdrop=None, max_edits=None, min_mapq: int = 0, lowq=None, dedup: bool = False, quals=None, phred_offset: int = 33,
            gap_costs=None, end_band: int = 0):
        """Maps the batch as Index.map_reads does and adds the mappings of the reads with mapq >= min_mapq (0 to 60) to the table,
        on the device: segments and operations are not downloaded.  Returns the read records of map_reads (MAP_DTYPE).  lowq: the
        batch's low-quality mask, a uint64 array of at least (offsets[-1] + 63) // 64 words (numpy, or a tensor on
        the index's device) in which bit offsets[r] + i belongs to letter i of read r as given -- a letter whose bit is set counts
        nowhere under = and X; pack_lowq makes it from quality bytes.  None: every letter counts.  dedup=True (an accumulator made
        with dedup=True): the batch goes through the duplicate filter and the call returns (reads, dup), dup a uint8
        per read: 0 kept or no candidate, 1 duplicate (not piled), 2 no room in the filter's table (piled).  quals (an accumulator
        made with quals=True): the batch's quality bytes, a uint8 array (numpy, or a tensor on the index's device)
        of at least offsets[-1] bytes in which byte offsets[r] + i belongs to letter i of read r as given, Phred + phred_offset; it
        works with lowq= and dedup= as they are.  gap_costs and end_band: as for Index.map_reads."""
        if not 0 <= int(min_mapq) <= 60:
            raise ValueError("min_mapq must be in [0, 60]")
        if quals is not None:
            need = int(np.asarray(offsets)[-1])
            if isinstance(quals, torch.Tensor):
                if quals.dtype != torch.uint8 or quals.device != self.index.device or not quals.is_contiguous():
                    raise ValueError("quals as a tensor: contiguous uint8 bytes on the index's device")
            else:
                quals = np.ascontiguousarray(np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals)
                if quals.dtype != np.uint8:
                    raise ValueError("quals must be a uint8 array")
            if quals.shape[0] < need:
                raise ValueError(f"quals has {quals.shape[0]} bytes, the batch's letters need {need}")
            if not 0 <= int(phred_offset) <= 255:
                raise ValueError("phred_offset must be in [0, 255]")
        if lowq is not None:
            need = (int(np.asarray(offsets)[-1]) + 63) // 64
            if isinstance(lowq, torch.Tensor):
                if lowq.dtype != torch.int64 or lowq.device != self.index.device or not lowq.is_contiguous():
                    raise ValueError("lowq as a tensor: contiguous int64 words on the index's device")
            else:
                lowq = np.ascontiguousarray(lowq)
                if lowq.dtype != np.uint64:
                    raise ValueError("lowq must be a uint64 array")
            if lowq.shape[0] < need:
                raise ValueError(f"lowq has {lowq.shape[0]} words, the batch's letters need {need}")
        recs = self.index._aln_like(queries, offsets, min_len, both_strands, max_gap, penalty, xdrop, aln_word(max_edits, gap_costs), None, True,
                                    pile=(self, int(min_mapq), lowq, bool(dedup), None if quals is None else (quals, int(phred_offset))),
                                    end_band=_end_band(end_band, gap_costs))
        return (recs, self.last_dup) if dedup else recs

    def _add_device(self, qd, od, num, segs, roff, ops, ooff, recs, min_mapq, lowq=None, dedup=False, quals=None):
        """dedup: through the duplicate filter; last_dup holds the batch's flags afterwards.  quals: (bytes, phred_offset)."""
        dev = self.index.device
        if quals is not None and not isinstance(quals[0], torch.Tensor):
            qb = torch.zeros(quals[0].shape[0] + 8, dtype=torch.uint8, device=dev)
            if quals[0].shape[0]:
                qb[:quals[0].shape[0]] = torch.from_numpy(quals[0] if quals[0].flags.writeable else quals[0].copy()).to(dev)
            quals = (qb, quals[1])
        if lowq is not None and not isinstance(lowq, torch.Tensor):
            lowq = torch.from_numpy(lowq.view(np.int64).copy()).to(dev) if lowq.shape[0] else None
        with torch.cuda.device(dev):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            if dedup:
                keep = torch.zeros((num + 1) * 12, dtype=torch.uint8, device=dev)
                dup = torch.zeros(num + 1, dtype=torch.uint8, device=dev)
            if quals is not None:
                rc = capi.lib().slamem_pileup_add_quals_device(self._h, _ptr(qd), _ptr(od), num, _ptr(segs), _ptr(roff), _ptr(ops),
                                                               _ptr(ooff), _ptr(recs), int(min_mapq), _ptr(lowq) if lowq is not None else None,
                                                               _ptr(quals[0]), quals[1], int(bool(dedup)), _ptr(keep) if dedup else None,
                                                               _ptr(dup) if dedup else None, _stream_handle(dev))
            elif dedup:
                rc = capi.lib().slamem_pileup_add_dedup_device(self._h, _ptr(qd), _ptr(od), num, _ptr(segs), _ptr(roff), _ptr(ops),
                                                               _ptr(ooff), _ptr(recs), int(min_mapq), _ptr(lowq) if lowq is not None else None,
                                                               _ptr(keep), _ptr(dup), _stream_handle(dev))
            elif lowq is not None:
                rc = capi.lib().slamem_pileup_add_masked_device(self._h, _ptr(qd), _ptr(od), num, _ptr(segs), _ptr(roff), _ptr(ops),
                                                                _ptr(ooff), _ptr(recs), int(min_mapq), _ptr(lowq), _stream_handle(dev))
            else:
                rc = capi.lib().slamem_pileup_add_device(self._h, _ptr(qd), _ptr(od), num, _ptr(segs), _ptr(roff), _ptr(ops),
                                                         _ptr(ooff), _ptr(recs), int(min_mapq), _stream_handle(dev))
            t1.record()
            capi.check(rc)
            t1.synchronize()  # (the batch's tensors go when the caller returns)
            self.last_add_ms = float(t0.elapsed_time(t1))
            if dedup:
                self.last_dup = dup[:num].cpu().numpy()

    def dedup_stats(self) -> dict:
        """slamem_pileup_dedup_stats: candidates, duplicates, no_room and kept (the slots newly claimed) of every add(dedup=True)
        since creation or the last reset(); candidates = kept + duplicates + no_room."""
        out = (C.c_uint64 * 4)()
        capi.check(capi.lib().slamem_pileup_dedup_stats(self._h, out))
        return dict(candidates=int(out[0]), duplicates=int(out[1]), no_room=int(out[2]), kept=int(out[3]))

    def counts(self, first: int = 0, count=None) -> np.ndarray:
        """Rows [first, first + count) of the table as a (count, 6) uint32 array (count None: up to the text's end).  The
        accumulator is left as it is: more batches may be added and the table read again."""
        first = int(first)
        count = self.index.n - first if count is None else int(count)
        dev = self.index.device
        out = torch.zeros((max(count, 1), 6), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            capi.check(capi.lib().slamem_pileup_counts_device(self._h, first, count, _ptr(out), _stream_handle(dev)))
            torch.cuda.current_stream(dev).synchronize()
        return out[:max(count, 0)].cpu().numpy().view(np.uint32)

    def sites(self, min_depth: int = 4, min_pct: int = 20, mode: int = SITES_VARIANT, first: int = 0, count=None, capacity=None):
        """The rows of [first, first + count) that the rule selects, compacted on the device, as (pos uint64 (m,),
        counts uint32 (m, 6), alleles uint8 (m,)) in ascending position.  SITES_VARIANT: the text's letter is one of A,C,G,T, the
        depth A+C+G+T+D is at least min_depth, and a counter other than the letter's own is > 0 and at least min_pct percent of
        the depth; bit k of alleles says which (A C G T D I).  SITES_NONZERO: any counter is not 0.  capacity: rows of room for the
        first attempt (default: one in 64 of the range, at least 4,096); when more are selected the call is made once more with
        the need it reported."""
        first = int(first)
        count = self.index.n - first if count is None else int(count)
        dev = self.index.device
        cap = max(4096, count // 64) if capacity is None else int(capacity)
        total = C.c_uint64()
        with torch.cuda.device(dev):
            for attempt in (0, 1):
                pos = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
                rows = torch.empty((max(cap, 1), 6), dtype=torch.int32, device=dev)
                alleles = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
                rc = capi.lib().slamem_pileup_sites_device(self._h, first, count, int(mode), int(min_depth), int(min_pct), cap, _ptr(pos),
                                                           _ptr(rows), _ptr(alleles), C.byref(total), _stream_handle(dev))
                if rc != capi.SLAMEM_ERR_CAPACITY or attempt:
                    break
                cap = int(total.value)
            capi.check(rc)
        m = int(total.value)
        return pos[:m].cpu().numpy().view(np.uint64), rows[:m].cpu().numpy().view(np.uint32), alleles[:m].cpu().numpy()

    def add_counts(self, table, first: int = 0) -> None:
        """Adds a table of (m, 6) counters A C G T D I -- a numpy array or a tensor on the accumulator's device, 32-bit -- to rows
        [first, first + m).  With counts() of another accumulator of the same text the read-out becomes the sum of both."""
        dev = self.index.device
        if isinstance(table, torch.Tensor):
            t = table
            if t.dtype not in (torch.int32, torch.uint32) or t.device != dev:
                raise ValueError("add_counts takes a 32-bit tensor on the accumulator's device")
        else:
            a = np.asarray(table)
            if a.dtype != np.uint32:
                raise ValueError("add_counts takes a uint32 array")
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
        if t.dim() != 2 or t.shape[1] != 6:
            raise ValueError("add_counts takes a table of shape (m, 6)")
        t = t.contiguous()
        with torch.cuda.device(dev):
            capi.check(capi.lib().slamem_pileup_add_counts_device(self._h, int(first), t.shape[0], _ptr(t), _stream_handle(dev)))
            torch.cuda.current_stream(dev).synchronize()  # (the table's tensor goes when the caller returns)

    def events(self, min_count: int = 1, first: int = 0, count=None, capacity=None):
        """(events, skipped): the indel events with first <= pos < first + count and fwd + rev >= min_count, sorted
        on the device by (pos, kind, len, letters), as a structured array of EVENT_DTYPE, and the three counters of observations
        that were not stored (insertions of more than 31 letters; no room in the table; malformed).  capacity: events of room for
        the first attempt (default 4,096); when there are more the call is made once more with the need it reported."""
        first = int(first)
        count = self.index.n - first if count is None else int(count)
        dev = self.index.device
        cap = 4096 if capacity is None else int(capacity)
        total = C.c_uint64()
        skipped = (C.c_uint64 * 3)()
        with torch.cuda.device(dev):
            for attempt in (0, 1):
                buf = torch.empty(max(cap, 1) * 32, dtype=torch.uint8, device=dev)
                rc = capi.lib().slamem_pileup_events_device(self._h, first, count, int(min_count), cap, _ptr(buf), skipped,
                                                            C.byref(total), _stream_handle(dev))
                if rc != capi.SLAMEM_ERR_CAPACITY or attempt:
                    break
                cap = int(total.value)
            capi.check(rc)
            torch.cuda.current_stream(dev).synchronize()
        m = int(total.value)
        return buf[:m * 32].cpu().numpy().view(EVENT_DTYPE).copy(), [int(v) for v in skipped]

    def add_events(self, events) -> None:
        """Adds events (a structured array of EVENT_DTYPE, in any -- not only the canonical -- form) with their fwd and rev counts:
        with events() of another accumulator of the same text the table becomes the sum of both."""
        a = np.ascontiguousarray(np.asarray(events))
        if a.dtype != EVENT_DTYPE or a.ndim != 1:
            raise ValueError("add_events takes a one-dimensional array of EVENT_DTYPE")
        dev = self.index.device
        t = torch.from_numpy(a.view(np.uint8).copy()).to(dev) if len(a) else None
        with torch.cuda.device(dev):
            capi.check(capi.lib().slamem_pileup_add_events_device(self._h, _ptr(t) if len(a) else None, len(a), _stream_handle(dev)))
            torch.cuda.current_stream(dev).synchronize()  # (the events' tensor goes when the caller returns)

    def junctions(self, min_count: int = 1, min_len: int = 1, first: int = 0, count=None, capacity=None):
        """(junctions, skipped): the junctions with first <= pos < first + count, fwd + rev >= min_count and
        len >= min_len, sorted on the device by (pos, kind, len), as a structured array of JUNCTION_DTYPE, and the four counters of
        junctions that were not stored (balanced; no room in the table; a letter that is none of A,C,G,T; too much slop or too many
        mismatches).  capacity: junctions of room for the first attempt (default 4,096); when there are more the call is made once
        more with the need it reported."""
        first = int(first)
        count = self.index.n - first if count is None else int(count)
        dev = self.index.device
        cap = 4096 if capacity is None else int(capacity)
        total = C.c_uint64()
        skipped = (C.c_uint64 * 4)()
        with torch.cuda.device(dev):
            for attempt in (0, 1):
                buf = torch.empty(max(cap, 1) * 24, dtype=torch.uint8, device=dev)
                rc = capi.lib().slamem_pileup_junctions_device(self._h, first, count, int(min_count), int(min_len), cap, _ptr(buf), skipped,
                                                               C.byref(total), _stream_handle(dev))
                if rc != capi.SLAMEM_ERR_CAPACITY or attempt:
                    break
                cap = int(total.value)
            capi.check(rc)
            torch.cuda.current_stream(dev).synchronize()
        m = int(total.value)
        return buf[:m * 24].cpu().numpy().view(JUNCTION_DTYPE).copy(), [int(v) for v in skipped]

    def add_junctions(self, junctions) -> None:
        """Adds junctions (a structured array of JUNCTION_DTYPE) with their fwd and rev counts: with junctions() of another
        accumulator of the same text the table becomes the sum of both.  A deletion is normalised; an insertion stays where it is
        given."""
        a = np.ascontiguousarray(np.asarray(junctions))
        if a.dtype != JUNCTION_DTYPE or a.ndim != 1:
            raise ValueError("add_junctions takes a one-dimensional array of JUNCTION_DTYPE")
        dev = self.index.device
        t = torch.from_numpy(a.view(np.uint8).copy()).to(dev) if len(a) else None
        with torch.cuda.device(dev):
            capi.check(capi.lib().slamem_pileup_add_junctions_device(self._h, _ptr(t) if len(a) else None, len(a), _stream_handle(dev)))
            torch.cuda.current_stream(dev).synchronize()  # (the junctions' tensor goes when the caller returns)

    def rows_at(self, positions) -> np.ndarray:
        """The rows of counts() at the listed positions as an (m, 6) uint32 array; a position at or beyond n gives zeros."""
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.uint64).reshape(-1))
        m = len(pos)
        dev = self.index.device
        out = torch.zeros((max(m, 1), 6), dtype=torch.int32, device=dev)
        if m:
            pd = torch.from_numpy(pos.view(np.int64)).to(dev)
            with torch.cuda.device(dev):
                capi.check(capi.lib().slamem_pileup_rows_at_device(self._h, _ptr(pd), m, _ptr(out), _stream_handle(dev)))
                torch.cuda.current_stream(dev).synchronize()
        return out[:m].cpu().numpy().view(np.uint32)

    def genotypes(self, ploidy: int = 2, err_q: int = 20, het_q: int = 30, min_depth: int = 4, min_qual: int = 20, first: int = 0,
                  count=None, capacity=None, weighted: bool = False, costs=None):
        """The rows of [first, first + count) whose best genotype is not the reference's, called and compacted on
        the device, as (pos uint64 (m,), counts uint32 (m, 6), gts GENOTYPE_DTYPE (m,)) in ascending position.  A row's ten
        (ploidy 1: four) genotypes are scored from its A C G T counters at a constant error rate of Phred err_q (gt_costs), with
        a prior cost of het_q Phred per non-reference allele; it is selected iff the text's letter is one of A,C,G,T, the depth
        A+C+G+T+D is at least min_depth, the best genotype differs from the reference's and its QUAL is at least min_qual Phred.
        capacity: rows of room for the first attempt (default: one in 64 of the range, at least 4,096); when more are selected
        the call is made once more with the need it reported.  costs: (M, H, E) in the place of gt_costs(err_q).
        weighted=True (an accumulator made with quals=True): a letter that a genotype does not hold costs E and
        1000 times its own quality -- E * c[i] + 1000 * quality.counts()[p][i] per column; the costs default to WQ_COSTS, err_q is
        not looked at, and the call returns (pos, counts, gts, qsums), qsums uint32 (m, 4) the A C G T columns of the quality sums."""
        first = int(first)
        count = self.index.n - first if count is None else int(count)
        dev = self.index.device
        params = _gt_params(ploidy, err_q, het_q, min_depth, min_qual, WQ_COSTS if weighted and costs is None else costs)
        cap = max(4096, count // 64) if capacity is None else int(capacity)
        total = C.c_uint64()
        with torch.cuda.device(dev):
            for attempt in (0, 1):
                pos = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
                rows = torch.empty((max(cap, 1), 6), dtype=torch.int32, device=dev)
                gts = torch.empty(max(cap, 1) * GENOTYPE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                if weighted:
                    qsums = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
                    rc = capi.lib().slamem_pileup_genotypes_weighted_device(self._h, first, count, C.byref(params), cap, _ptr(pos),
                                                                            _ptr(rows), _ptr(gts), _ptr(qsums), C.byref(total),
                                                                            _stream_handle(dev))
                else:
                    rc = capi.lib().slamem_pileup_genotypes_device(self._h, first, count, C.byref(params), cap, _ptr(pos), _ptr(rows),
                                                                   _ptr(gts), C.byref(total), _stream_handle(dev))
                if rc != capi.SLAMEM_ERR_CAPACITY or attempt:
                    break
                cap = int(total.value)
            capi.check(rc)
        m = int(total.value)
        out = (pos[:m].cpu().numpy().view(np.uint64), rows[:m].cpu().numpy().view(np.uint32),
               gts[:m * GENOTYPE_DTYPE.itemsize].cpu().numpy().view(GENOTYPE_DTYPE).copy())
        return out + (qsums[:m].cpu().numpy().view(np.uint32),) if weighted else out

    def genotype_events(self, events, anchors, ploidy: int = 2, err_q: int = 20, het_q: int = 30, min_depth: int = 4, min_qual: int = 20):
        """(gts GENOTYPE_DTYPE (m,), called uint8 (m,)): the genotype of every given event (a structured array of EVENT_DTYPE, as
        events() returns it) against everything else at its anchor row (anchors: m positions below n -- the row in front of the
        event, or the event's own row at a record's first letter), with the parameters of genotypes().  An event is called iff
        its anchor's depth is at least min_depth, its best genotype is not 0/0 and its QUAL is at least min_qual Phred.  Every
        event is genotyped on its own: two events of one anchor are not made one multi-allelic call."""
        a = np.ascontiguousarray(np.asarray(events))
        if a.dtype != EVENT_DTYPE or a.ndim != 1:
            raise ValueError("genotype_events takes a one-dimensional array of EVENT_DTYPE")
        pos = np.ascontiguousarray(np.asarray(anchors, dtype=np.uint64).reshape(-1))
        m = len(a)
        if len(pos) != m:
            raise ValueError(f"{m} events and {len(pos)} anchors")
        if m and int(pos.max()) >= self.index.n:
            raise ValueError("an anchor lies at or beyond the text's end")
        params = _gt_params(ploidy, err_q, het_q, min_depth, min_qual)
        dev = self.index.device
        gts = torch.zeros(max(m, 1) * GENOTYPE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        called = torch.zeros(max(m, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            ed = torch.from_numpy(a.view(np.uint8).copy()).to(dev) if m else None
            pd = torch.from_numpy(pos.view(np.int64)).to(dev) if m else None
            rows = torch.zeros((max(m, 1), 6), dtype=torch.int32, device=dev)
            if m:
                capi.check(capi.lib().slamem_pileup_rows_at_device(self._h, _ptr(pd), m, _ptr(rows), _stream_handle(dev)))
            capi.check(capi.lib().slamem_pileup_genotype_events_device(self._h, _ptr(ed) if m else None, _ptr(rows) if m else None, m,
                                                                       C.byref(params), _ptr(gts) if m else None,
                                                                       _ptr(called) if m else None, _stream_handle(dev)))
            torch.cuda.current_stream(dev).synchronize()
        return gts[:m * GENOTYPE_DTYPE.itemsize].cpu().numpy().view(GENOTYPE_DTYPE).copy(), called[:m].cpu().numpy()

    def consensus(self, min_depth: int = 4, first: int = 0, count=None, bounds=None, capacity=None, genotype=None):
        """The consensus sequence of rows [first, first + count), built on the device, as (bytes uint8 (total,),
        offs uint64 (m,), stats): the text with the majority alleles applied -- per row the plurality letter in upper case, the
        text's letter in lower case where the depth A+C+G+T+D is below min_depth, N where the text has none of A,C,G,T, and the
        indel events that more than half of their anchor row's depth show.  bounds: rows in [first, first + count]; offs[j] is
        the number of bytes the rows in front of bounds[j] emit.  stats: rows uncalled, rows called unlike the text, rows deleted,
        insertions emitted, letters inserted.  capacity: bytes of room for the first attempt (default: the range and a 64th, at
        least 4,096); when the consensus is longer the call is made once more with the need it reported.
        genotype: None, or a dict with any of ploidy=2, err_q=20, het_q=30, min_gq=20, weighted=False, costs=None (the one form:
        there are no keyword arguments beside it) -- the consensus by genotype likelihood.  A row is called by the
        genotype of genotypes(ploidy, err_q, het_q, weighted=, costs=): the text's letter in lower case unless the depth reaches
        min_depth, A+C+G+T > 0 and the genotype's GQ reaches min_gq Phred (0 to 999); else the best genotype in upper case, a
        heterozygous one as its IUPAC code.  An event is applied when the genotype of genotype_events(ploidy, err_q, het_q) at
        its anchor row is homozygous for it with that GQ.  weighted=True needs an accumulator made with quals=True; the rows'
        costs are then WQ_COSTS unless costs= gives (M, H, E).  stats has 8 entries: the five above (an IUPAC code counts as
        unlike the text), rows with an IUPAC code, rows left to the text for GQ alone, heterozygous events that were not applied."""
        first = int(first)
        count = self.index.n - first if count is None else int(count)
        dev = self.index.device
        b = np.zeros(0, dtype=np.uint64) if bounds is None else np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64).reshape(-1))
        m = len(b)
        cap = max(4096, count + count // 64) if capacity is None else int(capacity)
        total = C.c_uint64()
        params = None
        if genotype is not None:
            g = dict(ploidy=2, err_q=20, het_q=30, min_gq=20, weighted=False, costs=None)
            unknown = set(genotype) - set(g)
            if unknown:
                raise ValueError(f"genotype= takes ploidy, err_q, het_q, min_gq, weighted and costs, not {sorted(unknown)}")
            g.update(genotype)
            weighted = bool(g["weighted"])
            row = _gt_params(g["ploidy"], g["err_q"], g["het_q"], min_depth, 0, WQ_COSTS if weighted and g["costs"] is None else g["costs"])
            if not 0 <= int(g["min_gq"]) < 2 ** 32:
                raise ValueError("min_gq is an unsigned 32-bit number")
            params = capi.ConsGtParams(row, _gt_params(g["ploidy"], g["err_q"], g["het_q"], min_depth, 0), int(min_depth), int(g["min_gq"]),
                                       int(weighted))
        stats = (C.c_uint64 * (5 if params is None else 8))()
        with torch.cuda.device(dev):
            bd = torch.from_numpy(b.view(np.int64)).to(dev) if m else None
            offs = torch.zeros(max(m, 1), dtype=torch.int64, device=dev)
            for attempt in (0, 1):
                out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
                if params is None:
                    rc = capi.lib().slamem_pileup_consensus_device(self._h, first, count, int(min_depth), cap, _ptr(out),
                                                                   _ptr(bd) if m else None, m, _ptr(offs) if m else None, stats,
                                                                   C.byref(total), _stream_handle(dev))
                else:
                    rc = capi.lib().slamem_pileup_consensus_gt_device(self._h, first, count, C.byref(params), cap, _ptr(out),
                                                                      _ptr(bd) if m else None, m, _ptr(offs) if m else None, stats,
                                                                      C.byref(total), _stream_handle(dev))
                if rc != capi.SLAMEM_ERR_CAPACITY or attempt:
                    break
                cap = int(total.value)
            capi.check(rc)
            torch.cuda.current_stream(dev).synchronize()
        t = int(total.value)
        return out[:t].cpu().numpy(), offs[:m].cpu().numpy().view(np.uint64), [int(v) for v in stats]

    def depth_runs(self, levels=None, min_depth: int = 1, first: int = 0, count=None, bounds=None, capacity=None):
        """The depth of coverage d = A+C+G+T+D of rows [first, first + count) as runs, built on the device, as
        (pos uint64 (r,), value uint64 (r,), cum uint64 (m, 2)): run i spans rows [pos[i], pos[i + 1]), the last one ends at
        first + count, runs of depth 0 included.  levels: up to 16 ascending depths of at least 1; the value of a run is then the
        number of levels its depth reaches, without levels the depth itself.  bounds: non-decreasing rows in
        [first, first + count]; cum[j] is (the sum of d, the rows with d >= min_depth) over the rows in front of bounds[j].
        capacity: runs of room for the first attempt (default: one in 8 of the range, at least 4,096); when there are more the
        call is made once more with the need it reported."""
        first = int(first)
        count = self.index.n - first if count is None else int(count)
        dev = self.index.device
        lv = np.zeros(0, dtype=np.uint32) if levels is None else np.ascontiguousarray(np.asarray(levels, dtype=np.uint32).reshape(-1))
        b = np.zeros(0, dtype=np.uint64) if bounds is None else np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64).reshape(-1))
        m = len(b)
        cap = max(4096, count // 8) if capacity is None else int(capacity)
        total = C.c_uint64()
        with torch.cuda.device(dev):
            bd = torch.from_numpy(b.view(np.int64)).to(dev) if m else None
            cum = torch.zeros((max(m, 1), 2), dtype=torch.int64, device=dev)
            for attempt in (0, 1):
                out = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=dev)
                rc = capi.lib().slamem_pileup_depth_runs_device(self._h, first, count, lv.ctypes.data if len(lv) else None, len(lv),
                                                                int(min_depth), cap, _ptr(out), _ptr(bd) if m else None, m,
                                                                _ptr(cum) if m else None, C.byref(total), _stream_handle(dev))
                if rc != capi.SLAMEM_ERR_CAPACITY or attempt:
                    break
                cap = int(total.value)
            capi.check(rc)
            torch.cuda.current_stream(dev).synchronize()
        runs = out[:int(total.value)].cpu().numpy().view(np.uint64)
        return np.ascontiguousarray(runs[:, 0]), np.ascontiguousarray(runs[:, 1]), cum[:m].cpu().numpy().view(np.uint64)

    def reset(self) -> None:
        capi.check(capi.lib().slamem_pileup_reset(self._h))

    def close(self) -> None:
        h, self._h = self._h, None
        for view in (self.forward, getattr(self, "quality", None)):  # (the handles go with this one)
            if view is not None:
                view._h = None
        if h and self._owner is None:
            capi.lib().slamem_pileup_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# -stats: the sections of the table as (first word, words), in the order of include/slamem_hip.h
STATS_SECTIONS = {"totals": (0, 24), "mapq": (24, 64), "len": (88, 512), "nm": (600, 128), "cyc_aln": (728, 512), "cyc_mm": (1240, 512),
                  "cyc_ins": (1752, 512), "cyc_del": (2264, 512), "sub": (2776, 16), "q_aln": (2792, 96), "q_mm": (2888, 96),
                  "ins_len": (2984, 64), "del_len": (3048, 64)}
STATS_WORDS = 3112  # SLAMEM_STATS_WORDS
# the launch of the add (stats_filter.hip): lanes of a workgroup, a read each a trip; trips a workgroup makes at least; workgroups at most
STATS_BLOCK, STATS_TRIPS, STATS_GRID = 256, 4, 1024


class MapStats:
    """slamem_stats_*: the mapping QC table (-stats), STATS_WORDS uint64 counters in the sections of
    STATS_SECTIONS, added up on the GPU over every batch since creation or the last reset(), whatever the split into batches and
    their order.  A read is counted when it is mapped and its mapq >= min_mapq; include/slamem_hip.h defines every section."""

    def __init__(self, index: Index):
        self.index = index
        self._h = C.c_void_p()
        capi.check(capi.lib().slamem_stats_create(index._h, C.byref(self._h)))
        self.last_add_ms = 0.0  # device time of the last add's own kernel (the mapping in front of it not counted)

    def add(self, queries, offsets, min_len: int = 20, both_strands: bool = False, max_gap: int = 0, penalty: int = 0, xdrop=None,
            max_edits=None, min_mapq: int = 0, quals=None, phred_offset: int = 33, gap_costs=None, end_band: int = 0):
        """Maps the batch as Index.map_reads does and adds it to the table on the device: segments and operations are not
        downloaded.  Returns the read records of map_reads (MAP_DTYPE).  quals: the batch's quality bytes, a uint8 array (numpy, or
        a tensor on the index's device) of at least offsets[-1] bytes in which byte offsets[r] + i belongs to letter i of read r as
        given, Phred + phred_offset (0 to 126); None: the sections q_aln and q_mm stay as they are.  gap_costs and end_band: as for
        Index.map_reads."""
        quals = self._check(offsets, min_mapq, quals, phred_offset)
        return self.index._aln_like(queries, offsets, min_len, both_strands, max_gap, penalty, xdrop, aln_word(max_edits, gap_costs), None, True,
                                    pile=(self, int(min_mapq), None, False, None if quals is None else (quals, int(phred_offset))),
                                    end_band=_end_band(end_band, gap_costs))

    def add_mapped(self, queries, offsets, result, min_mapq: int = 0, quals=None, phred_offset: int = 33) -> None:
        """Adds a batch that is mapped already: result is what Index.map_reads returned for (queries, offsets) -- its first five
        values are looked at."""
        quals = self._check(offsets, min_mapq, quals, phred_offset)
        dev = self.index.device
        segs, roff, ops, ooff, reads = result[:5]
        q = np.ascontiguousarray(np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else queries, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        num = offsets.shape[0] - 1
        if len(reads) != num or len(roff) != num + 1 or len(ooff) != len(segs) + 1:
            raise ValueError("result is not the mapping of this batch: a record per read, read offsets, an operation offset per segment")

        def up(a, dtype, pad):
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            t = torch.zeros(raw.shape[0] + pad, dtype=torch.uint8, device=dev)
            if raw.shape[0]:
                t[: raw.shape[0]] = torch.from_numpy(raw.copy()).to(dev)
            return t
        abi = np.zeros(num, dtype=_MAP_ABI)
        for f in ("s1", "s2", "strand", "mapq"):
            abi[f] = reads[f]
        seg5 = np.zeros((len(segs), 5), dtype=np.uint32)
        for k, f in enumerate(("ref_pos", "query_pos", "ref_len", "query_len", "edits")):
            seg5[:, k] = segs[f]
        self._add_device(up(q, np.uint8, 16), up(offsets, np.uint64, 0), num, up(seg5, np.uint32, 20), up(np.asarray(roff, dtype=np.uint64), np.uint64, 0),
                         up(np.asarray(ops, dtype=np.uint32), np.uint32, 4), up(np.asarray(ooff, dtype=np.uint64), np.uint64, 0), up(abi, _MAP_ABI, 12),
                         int(min_mapq), quals=None if quals is None else (quals, int(phred_offset)))

    def _check(self, offsets, min_mapq, quals, phred_offset):
        if not 0 <= int(min_mapq) <= 60:
            raise ValueError("min_mapq must be in [0, 60]")
        if quals is None:
            return None
        need = int(np.asarray(offsets)[-1])
        if isinstance(quals, torch.Tensor):
            if quals.dtype != torch.uint8 or quals.device != self.index.device or not quals.is_contiguous():
                raise ValueError("quals as a tensor: contiguous uint8 bytes on the index's device")
        else:
            quals = np.ascontiguousarray(np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals)
            if quals.dtype != np.uint8:
                raise ValueError("quals must be a uint8 array")
        if quals.shape[0] < need:
            raise ValueError(f"quals has {quals.shape[0]} bytes, the batch's letters need {need}")
        if not 0 <= int(phred_offset) <= 126:
            raise ValueError("phred_offset must be in [0, 126]")
        return quals

    def _add_device(self, qd, od, num, segs, roff, ops, ooff, recs, min_mapq, lowq=None, dedup=False, quals=None):
        """The batch as it lies on the device (the signature of Pileup._add_device: Index._aln_like calls either).  quals: (bytes,
        phred_offset)."""
        dev = self.index.device
        qb, off = None, 33
        if quals is not None:
            qb, off = quals
            if not isinstance(qb, torch.Tensor):
                t = torch.zeros(qb.shape[0] + 8, dtype=torch.uint8, device=dev)
                if qb.shape[0]:
                    t[: qb.shape[0]] = torch.from_numpy(qb if qb.flags.writeable else qb.copy()).to(dev)
                qb = t
        with torch.cuda.device(dev):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rc = capi.lib().slamem_stats_add_device(self._h, _ptr(qd), _ptr(od), num, _ptr(segs), _ptr(roff), _ptr(ops), _ptr(ooff),
                                                    _ptr(recs), _ptr(qb) if qb is not None else None, int(off), int(min_mapq),
                                                    _stream_handle(dev))
            t1.record()
            capi.check(rc)
            t1.synchronize()  # (the batch's tensors go when the caller returns)
            self.last_add_ms = float(t0.elapsed_time(t1))

    def raw(self) -> np.ndarray:
        """The table: a uint64 array of STATS_WORDS.  The accumulator is left as it is."""
        out = np.zeros(STATS_WORDS, dtype=np.uint64)
        capi.check(capi.lib().slamem_stats_table_host(self._h, out.ctypes.data))
        return out

    def table(self) -> dict:
        """The table by section: name -> a view of raw()."""
        raw = self.raw()
        return {k: raw[a: a + n] for k, (a, n) in STATS_SECTIONS.items()}

    def add_table(self, raw) -> None:
        """Adds another table (raw() of an accumulator, of another GPU for instance) to this one."""
        t = np.ascontiguousarray(raw, dtype=np.uint64)
        if t.shape != (STATS_WORDS,):
            raise ValueError(f"a table has {STATS_WORDS} words")
        capi.check(capi.lib().slamem_stats_add_table_host(self._h, t.ctypes.data))

    def reset(self) -> None:
        capi.check(capi.lib().slamem_stats_reset(self._h))

    def close(self) -> None:
        h, self._h = self._h, None
        if h:
            capi.lib().slamem_stats_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def event_letters(ev) -> bytes:
    """The inserted letters of one event (an element of Pileup.events()' array) as bytes; b"" for a deletion."""
    if int(ev["kind"]) != 1:
        return b""
    k, v = int(ev["len"]), int(ev["letters"])
    return bytes(b"ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


class Matcher:
    """Pre-allocated output + workspace buffers for repeated slamem_find_mems_device calls (bench loop)."""

    def __init__(self, index: Index, num_queries: int, both_strands: bool, mems_capacity: int, query_bytes: int,
                 mam: bool = False, mum: bool = False, smem: bool = False, max_occ: int = 0, chain: bool = False,
                 max_gap: int = 0, ext: bool = False, penalty: int = 0, xdrop=None):
        self.index = index
        self.match_type = _match_type(mam, mum, smem, max_occ, chain, max_gap, ext, penalty, xdrop)
        self.ext = self.match_type == 5
        self.penalty = int(penalty)
        self.xdrop = _xdrop_arg(xdrop)
        self.mam = self.match_type == 1
        self.mum = self.match_type == 2
        self.smem = self.match_type == 3
        self.max_occ = int(max_occ)
        self.chain = self.match_type == 4
        self.max_gap = int(max_gap)
        self.num_queries = int(num_queries)
        self.both = bool(both_strands)
        self.capacity = int(mems_capacity)
        self.query_bytes = int(query_bytes)
        dev = index.device
        nb = self.num_queries * (2 if self.both else 1)
        need = C.c_uint64()
        L = capi.lib()
        ws_fn = (L.slamem_find_mems_workspace_bytes, L.slamem_find_mems_workspace_bytes, L.slamem_find_mums_workspace_bytes,
                 L.slamem_find_smems_workspace_bytes, L.slamem_find_chains_workspace_bytes,
                 L.slamem_find_exts_workspace_bytes)[self.match_type]
        capi.check(ws_fn(self.num_queries, int(self.both), self.query_bytes, self.capacity, C.byref(need)))
        self.workspace = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
        self.mems = torch.empty((max(self.capacity, 1), 3), dtype=torch.int32, device=dev)
        self.block_offsets = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        if self.chain:  # a uint32 per strand block: the score of its chain
            self.scores = torch.zeros(nb, dtype=torch.int32, device=dev)
        if self.ext:  # a uint32 per row: its mismatches
            self.mismatches = torch.zeros(max(self.capacity, 1), dtype=torch.int32, device=dev)
        self.last_total = 0

    def run(self, queries_dev: torch.Tensor, offsets_dev: torch.Tensor, min_len: int) -> int:
        dev = self.index.device
        total = C.c_uint64()
        L = capi.lib()
        fn = (L.slamem_find_mems_device, L.slamem_find_mams_device, L.slamem_find_mums_device,
              L.slamem_find_smems_device, L.slamem_find_chains_device, L.slamem_find_exts_device)[self.match_type]
        occ = (self.max_occ,) if self.smem else (self.max_gap,) if self.chain else (self.penalty, self.xdrop) if self.ext else ()
        scores = (_ptr(self.scores),) if self.chain else (_ptr(self.mismatches),) if self.ext else ()
        rc = fn(
            self.index._h, _ptr(queries_dev), _ptr(offsets_dev), self.num_queries, self.query_bytes, int(min_len),
            int(self.both), *occ,
            _ptr(self.mems), self.capacity, _ptr(self.block_offsets), *scores, _ptr(self.workspace), self.workspace.numel(),
            _stream_handle(dev), C.byref(total))
        self.last_total = int(total.value)
        capi.check(rc)
        return self.last_total


class PinnedBuffer:
    """Page-locked host memory from slamem_pinned_alloc, viewed as a numpy uint8 array (a front end's read buffer)."""

    def __init__(self, nbytes: int):
        self._p = C.c_void_p()
        capi.check(capi.lib().slamem_pinned_alloc(C.byref(self._p), int(nbytes)))
        self.nbytes = int(nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self._p.value))

    def close(self):
        p, self._p = self._p, None
        if p:
            self.array = None
            capi.lib().slamem_pinned_free(p)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    """slamem_stream_*: host-to-host MEM retrieval, pipelined over `slots` lanes (include/slamem_hip.h).  Replaces the
    query loop of GetMatches (slamem.c:90-207) for reads that live in host memory."""

    def __init__(self, index: Index, slots: int, max_batch_chars: int, max_batch_queries: int, both_strands: bool,
                 mam: bool = False, mum: bool = False, smem: bool = False, max_occ: int = 0, chain: bool = False,
                 max_gap: int = 0, ext: bool = False, penalty: int = 0, xdrop=None, aln: bool = False, max_edits=None, paf: bool = False,
                 pile: "Pileup" = None, min_mapq: int = 0, md: bool = False, dedup: bool = False, quals: bool = False,
                 phred_offset: int = 33, stats: "MapStats" = None, gap_costs=None, end_band: int = 0):
        """gap_costs=(x, o, e) (with aln, paf or pile): the gaps of every batch are closed at gap-affine cost, as
        Index.find_alns(gap_costs=) closes them.
        end_band=Z (with gap_costs): the outer ends of every batch as Index.find_alns(end_band=) builds them.
        stats=<MapStats> (with paf=True or pile=<Pileup>): every batch is also added to the table on the device,
        behind its map pass, counting the reads with mapq >= min_mapq; with quals=True the batches come through submit_quals and
        their quality bytes feed the table's quality sections (on a pile= stream whose accumulator has quality sums, they feed both).
        md=True (with paf=True): every batch also goes through the MD pass and mds() gives (md, md_offsets,
        seg_eq, primary) of the batch next() returned last, as Index.map_reads(md=True) appends them.
        dedup=True (with pile=<Pileup> made with dedup=True): every batch is added through the duplicate filter, in
        the order of the submits, and dups() gives the flags of the batch next() returned last.
        quals=True (with pile=<Pileup> made with quals=True): every batch comes through submit_quals with its quality
        bytes (Phred + phred_offset).
        pile=<Pileup>: -pile mode (match type 8): every batch is mapped as with paf=True and added to the accumulator on the
        device (the reads with mapq >= min_mapq); next() then returns (number of segments piled, None, timings) and maps() the read
        records; the segments are not downloaded.  It takes the parameters of paf and excludes the other modes.  aln=True: -aln mode (match type 6); it takes max_gap, penalty, xdrop and max_edits and excludes the other modes.
        next() then returns the segments (ALN_DTYPE) in the place of the rows, alns() their operations.  paf=True: -paf mode
        (match type 7), the same with the offsets per READ and maps() the read records (MAP_DTYPE)."""
        self.pile = pile
        self.stats = stats
        if stats is not None and not (paf or pile is not None):
            raise ValueError("stats is the table of the mappings: it needs paf=True or pile=<Pileup>")
        if quals and pile is None and stats is None:
            raise ValueError("quals are the quality bytes of pile and of stats: it needs pile=<Pileup> or stats=<MapStats>")
        if dedup and pile is None:
            raise ValueError("dedup is the duplicate filter of pile: it needs pile=<Pileup>")
        self.dedup = bool(dedup)
        if pile is not None and (aln or paf):
            raise ValueError("pile excludes aln and paf: one match type per search")
        if min_mapq and pile is None and stats is None:
            raise ValueError("min_mapq is the threshold of pile and of stats: it needs pile=<Pileup> or stats=<MapStats>")
        paf = bool(paf or pile is not None)
        if (aln or paf) and (mam or mum or smem or chain or ext or max_occ or (aln and paf)):
            raise ValueError("aln, paf and pile exclude mam, mum, smem, chain, ext and each other: one match type per search")
        if max_edits is not None and not (aln or paf):
            raise ValueError("max_edits is the edit limit of aln and paf: it needs aln=True or paf=True")
        if gap_costs is not None and not (aln or paf):
            raise ValueError("gap_costs are the costs of aln and paf: it needs aln=True, paf=True or pile=<Pileup>")
        max_edits = aln_word(max_edits, gap_costs)
        end_band = _end_band(end_band, gap_costs)
        if md and not (paf and pile is None):
            raise ValueError("md is the MD pass of paf: it needs paf=True")
        self.paf = bool(paf)
        self.aln = bool(aln or paf)
        self.md = bool(md)
        match_type = 8 if pile is not None else 7 if paf else 6 if aln else _match_type(mam, mum, smem, max_occ, chain, max_gap, ext, penalty, xdrop)
        self.index = index
        self.both = bool(both_strands)
        self._h = C.c_void_p()
        capi.check(capi.lib().slamem_stream_create(index._h, int(slots), int(max_batch_chars), int(max_batch_queries),
                                                   int(self.both), match_type, C.byref(self._h)))
        try:
            if max_occ:
                capi.check(capi.lib().slamem_stream_set_max_occ(self._h, int(max_occ)))
            if max_gap:
                capi.check(capi.lib().slamem_stream_set_max_gap(self._h, int(max_gap)))
            if penalty or xdrop is not None:
                capi.check(capi.lib().slamem_stream_set_ext_params(self._h, int(penalty), _xdrop_arg(xdrop)))
            if max_edits is not None:
                capi.check(capi.lib().slamem_stream_set_max_edits(self._h, int(max_edits)))
            if end_band:
                capi.check(capi.lib().slamem_stream_set_end_band(self._h, end_band))
            if pile is not None:
                capi.check(capi.lib().slamem_stream_set_pileup(self._h, pile._h, int(min_mapq)))
            if dedup:
                capi.check(capi.lib().slamem_stream_set_dedup(self._h, 1))
            if md:
                capi.check(capi.lib().slamem_stream_set_md(self._h, 1))
            if quals and (stats is None or (pile is not None and pile.quality is not None)):
                capi.check(capi.lib().slamem_stream_set_quals(self._h, int(phred_offset)))
            elif quals and int(phred_offset) != 33:
                raise ValueError("the quality bytes of a stats stream are Phred + 33 (another offset: an accumulator with quality sums)")
            if stats is not None:
                capi.check(capi.lib().slamem_stream_set_stats(self._h, stats._h, int(min_mapq), int(bool(quals))))
        except Exception:
            # a setter refused: the stream goes at once, while its index is alive -- not when the exception's traceback, which
            # holds this object, happens to be collected (by then the caller may have closed the index)
            self.close()
            raise
        self._keep = []
        self._last_total = 0

    def submit(self, chars: np.ndarray, offsets: np.ndarray, min_len: int) -> None:
        """chars: uint8 array holding the records; offsets: uint64[num+1] into it (offsets[0] need not be 0)."""
        assert chars.dtype == np.uint8 and offsets.dtype == np.uint64 and offsets.flags.c_contiguous
        self._keep.append((chars, offsets))  # must stay alive and unchanged until collected
        capi.check(capi.lib().slamem_stream_submit(self._h, chars.ctypes.data, offsets.ctypes.data, offsets.shape[0] - 1,
                                                   int(min_len)))

    def submit_masked(self, chars: np.ndarray, lowq, offsets: np.ndarray, min_len: int) -> None:
        """submit for a -pile stream with the batch's low-quality mask: lowq is a uint64 array indexed as chars is
        -- bit offsets[r] + i belongs to letter i of record r, whatever offsets[0] is.  None: submit."""
        assert chars.dtype == np.uint8 and offsets.dtype == np.uint64 and offsets.flags.c_contiguous
        assert lowq is None or (lowq.dtype == np.uint64 and lowq.flags.c_contiguous)
        self._keep.append((chars, lowq, offsets))
        capi.check(capi.lib().slamem_stream_submit_masked(self._h, chars.ctypes.data, lowq.ctypes.data if lowq is not None else None,
                                                          offsets.ctypes.data, offsets.shape[0] - 1, int(min_len)))

    def submit_quals(self, chars: np.ndarray, quals: np.ndarray, lowq, offsets: np.ndarray, min_len: int) -> None:
        """submit for a stream made with quals=True (a -pile stream, DESIGN.md 4.27, or one with stats=): quals is a uint8 array indexed as chars is -- byte
        offsets[r] + i is the quality of letter i of record r, whatever offsets[0] is; lowq as in submit_masked, or None."""
        assert chars.dtype == np.uint8 and quals.dtype == np.uint8 and quals.flags.c_contiguous
        assert offsets.dtype == np.uint64 and offsets.flags.c_contiguous and quals.shape[0] >= int(offsets[-1])
        assert lowq is None or (lowq.dtype == np.uint64 and lowq.flags.c_contiguous)
        self._keep.append((chars, quals, lowq, offsets))
        capi.check(capi.lib().slamem_stream_submit_quals(self._h, chars.ctypes.data, quals.ctypes.data,
                                                         lowq.ctypes.data if lowq is not None else None, offsets.ctypes.data,
                                                         offsets.shape[0] - 1, int(min_len)))

    def submit_packed(self, planes: np.ndarray, other, offsets: np.ndarray, min_len: int, units: int = 0) -> None:
        """planes: uint8 view of the batch's 16-byte units (slamem_pack_reads layout), other: uint64 per unit or None; offsets:
        uint64[num+1] in letters.  All must stay alive and unchanged until collected."""
        assert planes.dtype == np.uint8 and offsets.dtype == np.uint64 and offsets.flags.c_contiguous
        self._keep.append((planes, other, offsets))
        capi.check(capi.lib().slamem_stream_submit_packed(self._h, planes.ctypes.data, other.ctypes.data if other is not None else None,
                                                          offsets.ctypes.data, offsets.shape[0] - 1, int(units), int(min_len)))

    def next(self, copy: bool = True):
        """(mems structured array, block_offsets uint64 array, timings dict) of the oldest batch.  copy=False returns
        views of the stream's pinned buffers, valid until the next call."""
        mems, boff, total, nq, tm = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32(), capi.Timings()
        rc = capi.lib().slamem_stream_next(self._h, C.byref(mems), C.byref(boff), C.byref(total), C.byref(nq), C.byref(tm))
        if self._keep:
            self._keep.pop(0)
        capi.check(rc)
        self._last_total = int(total.value)
        nb = nq.value * (1 if self.paf else 2 if self.both else 1)
        if self.pile is not None:  # the segments stayed on the device: their number, and the read records through maps()
            recs = C.c_void_p()
            capi.check(capi.lib().slamem_stream_maps(self._h, C.byref(recs)))
            raw = np.ctypeslib.as_array((C.c_uint8 * (12 * max(1, nq.value))).from_address(recs.value))[: 12 * nq.value]
            self._last_maps = _map_records(raw)
            if self.dedup:
                flags = C.c_void_p()
                capi.check(capi.lib().slamem_stream_dups(self._h, C.byref(flags)))
                self._last_dups = np.ctypeslib.as_array((C.c_uint8 * max(1, nq.value)).from_address(flags.value))[: nq.value].copy()
            return int(total.value), None, tm.as_dict()
        if self.aln:  # the segments stand in the place of the rows
            segs, ops, ooff, nops = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
            capi.check(capi.lib().slamem_stream_alns(self._h, C.byref(segs), C.byref(ops), C.byref(ooff), C.byref(nops)))
            n = int(total.value)
            m = np.ctypeslib.as_array((C.c_uint8 * (20 * max(1, n))).from_address(segs.value))[: 20 * n].view(ALN_DTYPE)
            o = np.ctypeslib.as_array((C.c_uint32 * max(1, nops.value)).from_address(ops.value))[: nops.value]
            oo = np.ctypeslib.as_array((C.c_uint64 * (n + 1)).from_address(ooff.value))
            b = np.ctypeslib.as_array((C.c_uint64 * (nb + 1)).from_address(boff.value))
            self._last_alns = (o.copy(), oo.copy()) if copy else (o, oo)
            if self.paf:
                recs = C.c_void_p()
                capi.check(capi.lib().slamem_stream_maps(self._h, C.byref(recs)))
                raw = np.ctypeslib.as_array((C.c_uint8 * (12 * max(1, nq.value))).from_address(recs.value))[: 12 * nq.value]
                self._last_maps = _map_records(raw)
            if self.md:
                p = [C.c_void_p() for _ in range(4)]
                nmd = C.c_uint64()
                capi.check(capi.lib().slamem_stream_md(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3]), C.byref(nmd)))
                self._last_mds = (
                    np.ctypeslib.as_array((C.c_uint32 * max(1, nmd.value)).from_address(p[0].value))[: nmd.value].copy(),
                    np.ctypeslib.as_array((C.c_uint64 * (n + 1)).from_address(p[1].value)).copy(),
                    np.ctypeslib.as_array((C.c_uint32 * max(1, n)).from_address(p[2].value))[:n].copy(),
                    np.ctypeslib.as_array((C.c_uint32 * max(1, nq.value)).from_address(p[3].value))[: nq.value].copy())
            return (m.copy(), b.copy(), tm.as_dict()) if copy else (m, b, tm.as_dict())
        m = np.ctypeslib.as_array((C.c_uint8 * (12 * max(1, total.value))).from_address(mems.value))[: 12 * total.value]
        m = m.view(MEM_DTYPE)
        b = np.ctypeslib.as_array((C.c_uint64 * (nb + 1)).from_address(boff.value))
        if copy:
            m, b = m.copy(), b.copy()
        return m, b, tm.as_dict()

    def alns(self):
        """-aln: (ops, op_offsets) of the batch next() returned last (slamem_stream_alns), as next() took them."""
        return self._last_alns

    def maps(self):
        """-paf: the read records (MAP_DTYPE) of the batch next() returned last (slamem_stream_maps), as next() took them."""
        return self._last_maps

    def dups(self):
        """dedup=True: the duplicate flags (uint8 per read, as Pileup.add(dedup=True) returns them) of the batch next() returned
        last (slamem_stream_dups), copied."""
        return self._last_dups

    def mds(self):
        """md=True: (md, md_offsets, seg_eq, primary) of the batch next() returned last (slamem_stream_md), copied."""
        return self._last_mds

    def mismatches(self, copy: bool = True) -> np.ndarray:
        """-ext: the mismatches (uint32 per row) of the batch next() returned last (slamem_stream_mismatches).  copy=False
        returns a view of the stream's pinned buffer, valid until the next call of next()."""
        p = C.POINTER(C.c_uint32)()
        capi.check(capi.lib().slamem_stream_mismatches(self._h, C.byref(p)))
        if self._last_total == 0:
            return np.zeros(0, dtype=np.uint32)
        a = np.ctypeslib.as_array(p, shape=(self._last_total,))
        return a.copy() if copy else a

    def close(self):
        h, self._h = self._h, None
        if h:
            capi.lib().slamem_stream_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_reads(chars: np.ndarray, offsets: np.ndarray, planes_out: np.ndarray, other_out, threads: int = 16) -> int:
    """slamem_pack_reads: letters -> bit-planes (16-byte units) on the host; returns the number of units."""
    units = C.c_uint64()
    capi.check(capi.lib().slamem_pack_reads(chars.ctypes.data, offsets.ctypes.data, offsets.shape[0] - 1, planes_out.ctypes.data,
                                            other_out.ctypes.data if other_out is not None else None, C.byref(units), int(threads)))
    return int(units.value)


def pack_lowq(quals, min_bq: int, phred_offset: int = 33, device=False, threads: int = 16):
    """The low-quality mask of a letter buffer's quality bytes: letter j is low iff max(0, quals[j] - phred_offset)
    < min_bq (min_bq 0 to 93, phred_offset 0 to 126).  Returns (len + 63) // 64 uint64 words, bit j % 64 of word j // 64 for
    letter j, the last word's unused bits 0.  device=False: slamem_pack_lowq on the host, a numpy array.  device=True (or a device):
    the bytes go up and k_lowq_pack packs them; an int64 tensor on that device, which Pileup.add(lowq=...) takes as it is."""
    q = np.ascontiguousarray(np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals, dtype=np.uint8)
    total, words = int(q.shape[0]), (int(q.shape[0]) + 63) // 64
    if not 0 <= int(min_bq) < 2 ** 32 or not 0 <= int(phred_offset) < 2 ** 32:
        raise ValueError("min_bq and phred_offset are whole numbers from 0")
    L = capi.lib()
    if device is False or device is None:
        out = np.zeros(words, dtype=np.uint64)
        capi.check(L.slamem_pack_lowq(q.ctypes.data if total else None, total, int(min_bq), int(phred_offset),
                                      out.ctypes.data if words else None, int(threads)))
        return out
    dev = _require_gpu("cuda:0" if device is True else device)
    qd = torch.from_numpy(q if q.flags.writeable else q.copy()).to(dev)
    out = torch.zeros(words, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        capi.check(L.slamem_pack_lowq_device(_ptr(qd) if total else None, total, int(min_bq), int(phred_offset),
                                             _ptr(out) if words else None, _stream_handle(dev)))
        torch.cuda.current_stream(dev).synchronize()
    return out


def host_to_host_leg(index: Index, reads_dev: torch.Tensor, count: int, read_len: int, min_len: int, both: bool,
                     steps: int = 2, batch_reads: int = 1_000_000, slots: int = 6, schedule=None, packed: bool = False) -> dict:
    """SURVEY.md 8(d)'s metric as defined -- reads resident in host memory -> MEM triples in host memory -- through
    slamem_stream_*: the reads sit in pinned host memory, batches of `batch_reads` are pipelined over `slots` lanes, and
    the clock runs from the first submit to the last result.  Returns fields for the bench line."""
    import time
    L = read_len
    buf = PinnedBuffer(count * L + 64)
    # (one DMA into the pinned buffer: torch's .cpu() of 1.5 GB goes through the runtime's staged copy of pageable memory)
    torch.cuda.synchronize(reads_dev.device)
    capi.check(capi.lib().slamem_copy_to_host(buf.array.ctypes.data, _ptr(reads_dev), count * L))
    # the record offsets live in pinned memory like the reads: 8 bytes per read go up with every batch, and from pageable
    # memory that copy runs at a fifth of the link's rate (measured: 0.8 ms of a 3.6 ms upload per million reads)
    obuf = PinnedBuffer((count + 1) * 8)
    offsets = obuf.array.view(np.uint64)
    offsets[:] = np.arange(count + 1, dtype=np.uint64) * np.uint64(L)
    # batch boundaries: short batches first (the pipeline starts searching after a quarter of a batch is up), or the sizes
    # the caller asks for (`schedule`, in reads; the last size repeats)
    cuts, pos = [0], 0
    sizes = list(schedule) if schedule else [batch_reads // 4, batch_reads // 2]
    for size in sizes:
        if 0 < size and pos + size < count:
            pos += size
            cuts.append(pos)
    tail = (sizes[-1] if schedule else batch_reads) or batch_reads
    while pos < count:
        pos = min(count, pos + tail)
        cuts.append(pos)
    nb = len(cuts) - 1
    biggest = int(np.diff(np.array(cuts)).max())
    pbuf, upr = None, (L + 63) // 64  # packed: the reads as bit-planes in pinned memory (made once, before the clock starts)
    if packed:
        pbuf = PinnedBuffer(count * upr * 16 + 64)
        assert pack_reads(buf.array, offsets, pbuf.array, None) == count * upr
    st = Stream(index, slots, biggest * L, biggest, both)

    def submit(b):
        if packed:
            st.submit_packed(pbuf.array[cuts[b] * upr * 16:], None, offsets[cuts[b]: cuts[b + 1] + 1], min_len, units=(cuts[b + 1] - cuts[b]) * upr)
        else:
            st.submit(buf.array, offsets[cuts[b]: cuts[b + 1] + 1], min_len)
    passes, total_mems, kernel_ms = [], 0, 0.0
    try:
        for rep in range(steps + 1):  # first pass warms the stream's buffers up
            t0 = time.perf_counter()
            got, kms = 0, 0.0
            for b in range(min(slots - 1, nb)):
                submit(b)
            marks = []
            for b in range(nb):
                m, _, tm = st.next(copy=False)
                got += len(m)
                kms += tm["search_kernel_ms"]
                marks.append((time.perf_counter(), len(m)))
                nxt = b + slots - 1
                if nxt < nb:
                    submit(nxt)
            dt = time.perf_counter() - t0
            if rep:
                # the pipeline's rate once it is full: results of the full-size batches in the middle of the run
                lo, hi = min(3, nb - 1), max(nb - 2, 0)
                steady = (sum(c for _, c in marks[lo + 1: hi + 1]) / (marks[hi][0] - marks[lo][0])) if hi > lo + 1 else None
                passes.append((dt, steady))
            total_mems, kernel_ms = got, kms
    finally:
        st.close()
        offsets = None
        obuf.close()
        buf.close()
        if pbuf is not None:
            pbuf.close()
    passes.sort(key=lambda x: x[0])
    best = passes[0][0]
    med, steady = passes[len(passes) // 2] if len(passes) % 2 else \
        ((passes[len(passes) // 2 - 1][0] + passes[len(passes) // 2][0]) / 2, passes[len(passes) // 2][1])
    return {"value_host_to_host": total_mems / med, "host_to_host_ms": med * 1e3, "host_to_host_mems": int(total_mems),
            "host_to_host": {"batches": nb, "batch_reads": batch_reads, "slots": slots,
                             "h2d_bytes": (count * upr * 16 if packed else count * L) + 8 * (count + nb), "packed": bool(packed),
                             "passes_ms": [round(p[0] * 1e3, 3) for p in passes], "best_ms": best * 1e3,
                             "d2h_bytes": 12 * int(total_mems) + 8 * (count * (2 if both else 1) + nb),
                             "kernel_ms_sum": kernel_ms,
                             "steady_state_MEMs_per_s": steady,
                             "steady_state_note": "results of the full-size batches in the middle of the run / the time between "
                                                  "them: the pipeline without its ramp and drain (a longer job tends to this)",
                             "note": "reads and record offsets in pinned host memory -> MEMs in pinned host memory through slamem_stream_* "
                                     "(uploads, kernels and downloads of neighbouring batches overlap); MEDIAN of "
                                     f"{steps} passes over the same {count} reads behind one warm-up pass"}}


def build_bytes(n: int, layout: int = capi.LAYOUT_FULL) -> tuple[int, int]:
    """(arena bytes, build peak bytes) of a text of n letters in `layout` (slamem_index_build_bytes; host arithmetic)."""
    a, p = C.c_uint64(), C.c_uint64()
    capi.check(capi.lib().slamem_index_build_bytes(int(n), int(layout), C.byref(a), C.byref(p)))
    return int(a.value), int(p.value)


def timings() -> dict:
    t = capi.Timings()
    capi.check(capi.lib().slamem_get_timings(C.byref(t)))
    return t.as_dict()


def reset_timings() -> None:
    capi.lib().slamem_reset_timings()


def search_stats(matcher: "Matcher", queries_dev: torch.Tensor, offsets_dev: torch.Tensor, min_len: int) -> dict:
    """One extra launch of the search through the diagnostic kernel instantiations: the load counters of K8a / K8 for
    this batch (slamem_search_stats; same results as the normal launch, slower)."""
    L = capi.lib()
    L.slamem_search_stats_enable(1)
    try:
        matcher.run(queries_dev, offsets_dev, min_len)
    finally:
        L.slamem_search_stats_enable(0)
    st = capi.SearchStats()
    capi.check(L.slamem_get_search_stats(C.byref(st)))
    out = st.as_dict()
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    L.slamem_get_search_clock(C.byref(a), C.byref(b), C.byref(c))
    out["k8_us_until_list_empty"], out["k8_us_tail"], out["k8_wave_us_sum"] = a.value, b.value, c.value
    return out


def random_line_ceiling(index: "Index", lanes: int = 256 * 32 * 64 * 4, iters: int = 64) -> float:
    """Dependent random 64-byte-line gathers per second over THIS index arena (read-only), measured in a few ms: every
    lane walks a chain of random lines of the arena, one 16-byte access per line (csrc/synth.hip::k_gather_modes, mode
    0).  The search kernel's request rate is read against this ceiling."""
    dev = index.device
    S = capi.synth_lib()
    arena = index.arena_view()
    nblk = arena.numel() // 64
    sink = torch.zeros(8, dtype=torch.int64, device=dev)
    st = _stream_handle(dev)
    best = 0.0
    for rep in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = S.slamem_gather_modes(arena.data_ptr(), nblk, lanes, iters if rep else 4, 0, sink.data_ptr(), st)
        e1.record()
        if rc:
            raise RuntimeError(f"gather probe launch failed: hip error {rc}")
        torch.cuda.synchronize(dev)
        if rep:
            best = max(best, lanes * iters / (e0.elapsed_time(e1) * 1e-3))
    return best


# ---- bench / test support: synthetic inputs generated on the GPU (csrc/synth.hip) ----------------------
def synth_reference(n: int, seed: int = 42, device="cuda:0") -> torch.Tensor:
    dev = _require_gpu(device)
    out = torch.empty(n + 16, dtype=torch.uint8, device=dev)[:n]
    rc = capi.synth_lib().slamem_synth_reference(_ptr(out), n, seed, _stream_handle(dev))
    if rc:
        raise RuntimeError(f"synth kernel launch failed: hip error {rc}")
    return out


def synth_plant_repeats(ref: torch.Tensor, seed: int = 42) -> int:
    """Repeat model of SURVEY.md 8(d) applied in place to a text made by synth_reference(n, seed); returns the planted
    letters.  Same values as slamem_amd.synth.plant_repeats."""
    planted = C.c_uint64()
    rc = capi.synth_lib().slamem_synth_plant_repeats(_ptr(ref), ref.numel(), seed, _stream_handle(ref.device), C.byref(planted))
    if rc:
        raise RuntimeError(f"synth kernel launch failed: hip error {rc}")
    return int(planted.value)


def synth_plant_genome_like(ref: torch.Tensor, seed: int = 42, n_block: bool = True) -> None:
    """The genome-like repeat load (interspersed family, satellite array, block of N unless n_block=False) applied in place;
    same values as slamem_amd.synth.plant_genome_like."""
    rc = capi.synth_lib().slamem_synth_plant_genome_like(_ptr(ref), ref.numel(), seed, int(bool(n_block)), _stream_handle(ref.device))
    if rc:
        raise RuntimeError(f"synth kernel launch failed: hip error {rc}")


def synth_reads(ref: torch.Tensor, first: int, count: int, length: int = 150, sub: float = 0.02, seed: int = 42,
                rc_percent: int = 0, avoid: tuple = (0, 0)) -> torch.Tensor:
    """avoid = (at, len): reads that would touch text[at, at+len) are drawn behind it (slamem_amd.synth.make_reads)."""
    if count * length >= 1 << 32:
        raise ValueError("synth_reads: one thread per letter, fewer than 2^32 letters per call (make the reads in pieces)")
    dev = ref.device
    out = torch.zeros(count * length + 16, dtype=torch.uint8, device=dev)
    rc = capi.synth_lib().slamem_synth_reads_avoid(_ptr(ref), ref.numel(), _ptr(out), first, count, length, float(sub), seed,
                                                   rc_percent, int(avoid[0]), int(avoid[1]), _stream_handle(dev))
    if rc:
        raise RuntimeError(f"synth kernel launch failed: hip error {rc}")
    return out


def md_text(entries) -> bytes:
    """The MD:Z: text of ONE segment's MD entries (rule 2): an X entry prints m and the letter; a D entry with
    m == 0 whose predecessor is a D entry continues that ^ group, any other D entry prints m, ^ and the letter; the closing entry
    prints m."""
    out = []
    prev_d = False
    for e in entries:
        e = int(e)
        m = e >> 4
        if e & MD_CLOSE:
            out.append(b"%d" % m)
            break
        letter = b"ACGT"[e & 3:(e & 3) + 1]
        if e & 4:
            out.append(letter if (prev_d and m == 0) else b"%d^" % m + letter)
            prev_d = True
        else:
            out.append(b"%d" % m + letter)
            prev_d = False
    return b"".join(out)
