"""ctypes view of slamem_amd/host/libslamem_host.so (the front end's host logic) for the CPU tests."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "slamem_amd", "host")


class Record(C.Structure):
    _fields_ = [("name", C.c_char_p), ("size", C.c_uint32)]


class SeqSet(C.Structure):
    _fields_ = [("recs", C.POINTER(Record)), ("num", C.c_int), ("chars", C.POINTER(C.c_char)), ("total", C.c_uint64),
                ("offsets", C.POINTER(C.c_uint64)), ("merged_start", C.POINTER(C.c_uint32)), ("file_bytes", C.c_long),
                ("name_arena", C.c_void_p)]


class Options(C.Structure):
    _fields_ = [("usage", C.c_int), ("hidden_sort", C.c_int), ("hidden_clean", C.c_int), ("image_arg", C.c_int),
                ("no_ns", C.c_int), ("min_seq_len", C.c_int), ("ref_name", C.c_char_p), ("ref_name_given", C.c_int),
                ("ref_name_empty", C.c_int), ("match_type", C.c_int), ("both_strands", C.c_int), ("min_mem_len", C.c_int),
                ("out_arg", C.c_int), ("num_files", C.c_int), ("file_args", C.POINTER(C.c_int))]


class Run(C.Structure):
    """slh_run: Options and the values behind the other entry points."""
    _fields_ = [("o", Options)] + [(k, C.c_int) for k in ("max_occ", "max_gap", "ext_pen", "ext_xdrop", "max_edits", "min_mapq", "min_bq",
                                                          "bq_given", "min_depth", "min_pct")] + \
               [("ev_slots", C.c_uint64), ("dd_slots", C.c_uint64), ("levels", C.c_uint32 * 16), ("num_levels", C.c_int),
                ("window", C.c_uint64)] + \
               [(k, C.c_int) for k in ("gt_ploidy", "gt_err", "gt_hetq", "gt_qual", "sites", "vcf", "cons", "depth", "sam", "dedup", "gt")]


class Piece(C.Structure):
    _fields_ = [("rec", C.c_int), ("ends_record", C.c_int), ("start", C.c_uint64), ("a", C.c_uint64), ("b", C.c_uint64)]


def c_argv(args):
    return (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)


def entry_points(args, L=None):
    """Every slh_parse_* entry point on one argument vector: {name: [return code, outputs...]}, and the file arguments."""
    L = L or lib()
    argv, n = c_argv(args), len(args)
    i = [C.c_int() for _ in range(4)]
    u = C.c_uint64()
    out = {}
    for name in ("max_occ", "max_gap", "max_edits", "min_mapq", "min_bq"):
        out[name] = [getattr(L, "slh_parse_" + name)(n, argv, C.byref(i[0])), i[0].value]
    out["ext_params"] = [L.slh_parse_ext_params(n, argv, C.byref(i[0]), C.byref(i[1])), i[0].value, i[1].value]
    out["sites_params"] = [L.slh_parse_sites_params(n, argv, C.byref(i[0]), C.byref(i[1])), i[0].value, i[1].value]
    out["gt_params"] = [L.slh_parse_gt_params(n, argv, *[C.byref(x) for x in i])] + [x.value for x in i]
    out["event_slots"] = [L.slh_parse_event_slots(n, argv, C.byref(u)), u.value]
    out["depth"] = [L.slh_parse_depth(n, argv)]
    out["dedup"] = [L.slh_parse_dedup(n, argv, C.byref(u)), u.value]
    lev = (C.c_uint32 * 16)()
    rc = L.slh_parse_depth_params(n, argv, lev, C.byref(i[0]), C.byref(u))
    out["depth_params"] = [rc, list(lev[:i[0].value]), u.value]
    o = Options()
    rc = L.slh_parse_options(n, argv, C.byref(o))
    out["options"] = [rc] + [getattr(o, k) for k, _ in Options._fields_ if k not in ("file_args", "ref_name")] + \
                     [o.ref_name.decode(errors="replace") if o.ref_name else None]
    out["files"] = [o.file_args[k] for k in range(o.num_files)]
    L.slh_free_options.argtypes = [C.POINTER(Options)]
    L.slh_free_options(C.byref(o))
    return out


def parse_run(args):
    """slh_parse_run: (return code, refusal or None, the values as the old entry points name them)."""
    L = lib()
    r, msg = Run(), C.c_char_p()
    rc = L.slh_parse_run(len(args), c_argv(args), C.byref(r), C.byref(msg))
    vals = {"max_occ": r.max_occ, "max_gap": r.max_gap, "max_edits": r.max_edits, "min_mapq": r.min_mapq, "min_bq": r.min_bq,
            "bq_given": r.bq_given, "ext_params": [r.ext_pen, r.ext_xdrop], "sites_params": [r.min_depth, r.min_pct],
            "gt_params": [r.gt_ploidy, r.gt_err, r.gt_hetq, r.gt_qual], "event_slots": r.ev_slots, "dd_slots": r.dd_slots,
            "levels": list(r.levels[:r.num_levels]), "window": r.window, "depth": r.depth, "dedup": r.dedup,
            "files": [r.o.file_args[k] for k in range(r.o.num_files)] if r.o.file_args else [],
            "flags": [r.sites, r.vcf, r.cons, r.sam, r.gt], "usage": r.o.usage, "hidden": [r.o.hidden_sort, r.o.hidden_clean],
            "image_arg": r.o.image_arg}
    refusal = msg.value.decode() if msg.value else None
    L.slh_free_options(C.byref(r.o))
    return rc, refusal, vals


def option_rows():
    """The rows of the option table: (name, takes a value)."""
    L = lib()
    rows, name, k = [], C.c_char_p(), 0
    while (v := L.slh_option_info(k, C.byref(name))) >= 0:
        rows.append((name.value.decode(), bool(v)))
        k += 1
    return rows


def pieces(sizes, chunk):
    """slh_next_piece over a merged text of records of these sizes, read in ranges of `chunk` rows: per range the pieces
    (record, a, b, ends_record)."""
    L = lib()
    num = len(sizes)
    recs = (Record * num)(*[Record(b"r%d" % k, s) for k, s in enumerate(sizes)])
    starts, at = [], 0
    for s in sizes:
        starts.append(at)
        at += s + 1
    total = at - 1
    ms = (C.c_uint32 * num)(*starts)
    r, x, p, out = C.c_int(0), C.c_uint64(), Piece(), []
    for x0 in range(0, total, chunk):
        end, got = min(x0 + chunk, total), []
        x.value = x0
        while L.slh_next_piece(recs, ms, num, C.byref(r), C.byref(x), C.c_uint64(end), C.byref(p)):
            assert p.start == starts[p.rec]
            got.append((p.rec, p.a, p.b, p.ends_record))
            assert len(got) <= num
        out.append(got)
    return out


class Buffer(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_char)), ("len", C.c_size_t), ("cap", C.c_size_t)]


_L = None


def lib():
    global _L
    if _L is None:
        so = os.path.join(HOST_DIR, "libslamem_host.so")
        src = os.path.join(HOST_DIR, "slamem_host.c")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["make", "-C", HOST_DIR, "libslamem_host.so"], stdout=subprocess.DEVNULL)
        L = C.CDLL(so)
        L.slh_load_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_int, C.c_long,
                                    C.POINTER(SeqSet), C.c_void_p]
        L.slh_free_seqset.argtypes = [C.POINTER(SeqSet)]
        L.slh_parse_options.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(Options)]
        L.slh_free_options.argtypes = [C.POINTER(Options)]
        L.slh_parse_argument.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
        L.slh_append_to_basename.restype = C.c_void_p
        L.slh_append_to_basename.argtypes = [C.c_char_p, C.c_char_p]
        L.slh_format_block.argtypes = [C.POINTER(Buffer), C.c_char_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(Record),
                                       C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]
        L.slh_buffer_free.argtypes = [C.POINTER(Buffer)]
        L.slh_progress_dots.argtypes = [C.c_uint32]
        L.slh_seq_id_from_merged_pos.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32)]
        _L = L
    return _L


def parse_options(args):
    argv = (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)
    o = Options()
    assert lib().slh_parse_options(len(args), argv, C.byref(o)) == 0
    d = {k: getattr(o, k) for k, _ in Options._fields_ if k != "file_args"}
    d["files"] = [args[o.file_args[i]] for i in range(o.num_files)]
    d["ref_name"] = o.ref_name.decode() if o.ref_name else None
    lib().slh_free_options(C.byref(o))
    return d


class Loaded:
    def __init__(self, path, merge, acgt_only=0, min_len=0, name_filter=None, log_limit=100):
        self.s = SeqSet()
        self.n = lib().slh_load_file(path.encode(), merge, acgt_only, min_len,
                                     name_filter.encode() if name_filter is not None else None, 1, log_limit, C.byref(self.s), None)
        s = self.s
        self.names = [s.recs[i].name for i in range(s.num)]
        self.sizes = [s.recs[i].size for i in range(s.num)]
        self.chars = C.string_at(s.chars, s.total) if self.n else b""
        self.offsets = [s.offsets[i] for i in range(s.num + 1)] if (self.n and not merge) else None
        self.merged_start = [s.merged_start[i] for i in range(s.num)] if (self.n and merge) else None

    def __del__(self):
        lib().slh_free_seqset(C.byref(self.s))


def format_block(name: bytes, reverse: int, mems, ref: Loaded) -> bytes:
    """mems: (count,3) uint32 numpy array of 0-based triples."""
    import numpy as np
    m = np.ascontiguousarray(mems, dtype=np.uint32)
    b = Buffer()
    s = C.c_uint64()
    rc = lib().slh_format_block(C.byref(b), name, reverse, m.ctypes.data, m.shape[0], ref.s.recs, ref.s.merged_start,
                                ref.s.num, C.byref(s))
    assert rc == 0
    out = C.string_at(b.data, b.len)
    lib().slh_buffer_free(C.byref(b))
    return out
