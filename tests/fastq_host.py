"""ctypes view of the FASTQ side of slamem_amd/host/libslamem_host.so for the CPU tests: slh_load_file_q,
slh_pieces_next_q and slh_parse_min_bq.  hostlib.py has the rest (and the mirror of slh_seqset, which did not grow)."""
import ctypes as C
import os
import tempfile

import hostlib

_DECLARED = False


def lib():
    global _DECLARED
    L = hostlib.lib()
    if not _DECLARED:
        L.slh_load_file_q.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_int, C.c_long, C.POINTER(hostlib.SeqSet),
                                      C.POINTER(C.c_void_p), C.c_void_p]
        L.slh_pieces_open.restype = C.c_void_p
        L.slh_pieces_open.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_long, C.c_long, C.c_void_p]
        L.slh_pieces_next_q.argtypes = [C.c_void_p, C.POINTER(hostlib.SeqSet), C.POINTER(C.c_void_p)]
        L.slh_pieces_close.argtypes = [C.c_void_p]
        L.slh_parse_min_bq.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
        _DECLARED = True
    return L


_LIBC = C.CDLL(None)
_LIBC.fopen.restype = C.c_void_p
_LIBC.fopen.argtypes = [C.c_char_p, C.c_char_p]
_LIBC.fclose.argtypes = [C.c_void_p]
_LIBC.free.argtypes = [C.c_void_p]


def _take(s, quals, n):
    """(names, sizes, chars, offsets, quals bytes or None) of a loaded set; frees it."""
    names = [s.recs[i].name for i in range(s.num)] if n > 0 else []
    sizes = [s.recs[i].size for i in range(s.num)] if n > 0 else []
    chars = C.string_at(s.chars, s.total) if n > 0 else b""
    offsets = [s.offsets[i] for i in range(s.num + 1)] if n > 0 else None
    qb = C.string_at(quals.value, s.total) if (n > 0 and quals.value) else None
    if quals.value:
        _LIBC.free(quals)
    lib().slh_free_seqset(C.byref(s))
    return names, sizes, chars, offsets, qb


class LoadedQ:
    """slh_load_file_q of a path: n, names, sizes, chars, offsets, quals (None when quals_out came back NULL), log (the text the
    loader wrote)."""

    def __init__(self, path, merge=0, acgt_only=0, min_len=0, log_limit=100):
        s, quals = hostlib.SeqSet(), C.c_void_p()
        with tempfile.NamedTemporaryFile() as t:
            f = _LIBC.fopen(t.name.encode(), b"w")
            self.n = lib().slh_load_file_q(os.fsencode(path), merge, acgt_only, min_len, None, 1, log_limit, C.byref(s), C.byref(quals), f)
            _LIBC.fclose(f)
            self.log = open(t.name, "rb").read()
        self.merged_chars = C.string_at(s.chars, s.total) if (merge and self.n > 0) else None
        if merge:
            lib().slh_free_seqset(C.byref(s))
            self.quals = None
            return
        self.names, self.sizes, self.chars, self.offsets, self.quals = _take(s, quals, self.n)


def pieces(path, piece_bytes, acgt_only=0, min_len=0):
    """Every piece of slh_pieces_next_q: a list of (names, sizes, chars, offsets, quals), and the last return value (0 or -1)."""
    L = lib()
    p = L.slh_pieces_open(os.fsencode(path), acgt_only, min_len, 1, 100, piece_bytes, None)
    assert p
    out = []
    while True:
        s, quals = hostlib.SeqSet(), C.c_void_p()
        n = L.slh_pieces_next_q(p, C.byref(s), C.byref(quals))
        if n <= 0:
            break
        out.append(_take(s, quals, n))
    L.slh_pieces_close(p)
    return out, n


def parse_min_bq(args):
    argv = (C.c_char_p * (len(args) + 1))(*[a.encode() for a in args], None)
    out = C.c_int(-7)
    return lib().slh_parse_min_bq(len(args), argv, C.byref(out)), out.value
