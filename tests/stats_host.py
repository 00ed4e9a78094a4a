"""ctypes door to the -stats parts of libslamem_host.so: the report writer (slh_write_stats) and the option's entry point."""
import ctypes as C
import os

import numpy as np

import hostlib


def _libc():
    return C.CDLL(None)


def write_report(table, path) -> str:
    """slh_write_stats(table, FILE*) into `path`; returns the file's text."""
    L, libc = hostlib.lib(), _libc()
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    L.slh_write_stats.argtypes = [C.c_void_p, C.c_void_p]
    t = np.ascontiguousarray(table, dtype=np.uint64)
    assert t.shape == (3112,)
    f = libc.fopen(os.fsencode(str(path)), b"w")
    assert f
    try:
        assert L.slh_write_stats(t.ctypes.data, f) == 0
    finally:
        assert libc.fclose(f) == 0
    with open(path) as fh:
        return fh.read()


def parse_stats(args) -> int:
    L = hostlib.lib()
    L.slh_parse_stats.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    return L.slh_parse_stats(len(args), hostlib.c_argv(args))
