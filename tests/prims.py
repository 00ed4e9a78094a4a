"""ctypes doors to the primitives of slamem_amd/csrc/prims.h -- TEST INFRASTRUCTURE ONLY (never imported by slamem_amd/).

tests/prims/libprims_shim.so (built by __graft_entry__.build()) holds one extern "C" wrapper per function and links
against the product's libslamem_hip.so, so what runs is the product's own code.  Every wrapper takes raw device pointers,
runs on the null stream, synchronises it, and returns the hipError_t as an int.

`Guarded` is the only way the tests hand memory to a primitive: a torch.uint8 allocation with GUARD bytes of 0xA5 in
front of the payload and GUARD bytes behind it, the payload itself filled with 0xA5 as well, so that a store in front of,
behind, or past the defined length of a buffer is seen afterwards.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "prims", "libprims_shim.so")

HIP_SUCCESS = 0
HIP_ERROR_INVALID_VALUE = 1
GUARD = 256
FILL = 0xA5

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        P, U64, I = C.c_void_p, C.c_uint64, C.c_int
        PB = C.POINTER(C.c_uint64)
        for name, args in (("prims_sort_pairs_u64_u32", [P, PB, P, P, P, P, U64, I, I]),
                           ("prims_exclusive_scan_u32", [P, P, U64, P]),
                           ("prims_scan_max_inclusive_u32", [P, PB, P, P, U64]),
                           ("prims_scan_sum_exclusive_u32_u64", [P, PB, P, P, U64]),
                           ("prims_scan_sum_exclusive_u64", [P, PB, P, P, U64]),
                           ("prims_scan_sum_exclusive_uint4", [P, PB, P, P, U64]),
                           ("prims_select_flagged_u32", [P, PB, P, P, P, P, U64]),
                           ("prims_select_indices_u32", [P, PB, P, P, P, U64])):
            f = getattr(L, name)
            f.restype, f.argtypes = I, args
        L.prims_scan_u32_tmp_words.restype, L.prims_scan_u32_tmp_words.argtypes = U64, [U64]
        _LIB = L
    return _LIB


class Guarded:
    """`nbytes` of device memory between two guards.  data: a numpy array to upload (its bytes become the payload's first)."""

    def __init__(self, nbytes: int, data: np.ndarray | None = None, device="cuda:0"):
        import torch
        self.nbytes = int(nbytes)
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
        if data is not None:
            self.upload(data)

    @classmethod
    def of(cls, data: np.ndarray, device="cuda:0") -> "Guarded":
        return cls(data.nbytes, data, device)

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + GUARD

    def upload(self, data: np.ndarray) -> None:
        import torch
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert raw.shape[0] <= self.nbytes
        if raw.shape[0]:
            self.buf[GUARD:GUARD + raw.shape[0]] = torch.from_numpy(raw.copy()).to(self.buf.device)

    def payload(self, dtype=np.uint8) -> np.ndarray:
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype)

    def guards_intact(self) -> bool:
        import torch
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.nbytes:]])
        return bool((g == FILL).all().item())

    def untouched(self) -> bool:
        """Guards and payload all still hold the fill: nothing was written here."""
        return bool((self.buf == FILL).all().item())


def filled(dtype, count: int = 1) -> np.ndarray:
    """What `count` untouched elements of `dtype` read as."""
    return np.full(count * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).view(dtype)


def tmp_query(fn, *args) -> int:
    """The size call of the two-call convention (tmp == nullptr)."""
    b = C.c_uint64(0)
    rc = fn(None, C.byref(b), *args)
    assert rc == HIP_SUCCESS, f"{fn.__name__} size query: hipError {rc}"
    return int(b.value)


def call(fn, tmp: Guarded, tmp_bytes: int, *args) -> int:
    b = C.c_uint64(tmp_bytes)
    return fn(tmp.ptr, C.byref(b), *args)
