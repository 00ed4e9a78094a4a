"""A ctypes door to the list filters behind K9 (-mum, -smem, -chain) -- TEST INFRASTRUCTURE ONLY (never imported by slamem_amd/).

tests/filters/libfilters_shim.so (built by __graft_entry__.build()) links against the product's libslamem_hip.so and reaches a
filter the way the search does (filter_for, resolve_filter_params, workspace_bytes, filter_list_buffers, run, finish), on a -mem
list the test GIVES it instead of one a search emitted.  The three filters read neither index nor reads: they are integer
functions of (rows, block offsets, parameters), so the comparison with tests/chain_spec.py, smem_spec.py and mum_spec.py is exact.

Every buffer is a prims.Guarded: out_rows is exactly `capacity` rows, out_boff exactly num_blocks + 1 words, the score column
exactly num_blocks words; run() checks every guard, the return code, and that no output row beyond the kept ones was written.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

import prims

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "filters", "libfilters_shim.so")

MUM, SMEM, CHAIN = 2, 3, 4  # the match types of filter_for()
SLAMEM_OK = 0
ROW = 12  # bytes of a slamem_mem: ref_pos, query_pos, length

Result = collections.namedtuple("Result", "rows boff column scalars total")

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        P, U64, U32, I = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.filters_workspace_bytes.restype, L.filters_workspace_bytes.argtypes = U64, [I, U64, U64, U32, U32]
        L.filters_run.restype = I
        L.filters_run.argtypes = [I, P, P, U64, U64, U64, U32, U32, P, P, P, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint64)]
        _LIB = L
    return _LIB


def workspace_bytes(match_type: int, num_blocks: int, capacity: int, max_occ: int = 0, max_gap: int = 0) -> int:
    return int(lib().filters_workspace_bytes(match_type, num_blocks, capacity, max_occ, max_gap))


def run(match_type: int, tri, boff, capacity: int | None = None, max_occ: int = 0, max_gap: int = 0) -> Result:
    """tri: (n, 3) rows (ref_pos, query_pos, length), each below 2^32; boff: num_blocks + 1 offsets into them.
    Returns (kept rows as (k, 3) int64, new offsets as int64, the uint32 per block of -chain or None, the two scalars run()
    sent to the host, the rows kept -- -mum: after finish())."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    assert tri.size == 0 or (tri.min() >= 0 and tri.max() <= 0xFFFFFFFF)
    boff = np.asarray(boff, dtype=np.uint64)
    n, nb = tri.shape[0], boff.shape[0] - 1
    capacity = n if capacity is None else int(capacity)
    assert nb >= 0 and capacity >= n and int(boff[-1]) == n
    rows_in = prims.Guarded.of(tri.astype(np.uint32))
    boff_in = prims.Guarded.of(boff)
    out_rows = prims.Guarded(ROW * capacity)
    out_boff = prims.Guarded(8 * (nb + 1))
    column = prims.Guarded(4 * nb) if match_type == CHAIN else None
    scal = (C.c_ulonglong * 2)(0, 0)
    total = C.c_uint64(0)
    rc = lib().filters_run(match_type, rows_in.ptr, boff_in.ptr, n, nb, capacity, max_occ, max_gap, out_rows.ptr, out_boff.ptr,
                           column.ptr if column else None, scal, C.byref(total))
    assert rc == SLAMEM_OK, f"filters_run({match_type}): code {rc} (1000 + n: hipError n of the door's own calls)"
    for name, b in (("rows", rows_in), ("block offsets", boff_in), ("out_rows", out_rows), ("out_boff", out_boff), ("column", column)):
        assert b is None or b.guards_intact(), f"guard bytes of {name} were overwritten"
    assert np.array_equal(rows_in.payload(np.uint32).reshape(-1, 3), tri.astype(np.uint32)), "the input rows were changed"
    kept = int(total.value)
    assert kept <= capacity
    raw = out_rows.payload(np.uint32).reshape(-1, 3)
    assert np.array_equal(raw[kept:].reshape(-1), prims.filled(np.uint32, 3 * (capacity - kept))), "rows written behind the kept ones"
    return Result(raw[:kept].astype(np.int64), out_boff.payload(np.uint64).astype(np.int64),
                  column.payload(np.uint32).copy() if column else None, (int(scal[0]), int(scal[1])), kept)
