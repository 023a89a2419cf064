"""The split emitters' entry points without a GPU: exported, listed, and a NULL context is an error code, not a crash (the argument checks
come in front of any device call).  What the calls write is tests/test_gpu_split_out.py's."""
import ctypes as C

import numpy as np

from elprep_amd import _lib

NEW = ["elp_emit_split_bam", "elp_emit_split_bgzf", "elp_emit_split_sam"]
ELP_ERR_ARG = -1


def test_the_three_entry_points_are_exported_and_listed():
    L = _lib.hip()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.HIP_SYMBOLS, name


def test_the_entry_points_reject_a_null_context_without_a_gpu():
    L = _lib.hip()
    gof = np.ones(3, np.int32)
    off = np.zeros(5, np.uint64)
    n = C.c_uint64(7)
    for name in NEW:
        rc = getattr(L, name)(C.c_void_p(0), C.c_void_p(gof.ctypes.data), 2, 0, C.c_void_p(0), 0, C.c_void_p(off.ctypes.data), C.byref(n))
        assert rc == ELP_ERR_ARG, name
    assert n.value == 7 and not off.any()          # nothing written
