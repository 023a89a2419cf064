"""GPU tests (-m gpu) of the seam between a size query and the real call of the emitters' pass loop (emit_stream, elprep_amd/csrc/emit.hip,
with the pass arithmetic of emit_plan.hpp): what a query (out = NULL) answers against what the call writes, and a buffer one byte short,
in passes of 1 and of 333 records.  BAM records and SAM lines: the query is exact.  BGZF members: the query frames every pass on its own
and is an upper bound (emit_query_bytes); the call carries the bytes behind a pass's last whole member into the next pass."""
import ctypes as C

import numpy as np
import pytest

from elprep_amd.engine import Engine
from tests.test_gpu_round4 import _bam_case, _members
from tests.test_gpu_split_out import _call

pytestmark = pytest.mark.gpu

ELP_ERR_ARG = -1
GOF, N_GROUPS = [1, 1, 2], 2   # the tiny genome's three contigs in two group files (+ the unmapped and the spread file)


def _emit(e, form, fmt, out, cap):
    """the C call itself -> (return code, n_bytes)"""
    if form == "split":
        rc, size, _ = _call(e, fmt, GOF, N_GROUPS, False, out, cap)
        return rc, size
    n = C.c_uint64(12345)
    rc = getattr(e.L, "elp_emit_sorted_" + fmt)(e.h, C.c_void_p(out.ctypes.data if out is not None else 0), cap, C.byref(n))
    return rc, int(n.value)


# (the stored form differs from the compressed one in bgzf_frame alone: one pass size covers it)
CASES = [(per_pass, form, fmt, 0) for per_pass in (1, 333) for form in ("sorted", "split") for fmt in ("bam", "sam", "bgzf")] + [(333, "sorted", "bgzf", 1), (333, "split", "bgzf", 1)]


@pytest.mark.parametrize("per_pass,form,fmt,stored", CASES)
def test_size_query_against_the_call_and_a_buffer_one_byte_short(per_pass, form, fmt, stored):
    """_bam_case()'s 3000 pairs, every record a pass of its own or 333 a pass.  The query's answer is the call's size (BAM, SAM) or at
    least that (BGZF, compressed or stored).  A buffer of the call's size - 1 is refused with "output buffer too small" and status
    ELP_ERR_ARG; the context stays usable: the next call gives the bytes of the first (BGZF members as the device compressed them are
    compared by what they inflate to, stored ones byte by byte)."""
    b, h, raw, rec_off = _bam_case()
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw, rec_off=rec_off)
        e.sort_coordinate()
        if fmt == "sam":
            e._header_names()
        e.set_tuning("bgzf_stored", stored)
        e.set_tuning("emit_pass", per_pass)
        rc, query = _emit(e, form, fmt, None, 0)
        assert rc == 0 and query > 0
        out = np.full(query + 8, 0xAA, np.uint8)
        rc, size = _emit(e, form, fmt, out, query)
        print("%s %s stored=%d per_pass=%d: query %d, call %d" % (form, fmt, stored, per_pass, query, size))
        assert rc == 0 and (out[query:] == 0xAA).all()
        assert query >= size > 0 if fmt == "bgzf" else query == size
        first = out[:size].tobytes()
        short = np.full(query + 8, 0xBB, np.uint8)
        rc, _ = _emit(e, form, fmt, short, size - 1)
        assert rc == ELP_ERR_ARG and b"output buffer too small" in e.L.elp_last_error(e.h)
        again = np.full(query + 8, 0xCC, np.uint8)
        rc, size2 = _emit(e, form, fmt, again, query)
        assert rc == 0 and (again[query:] == 0xCC).all()
        if fmt == "bgzf" and not stored:
            assert [m for _, m in _members(again[:size2].tobytes())] == [m for _, m in _members(first)]
        else:
            assert size2 == size and again[:size].tobytes() == first
        assert b.n > 2 * per_pass  # (several passes)
    finally:
        e.set_tuning("emit_pass", 0)
        e.set_tuning("bgzf_stored", 0)
        e.close()
