"""GPU tests (-m gpu) of SAM text out: elp_set_reference_names_flat, elp_emit_sorted_sam, elp_emit_merged_sam, elp_emit_concat_sam.

The expected bytes are tests/samref.py's lines - FormatAlignment(parseBamAlignment(record)) restated, pinned by test_samref_cpu.py - of
the expected BAM records: the oracle's records (its order, flags and recalibrated qualities) with the appended fields as formatBamTag
writes them, as test_gpu_tag_filters.py builds them; for the two-context forms the records of elp_emit_merged_bam / elp_emit_concat_bam,
which test_gpu_keep_order.py pins.  Every comparison is of bytes."""
import ctypes as C
import struct

import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch, Header, batch_from_records
from elprep_amd.engine import BqsrTables, ElpError, Engine
from tests import samref, tagref
from tests.common import dataset
from tests.test_gpu_tag_filters import NIL16, _case, _expected_records, _names, _one_group_header, _with_rgid
from tests.test_samref_cpu import KAT, SPECIAL

pytestmark = pytest.mark.gpu

ELP_ERR_ARG, ELP_ERR_DATA, ELP_ERR_UNSUPPORTED = -1, -4, -5


def _size_query(e):
    n = C.c_uint64()
    e._check(e.L.elp_emit_sorted_sam(e.h, C.c_void_p(0), 0, C.byref(n)))
    return int(n.value)


def _emit_checked(e):
    """the lines, with the size query equal to the bytes returned"""
    got = e.emit_sorted_sam().tobytes()
    assert _size_query(e) == len(got)
    return got


def _oracle_path(b, h, refs, sites, order):
    oflags = orc.mark_duplicates(b, h)
    if order == "coordinate":
        operm = orc.sort_coordinate(b, oflags)
    elif order == "queryname":
        names = _names(b)
        operm = np.asarray(sorted(range(b.n), key=lambda i: names[i]), dtype=np.uint32)
    else:
        operm = np.arange(b.n, dtype=np.uint32)            # keep: the input's order (no record is tagged sr)
    oq, oc, ox = orc.bqsr_gather(b, h, orc.BqsrRef(refs, sites), oflags, 500)
    return oflags, operm, orc.BqsrFinal(oq, oc, ox, 500).apply(b, h, 0)


def _device_path(e, h, refs, sites, order):
    flags = e.mark_duplicates(True)
    perm = {"coordinate": e.sort_coordinate, "queryname": e.sort_queryname, "keep": e.order_keep}[order]()
    for r in range(h.n_ref):
        e.set_reference(r, refs[r])
        e.set_known_sites(r, sites[r])
    qt, ct, xt = e.recalibrate(500)
    lut, present = BqsrTables(qt, ct, xt, 500).finalize().build_lut(0)
    return flags, perm, e.apply_bqsr(lut, present, 500)


# ---- 1. the whole path
@pytest.mark.parametrize("n_pairs,seed", [(150, 3), (4000, 5)])
@pytest.mark.parametrize("order", ["coordinate", "queryname", "keep"])
def test_whole_path_lines(n_pairs, seed, order):
    cfg, b, h, refs, sites, extra, raw = _case(n_pairs, seed)
    oflags, operm, oqual = _oracle_path(b, h, refs, sites, order)
    want = samref.lines(b"".join(_expected_records(b, h.rg_ids, operm, oflags, oqual, extra)), h.ref_names)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        for run in ("fresh", "reused"):
            e.stage_bam(raw)
            flags, perm, qual = _device_path(e, h, refs, sites, order)
            assert np.array_equal(flags, oflags) and np.array_equal(perm, operm) and np.array_equal(qual, oqual), run
            assert _emit_checked(e) == want, run
            e.reset()                                      # a plain reset keeps the names
    finally:
        e.close()


# ---- 2. the seams of the emit kernel
L_SEQ = [0, 1, 2, 63, 64, 65, 127, 128, 129]
L_QNAME = [1, 63, 64, 65, 254]
N_CIGAR = [0, 1, 63, 64, 65, 200]
OP_LEN = [1, 9, 10, 99999999, 268435455]
COUNTS = [0, 1, 63, 64, 65, 130]
SEAM_NAMES = ["c", "contig_with_a_name_of_seventy_bytes_" + "0123456789" * 3 + "abcd", "chr3"]
REFIDS = [(-1, -1), (0, 0), (1, 1), (0, 1), (1, 0), (2, -1), (-1, 2), (1, 2)]   # refid, next_refid: each -1, equal, different; both name lengths
TLEN = [0, 2147483647, -2147483648, -1, 350]
MIXED = {b"c": [-128, -100, -10, -9, -1, 0, 9, 10, 99, 100, 127], b"C": [0, 9, 10, 99, 100, 255],
         b"s": [-32768, -10000, -1000, -100, -10, -1, 0, 9, 10, 999, 1000, 32767], b"S": [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535],
         b"i": [-2147483648, -1000000000, -999999999, -1, 0, 9, 99999, 100000, 2147483647], b"I": [0, 9, 10, 99999999, 100000000, 999999999, 1000000000, 4294967295]}
FLOAT_BITS = [bits for bits, _ in KAT + SPECIAL]


def _seam_fields():
    """every appended field of the seams test, each once"""
    f = [(b"A", b"q"), (b"A", b"!")]
    for ty, fmt, lo, hi in ((b"c", "<b", -128, 127), (b"C", "<B", 0, 255), (b"s", "<h", -32768, 32767), (b"S", "<H", 0, 65535),
                            (b"i", "<i", -2147483648, 2147483647), (b"I", "<I", 0, 4294967295)):
        f += [(ty, struct.pack(fmt, lo)), (ty, struct.pack(fmt, hi))]
    f += [(b"f", struct.pack("<I", bits)) for bits in FLOAT_BITS]
    f += [(b"Z", bytes(33 + (k * 7) % 90 for k in range(n)) + b"\0") for n in (0, 1, 63, 64, 65, 200)]
    for sub, vals in MIXED.items():
        fmt = {b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I"}[sub]
        f += [(b"B", sub + struct.pack("<I%d%s" % (n, fmt), n, *[vals[(3 * k + n) % len(vals)] for k in range(n)])) for n in COUNTS]
    f += [(b"B", b"f" + struct.pack("<I%dI" % n, n, *[FLOAT_BITS[(5 * k + n) % len(FLOAT_BITS)] for k in range(n)])) for n in COUNTS]
    keys = [bytes([a, d]) for a in b"abcdefghijklmnopqrtuvwxyz" for d in b"0123456789"]   # (no s: sr is the split tag; neither RG nor CG)
    assert len(f) <= len(keys)
    return [(keys[k], ty, val) for k, (ty, val) in enumerate(f)]


def _seam_case():
    rng = np.random.default_rng(11)
    n_rec = 36
    recs = []
    for i in range(n_rec):
        l_seq, lq, nc = L_SEQ[i % len(L_SEQ)], L_QNAME[i % len(L_QNAME)], N_CIGAR[(i // 2) % len(N_CIGAR)]
        refid, nref = REFIDS[i % len(REFIDS)]
        recs.append(dict(qname=bytes(rng.integers(48, 123, lq).astype(np.uint8)), flag=[0, 4, 16, 99, 147, 65535, 1024][i % 7], refid=refid,
                         pos=0 if i % 5 == 0 else 1 + 1000 * i, mapq=[0, 9, 10, 99, 100, 255][i % 6],
                         cigar=[(OP_LEN[(k + i) % len(OP_LEN)] << 4) | ((k + i) % 9) for k in range(nc)], next_refid=nref,
                         pnext=0 if i % 4 == 0 else 7 + 999 * i, tlen=TLEN[i % len(TLEN)],
                         seq="".join("=ACMGRSVTWYHKDBN"[int(c)] for c in rng.integers(0, 16, l_seq)), qual=rng.integers(0, 94, l_seq).astype(np.uint8),
                         rgid=i % 2 if i % 3 else None))
    used = lambda key, vals: set(vals) <= {r[key] if key != "l_seq" else len(r["seq"]) for r in recs}
    assert used("l_seq", L_SEQ) and used("tlen", TLEN) and {len(r["qname"]) for r in recs} == set(L_QNAME) and {len(r["cigar"]) for r in recs} == set(N_CIGAR)
    assert {(r["refid"], r["next_refid"]) for r in recs} == set(REFIDS) and any(r["pos"] == 0 for r in recs) and any(r["pnext"] == 0 for r in recs)
    fields = _seam_fields()
    extra = [fields[i::n_rec] for i in range(n_rec)]
    h = Header.from_read_groups(SEAM_NAMES, [2 ** 31 - 1, 1 << 29, 1 << 20], [{"ID": "g%d" % k, "LB": "lib", "PU": "pu%d" % k} for k in range(2)])
    assert sorted(len(nm) for nm in SEAM_NAMES) == [1, 4, 70]
    return batch_from_records(recs), h, extra


def test_seams_of_the_emit_kernel():
    b, h, extra = _seam_case()
    raw = np.frombuffer(tagref.append_fields(orc.bam_encode(b, h.rg_ids).tobytes(), extra), np.uint8)
    recs = tagref.records(orc.bam_encode(b, h.rg_ids, normalize_tags=True).tobytes())
    want_recs = [tagref.with_fields(r, tagref.parse_fields(r) + tagref.normalize(x)) for r, x in zip(recs, extra)]
    want = [samref.line(r, [nm.encode() for nm in SEAM_NAMES]) for r in want_recs]
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        for run in ("fresh", "reused"):
            e.stage_bam(raw)
            e.order_keep(fetch=False)
            got = _emit_checked(e)
            assert got.count(b"\n") == len(want), run
            for k, (g, w) in enumerate(zip(got.split(b"\n"), want)):
                assert g + b"\n" == w, (run, k)
            assert got == b"".join(want), run
            e.reset()
    finally:
        e.close()


# ---- 3. missing qualities
def test_missing_qualities_leave_as_spaces():
    """a run without BQSR on records whose QUAL bytes are BAM's 0xFF: qual + 33 wraps to a space, as the reference's byte arithmetic does"""
    cfg, b, h, refs, sites = dataset("tiny", 150, 3, 0.03)
    cols = {name: getattr(b, name) for name in b.__dataclass_fields__}
    qual = b.qual.copy()
    lo, hi = b.qual_off[:-1].astype(np.int64), b.qual_off[1:].astype(np.int64)
    for i in range(0, b.n, 3):
        qual[lo[i]:hi[i]] = 0xFF
    cols["qual"] = qual
    bq = Batch(**cols)
    want = samref.lines(orc.bam_encode(bq, h.rg_ids, normalize_tags=True).tobytes(), h.ref_names)
    assert want.count(b"\t" + b" " * 20) >= b.n // 3 - 1
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(orc.bam_encode(bq, h.rg_ids))
        e.order_keep(fetch=False)
        assert _emit_checked(e) == want
    finally:
        e.close()


# ---- 4. the options
@pytest.mark.parametrize("f", [dict(remove=["XT", "MD", "X0"]), dict(keep=["NM", "RG", "XB"]), dict(remove="all")])
def test_tag_filters(f):
    cfg, b, h, refs, sites, extra, raw = _case(150, 3)
    oflags = orc.mark_duplicates(b, h)
    operm = orc.sort_coordinate(b, oflags)
    want0 = _expected_records(b, h.rg_ids, operm, oflags, None, extra)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        e.mark_duplicates(True)
        e.sort_coordinate(fetch=False)
        e.set_tag_filter(**f)
        assert _emit_checked(e) == samref.lines(b"".join(tagref.apply_tag_filter(r, **f) for r in want0), h.ref_names)
        e.set_tag_filter()
        assert _emit_checked(e) == samref.lines(b"".join(want0), h.ref_names)
    finally:
        e.close()


def test_replace_read_group():
    """the first RG field is replaced, a record without one gets RG:Z:<id> behind its last field, a second RG field stays"""
    cfg, b_in, h4, refs, sites, extra, raw = _case(600, 10, batch=lambda b: _with_rgid(b, np.where(b.rgid == 3, NIL16, b.rgid)), second_rg=True)
    h1 = _one_group_header(h4)
    b0 = _with_rgid(b_in, np.zeros(b_in.n, np.uint16))
    oflags = orc.mark_duplicates(b0, h1)
    operm = orc.sort_coordinate(b0, oflags)
    want0 = [tagref.replace_read_group(r, "new") for r in _expected_records(b_in, h4.rg_ids, operm, oflags, None, extra)]
    want = samref.lines(b"".join(want0), h1.ref_names)
    n_rg = [sum(1 for k, _, _ in tagref.parse_fields(r) if k == b"RG") for r in want0]
    assert 2 in n_rg and any(tagref.parse_fields(r)[-1][0] == b"RG" and n == 1 for r, n in zip(want0, n_rg)) and want.count(b"\tRG:Z:zz") > 0
    e = Engine(h1)
    try:
        e.set_replace_read_group("new")
        e.stage_bam(raw)
        assert np.array_equal(e.mark_duplicates(True), oflags) and np.array_equal(e.sort_coordinate(), operm)
        assert _emit_checked(e) == want
        e.set_tag_filter(remove=["RG"])                    # the tag filter acts on the result
        assert _emit_checked(e) == samref.lines(b"".join(tagref.apply_tag_filter(r, remove=["RG"]) for r in want0), h1.ref_names)
    finally:
        e.close()


def test_clean_sam_rewrites_the_cigar_column():
    from oracle import simple_filters as sf
    cfg, b, h, refs, sites = dataset("tiny", 4000, 9, 0.03)
    cut = np.array([41000, 30000, 22000], np.int32)
    clip = np.clip(b.refid, 0, None)
    sel = np.nonzero((b.refid < 0) | (b.pos <= cut[clip] - 20))[0]    # some alignments hang over the new end, none starts behind it
    bb = b.take(sel)
    h2 = Header(ref_len=cut, rg_lib=h.rg_lib, rg_cov=h.rg_cov, ref_names=h.ref_names, rg_ids=h.rg_ids, lib_names=h.lib_names, cov_names=h.cov_names)
    cleaned, n_changed = sf.clean_sam(bb, cut)
    assert n_changed > 5 and not np.array_equal(cleaned.cigar, bb.cigar)
    want = samref.lines(orc.bam_encode(cleaned, h2.rg_ids, normalize_tags=True).tobytes(), h2.ref_names)
    e = Engine(h2)
    try:
        e.set_read_group_ids(h2.rg_ids)
        e.stage_bam(orc.bam_encode(bb, h2.rg_ids))
        assert e.clean_sam() == n_changed
        e.order_keep(fetch=False)
        assert _emit_checked(e) == want
    finally:
        e.close()


def test_replaced_dictionary_needs_and_writes_the_new_names():
    from tests.test_gpu_replace_dictionary import Case, _full_flags_qual
    c = Case("one_dropped", n_pairs=600)
    oflags = orc.mark_duplicates(c.prepared, c.new_h)
    operm = orc.sort_coordinate(c.prepared, oflags)
    full_flags, _, _ = _full_flags_qual(c, oflags, None)
    want = samref.lines(orc.bam_encode(c.full, c.h.rg_ids, order=c.kept[operm], flags=full_flags, normalize_tags=True).tobytes(), c.new_h.ref_names)
    mate_left = (c.b.next_refid[c.kept] >= 0) & (c.full.next_refid[c.kept] < 0)
    assert mate_left.sum() > 0
    e = Engine(c.h)
    try:
        e.set_read_group_ids(c.h.rg_ids)
        e.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
        e.set_reference_names()                            # the header's names ...
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        e.mark_duplicates(True)
        e.sort_coordinate(fetch=False)
        with pytest.raises(ElpError) as ei:                # ... left with its dictionary
            e.emit_sorted_sam()
        assert ei.value.code == ELP_ERR_ARG
        e.set_reference_names(c.new_h.ref_names)
        got = _emit_checked(e)
        assert got == want
        cols = [ln.split(b"\t") for ln in got.split(b"\n")[:-1]]
        assert sum(1 for x, left in zip(cols, mate_left[operm]) if left and x[6] == b"*") == int(mate_left.sum())
        e.reset()                                          # undoes the replacement: the new names leave with it
        e.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
        e.order_keep(fetch=False)
        with pytest.raises(ElpError) as ei:
            n = C.c_uint64()
            e._check(e.L.elp_emit_sorted_sam(e.h, C.c_void_p(0), 0, C.byref(n)))
        assert ei.value.code == ELP_ERR_ARG
        assert _emit_checked(e) == samref.lines(orc.bam_encode(c.b, c.h.rg_ids, normalize_tags=True).tobytes(), c.h.ref_names)   # (emit_sorted_sam sets the header's)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["one_dropped", "reversed", "two_in_front"])
def test_replaced_dictionary_never_goes_out_under_the_headers_names(name):
    """names never set before the replacement, a new dictionary with fewer, as many and more contigs than the header's: the emitters do
    not fall back to the header's names (the old contigs'), the call returns ELP_ERR_ARG; a list of another length than the dictionary
    in force never reaches the C call, which is told no count"""
    from tests.test_gpu_replace_dictionary import Case
    c = Case(name, n_pairs=300)
    assert (c.new_h.n_ref < c.h.n_ref, c.new_h.n_ref == c.h.n_ref, c.new_h.n_ref > c.h.n_ref) == (name == "one_dropped", name == "reversed", name == "two_in_front")
    e, other = Engine(c.h), Engine(c.h)
    try:
        for x in (e, other):
            x.set_read_group_ids(c.h.rg_ids)
            x.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
            x.replace_reference_dictionary(c.map, c.new_h.ref_len)
            x.order_keep(fetch=False)
        for call in (e.emit_sorted_sam, lambda: e.emit_merged_sam(other)):
            with pytest.raises(ElpError) as ei:
                call()
            assert ei.value.code == ELP_ERR_ARG and "names" in str(ei.value)
        with pytest.raises(ElpError) as ei:
            e.set_reference_names()                        # the header's names are the old contigs'
        assert ei.value.code == ELP_ERR_ARG
        for bad in (list(c.new_h.ref_names) + ["one_more"], list(c.new_h.ref_names)[:-1]):
            with pytest.raises(ElpError) as ei:
                e.set_reference_names(bad)
            assert ei.value.code == ELP_ERR_ARG and "contigs" in str(ei.value)
        with pytest.raises(ElpError):
            e.emit_sorted_sam()                            # a refused call set nothing
        e.set_reference_names(c.new_h.ref_names)
        want = samref.lines(orc.bam_encode(c.full, c.h.rg_ids, order=c.kept, normalize_tags=True).tobytes(), c.new_h.ref_names)
        assert _emit_checked(e) == want
    finally:
        e.close()
        other.close()


def test_next_refid_outside_the_dictionary_is_reported():
    """staging checks refid alone: a mate on a contig the dictionary does not hold is found by the size pass, before a name is read"""
    cfg, b, h, refs, sites = dataset("tiny", 150, 3, 0.03)
    for beyond in (h.n_ref, h.n_ref + 4, 2 ** 31 - 1):
        recs = tagref.records(orc.bam_encode(b, h.rg_ids).tobytes())
        recs[7] = recs[7][:24] + struct.pack("<i", beyond) + recs[7][28:]
        e = Engine(h)
        try:
            e.set_read_group_ids(h.rg_ids)
            e.stage_bam(np.frombuffer(b"".join(recs), np.uint8))
            e.order_keep(fetch=False)
            with pytest.raises(ElpError) as ei:
                e.emit_sorted_sam()
            assert ei.value.code == ELP_ERR_DATA and "next_refid" in str(ei.value), beyond
        finally:
            e.close()


# ---- 5. passes
def test_passes_of_97_records_give_the_same_bytes():
    cfg, b, h, refs, sites, extra, raw = _case(4000, 5)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        e.sort_coordinate(fetch=False)
        one = _emit_checked(e)
        assert one == samref.lines(b"".join(_expected_records(b, h.rg_ids, orc.sort_coordinate(b), None, None, extra)), h.ref_names)
        e.set_tuning("emit_pass", 97)
        assert _emit_checked(e) == one
    finally:
        e.set_tuning("emit_pass", 0)
        e.close()


# ---- 6. two contexts
def _two(fn, eg, es):
    n = C.c_uint64()
    eg._check(fn(eg.h, es.h, C.c_void_p(0), 0, C.byref(n)))
    out = np.empty(int(n.value), np.uint8)
    eg._check(fn(eg.h, es.h, C.c_void_p(out.ctypes.data), out.size, C.byref(n)))
    assert int(n.value) == out.size                        # the size query is exact
    return out.tobytes()


def test_merged_stream_lines():
    from tests.test_gpu_keep_order import _sorted_case, _split_on_device
    h, b, gof, n_groups, split, spread = _sorted_case()
    eg, es = _split_on_device(h, b, gof, n_groups)
    try:
        for order in ("keep", "coordinate"):
            for e in (eg, es):
                (e.order_keep if order == "keep" else e.sort_coordinate)(fetch=False)
            want = samref.lines(eg.emit_merged_bam(es).tobytes(), h.ref_names)
            assert want.count(b"\n") == b.n
            assert eg.emit_merged_sam(es).tobytes() == want, order
            assert _two(eg.L.elp_emit_merged_sam, eg, es) == want, order
        eg.set_tuning("emit_pass", 97)
        assert eg.emit_merged_sam(es).tobytes() == want
        eg.set_tuning("emit_pass", 0)
        es.set_reference_names([nm + "x" for nm in h.ref_names])     # unequal names
        with pytest.raises(ElpError) as ei:
            eg.emit_merged_sam(es)
        assert ei.value.code == ELP_ERR_ARG
        es.set_reference_names()
        eg.set_tag_filter(remove=["NM"])                   # the rules of elp_emit_merged_bam hold: the filters differ
        with pytest.raises(ElpError) as ei:
            eg.emit_merged_sam(es)
        assert ei.value.code == ELP_ERR_ARG
    finally:
        eg.set_tuning("emit_pass", 0)
        eg.close()
        es.close()


def test_concat_stream_lines():
    from tests.test_gpu_keep_order import _stage_unsorted, _unsorted_case
    h, b, files, spread, want_bam = _unsorted_case()
    eg, es = _stage_unsorted(h, b, files, spread)
    try:
        with pytest.raises(ElpError) as ei:                # no permutation: elp_emit_concat_bam's rule
            eg.emit_concat_sam(es)
        assert ei.value.code == ELP_ERR_ARG
        eg.order_keep(by_split=True, fetch=False)
        es.order_keep(fetch=False)
        assert eg.emit_concat_bam(es).tobytes() == want_bam
        want = samref.lines(want_bam, h.ref_names)
        assert eg.emit_concat_sam(es).tobytes() == want
        assert _two(eg.L.elp_emit_concat_sam, eg, es) == want
        es.set_reference_names(list(h.ref_names[:-1]) + ["other"])
        with pytest.raises(ElpError) as ei:
            eg.emit_concat_sam(es)
        assert ei.value.code == ELP_ERR_ARG
    finally:
        eg.close()
        es.close()


def test_sfm_merged_emit_takes_the_format():
    """sfm.SfmRank.emit_merged / sfm.emit_merged_device with fmt="sam": the lines of the records fmt="bam" gives; another fmt is refused"""
    from elprep_amd import sfm
    from tests.test_gpu_keep_order import _sorted_case
    h, b, gof, n_groups, split, spread = _sorted_case()
    owner = np.zeros(n_groups + 2, np.int32)
    rk = sfm.SfmRank(h, 0, sfm.Comm())
    try:
        raw = orc.bam_encode(b, h.rg_ids)
        for e in rk.engines:
            e.set_read_group_ids(h.rg_ids)
        rk.route(b, gof, n_groups, owner, stage=lambda e, x: e.stage_bam(raw))
        for order in ("keep", "coordinate"):
            for e in rk.engines:
                sfm._order_call(e, order)(False)
            bam = rk.emit_merged(gof, n_groups, owner, order).tobytes()
            assert len(tagref.records(bam)) == b.n
            assert rk.emit_merged(gof, n_groups, owner, order, fmt="sam").tobytes() == samref.lines(bam, h.ref_names), order
            assert rk.emit_merged(gof, n_groups, owner, order, fmt="bam").tobytes() == bam
        with pytest.raises(ValueError):
            rk.emit_merged(gof, n_groups, owner, "keep", fmt="cram")
    finally:
        rk.close()


# ---- 7. errors
def _flat(names):
    enc = [nm.encode() for nm in names]
    return np.frombuffer(b"".join(enc) + b"\0", np.uint8), np.cumsum([0] + [len(x) for x in enc]).astype(np.uint32)


def test_errors():
    cfg, b, h, refs, sites = dataset("tiny", 150, 3, 0.03)
    raw = orc.bam_encode(b, h.rg_ids)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        n = C.c_uint64()
        query = lambda: e.L.elp_emit_sorted_sam(e.h, C.c_void_p(0), 0, C.byref(n))
        e.order_keep(fetch=False)
        assert query() == ELP_ERR_ARG and b"names" in e.L.elp_last_error(e.h)          # no names
        # the setter
        setter = lambda names, off: e.L.elp_set_reference_names_flat(e.h, C.c_void_p(names.ctypes.data), C.c_void_p(off.ctypes.data))
        for bad in (["chrA", "chrB", "chrA"], ["chrA", "", "chrC"], ["chrA", "*", "chrC"], ["=", "chrB", "chrC"]):
            assert setter(*_flat(bad)) == ELP_ERR_ARG, bad
        cat, off = _flat(h.ref_names)
        assert setter(cat, off[::-1].copy()) == ELP_ERR_ARG                              # offsets that decrease
        assert e.L.elp_set_reference_names_flat(e.h, C.c_void_p(0), C.c_void_p(off.ctypes.data)) == ELP_ERR_ARG
        assert e.L.elp_set_reference_names_flat(e.h, C.c_void_p(cat.ctypes.data), C.c_void_p(0)) == ELP_ERR_ARG
        assert query() == ELP_ERR_ARG                                                   # a refused call sets nothing
        assert setter(cat, off) == 0
        assert query() == 0
        size = int(n.value)
        # cap one byte short
        out = np.empty(size, np.uint8)
        assert e.L.elp_emit_sorted_sam(e.h, C.c_void_p(out.ctypes.data), size - 1, C.byref(n)) == ELP_ERR_ARG
        assert e.L.elp_emit_sorted_sam(e.h, C.c_void_p(out.ctypes.data), size, C.byref(n)) == 0 and int(n.value) == size
        assert out.tobytes() == samref.lines(orc.bam_encode(b, h.rg_ids, normalize_tags=True).tobytes(), h.ref_names)
        # no permutation
        e.reset()
        e.stage_bam(raw)
        assert query() == ELP_ERR_ARG
        # column-staged records
        e.reset()
        e.stage(b)
        e.order_keep(fetch=False)
        assert query() == ELP_ERR_ARG and b"elp_stage_bam" in e.L.elp_last_error(e.h)
        # an H field
        e.reset()
        recs = tagref.records(raw.tobytes())
        recs[5] = tagref.with_fields(recs[5], tagref.parse_fields(recs[5]) + [(b"XH", b"H", b"1AE3\0")])
        e.stage_bam(np.frombuffer(b"".join(recs), np.uint8))
        e.order_keep(fetch=False)
        assert query() == ELP_ERR_UNSUPPORTED
        # zero output records
        e.reset()
        e.order_keep(fetch=False)
        assert query() == 0 and int(n.value) == 0
        assert e.emit_sorted_sam().size == 0
    finally:
        e.close()
    e = Engine(h)
    try:
        hdr_less = C.c_void_p()
        assert e.L.elp_create(0, C.byref(hdr_less)) == 0
        cat, off = _flat(h.ref_names)
        assert e.L.elp_set_reference_names_flat(hdr_less, C.c_void_p(cat.ctypes.data), C.c_void_p(off.ctypes.data)) == ELP_ERR_ARG   # no header
        e.L.elp_destroy(hdr_less)
    finally:
        e.close()
