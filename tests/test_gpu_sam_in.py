"""GPU tests (-m gpu) of SAM text in: elp_stage_sam / Engine.stage_sam.

The expected records are tests/samin_ref.py's - formatBamAlignment(parseSamAlignment(line)) restated, pinned by test_samin_ref_cpu.py -
and, for the whole path, the oracle's.  Every comparison is of bytes.

The records of test_gpu_tag_filters._case carry second fields of a key (a second NM, a second X0): elp_stage_sam refuses such a line
(the reference would overwrite the first field in place), and the oracle's encoder writes an XB:B:s field with negative entries, which
the reference refuses to read back, as it does an empty B array (test_samin_ref_cpu.py).  So the cases here are _case's with every
field of a key the record already holds left out, and all records - _case's and test_gpu_sam_out's seam records - go through _readable:
no empty B arrays, the negative entries of B:s arrays made positive.  Hand-written lines cover what no emitter writes."""
import ctypes as C
import struct

import numpy as np
import pytest

import oracle as orc
from elprep_amd.engine import ElpError, Engine
from tests import samin_ref, samref, tagref
from tests.common import dataset
from tests.test_gpu_sam_out import SEAM_NAMES, _device_path, _oracle_path, _seam_case
from tests.test_gpu_tag_filters import _case, _expected_records, _one_group_header

pytestmark = pytest.mark.gpu

ELP_ERR_ARG, ELP_ERR_DATA, ELP_ERR_UNSUPPORTED = -1, -4, -5
TILE = 4096                                                # bytes per workgroup of the line-start kernels


def _readable(rec):
    """the record with the negative entries of its B:s arrays made positive and without empty B arrays: text the reference reads back"""
    out = []
    for key, ty, val in tagref.parse_fields(rec):
        if ty == b"B":
            n = struct.unpack_from("<I", val, 1)[0]
            if n == 0:
                continue                                                  # "B:c" without an entry: refused
            if val[:1] == b"s":
                val = b"s" + struct.pack("<I%dh" % n, n, *[v if v >= 0 else -v - 1 for v in struct.unpack_from("<%dh" % n, val, 5)])
        out.append((key, ty, val))
    return tagref.with_fields(rec, out)


def _unique_case(n_pairs, seed):
    cfg, b, h, refs, sites, extra, _ = _case(n_pairs, seed)
    plain = b"".join(_readable(r) for r in tagref.records(orc.bam_encode(b, h.rg_ids).tobytes()))
    uniq = []
    for rec, fields in zip(tagref.records(plain), extra):
        seen = {k for k, _, _ in tagref.parse_fields(rec)}
        keep = []
        for f in fields:
            if f[0] not in seen:
                seen.add(f[0])
                keep.append(f)
        uniq.append(keep)
    assert sum(len(x) for x in uniq) < sum(len(x) for x in extra)
    return cfg, b, h, refs, sites, uniq, np.frombuffer(tagref.append_fields(plain, uniq), np.uint8)


def _text_of(h, raw):
    """the SAM text elp_emit_sorted_sam writes for BAM-staged records in input order, and their re-encoded BAM records"""
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        e.order_keep(fetch=False)
        return e.emit_sorted_sam().tobytes(), e.emit_sorted_bam().tobytes()
    finally:
        e.close()


# ---- 1. the seams
def _short(length, qname):
    """a line of this many bytes, padded by a Z field"""
    front = qname + b"\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\tpd:Z:"
    assert length >= len(front)
    return front + b"p" * (length - len(front))


def _term(k):
    return b"\r\n" if k % 5 == 2 else b"\n"


def _seam_text():
    b, h, extra = _seam_case()
    names = [nm.encode() for nm in SEAM_NAMES]
    recs = [_readable(r) for r in tagref.records(tagref.append_fields(orc.bam_encode(b, h.rg_ids).tobytes(), extra))]
    lines = [samref.line(r, names)[:-1] for r in recs]
    # short lines of 63 .. 129 bytes in front; the next line is padded so that its newline is the last byte of the first tile: the line
    # behind it starts on residue 0, the long lines behind that start wherever they fall and cross the later tiles' borders
    head = [_short(n, b"s%d" % n) for n in (63, 64, 65, 127, 128, 129)]
    assert [len(x) for x in head] == [63, 64, 65, 127, 128, 129]
    used = sum(len(x) + len(_term(k)) for k, x in enumerate(head))
    head.append(_short(TILE - used - len(_term(len(head))), b"t"))
    assert sum(len(x) + len(_term(k)) for k, x in enumerate(head)) == TILE
    hand = [b"m\t0\tc\t5\t9\t5M5M3I0M\t=\t9\t-3\tacgtN*=\t!!!!!!!\tXs:B:s,40000,65535,0\tXf:B:f,1.5,-0,3.4028235e38,1e-45,nan,+Inf\tXi:i:-2147483648\tXj:i:4294967295\tXa:A::\tXz:Z:",
            b"u\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\t",                        # SEQ * / QUAL *: one base N of quality 9; a tab behind the last field
            b"e\t0\t=\t+7\t0\t\tchr3\t-0\t+1\t\t"]                        # RNAME "=", an empty CIGAR, signs, empty SEQ and QUAL
    all_lines = head + lines + hand
    text = b"".join(ln + _term(k) for k, ln in enumerate(all_lines))
    text = text[:-len(_term(len(all_lines) - 1))]                         # the last line has no newline
    assert 40 <= len(all_lines) <= 50
    starts = np.cumsum([0] + [len(ln) + len(_term(k)) for k, ln in enumerate(all_lines)])[:-1]
    assert TILE in starts and len({int(s) // TILE for s in starts}) >= 3
    return h, names, text, all_lines


@pytest.mark.parametrize("sam_pass", [0, 1, 7])
def test_seams_of_the_line_kernels(sam_pass):
    h, names, text, all_lines = _seam_text()
    assert samin_ref.split_lines(text) == all_lines
    want = samin_ref.records(text, names)
    e = Engine(h, tuning={"sam_pass": sam_pass} if sam_pass else None)
    try:
        e.set_read_group_ids(h.rg_ids)
        for run in ("fresh", "reused"):
            e.stage_sam(text)
            assert e.n == len(want)
            e.order_keep(fetch=False)
            got = tagref.records(e.emit_sorted_bam().tobytes())
            for k, (g, w) in enumerate(zip(got, want)):
                assert g == w, (run, k, all_lines[k][:60])
            assert len(got) == len(want)
            e.reset()
    finally:
        e.close()


# ---- 2. the round trip
@pytest.mark.parametrize("n_pairs,seed", [(150, 3), (4000, 5)])
def test_round_trip(n_pairs, seed):
    cfg, b, h, refs, sites, extra, raw = _unique_case(n_pairs, seed)
    text, bam = _text_of(h, raw)
    assert text.count(b"\n") == b.n
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_sam(np.frombuffer(text, np.uint8))
        assert e.n == b.n
        e.order_keep(fetch=False)
        assert e.emit_sorted_sam().tobytes() == text
        assert e.emit_sorted_bam().tobytes() == bam
    finally:
        e.close()


# ---- 3. the whole path from text
@pytest.mark.parametrize("n_pairs,seed", [(150, 3), (4000, 5)])
def test_whole_path_from_text(n_pairs, seed):
    cfg, b, h, refs, sites, extra, raw = _unique_case(n_pairs, seed)
    text, _ = _text_of(h, raw)
    oflags, operm, oqual = _oracle_path(b, h, refs, sites, "coordinate")
    want = samref.lines(b"".join(_readable(r) for r in _expected_records(b, h.rg_ids, operm, oflags, oqual, extra)), h.ref_names)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_sam(text)
        flags, perm, qual = _device_path(e, h, refs, sites, "coordinate")
        assert np.array_equal(flags, oflags) and np.array_equal(perm, operm) and np.array_equal(qual, oqual)
        assert e.emit_sorted_sam().tobytes() == want
    finally:
        e.close()


# ---- 4. mixed staging and the settings
def test_mixed_staging_with_two_splits_and_sr_records():
    cfg, b, h, refs, sites, extra, raw = _unique_case(150, 3)
    recs = tagref.records(raw.tobytes())
    recs = [tagref.with_fields(r, tagref.parse_fields(r) + [tagref.int_field(b"sr", b"C", 1)]) if k % 7 == 3 else r for k, r in enumerate(recs)]
    tagged = np.asarray([k % 7 == 3 for k in range(len(recs))])
    raw = np.frombuffer(b"".join(recs), np.uint8)
    text, bam = _text_of(h, raw)                                          # (sr-tagged records stay behind: RemoveOptionalReads)
    names = [nm.encode() for nm in h.ref_names]
    lines = [samref.line(r, names) for r in recs]
    assert text == b"".join(ln for ln, t in zip(lines, tagged) if not t)
    half = len(recs) // 2
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(np.frombuffer(b"".join(recs[:half]), np.uint8), split_id=2)
        e.stage_sam(b"".join(lines[half:]), split_id=1)
        assert e.n == len(recs) and e.n_sorted == int((~tagged).sum())
        e.order_keep(fetch=False)
        assert e.emit_sorted_bam().tobytes() == bam
        assert e.emit_sorted_sam().tobytes() == text
        e.order_keep(by_split=True, fetch=False)                          # the text's records carry the smaller split id: they go first
        out = tagref.records(bam)
        first = int((~tagged[:half]).sum())
        assert e.emit_sorted_bam().tobytes() == b"".join(out[first:] + out[:first])
    finally:
        e.close()


def test_replace_read_group_tag_filter_and_strict_filter_on_text():
    cfg, b, h4, refs, sites, extra, raw = _unique_case(600, 10)
    h1 = _one_group_header(h4)
    names = [nm.encode() for nm in h4.ref_names]
    recs = tagref.records(raw.tobytes())
    text = b"".join(samref.line(r, names) for r in recs)
    norm = [tagref.with_fields(r, tagref.normalize(tagref.parse_fields(r))) for r in recs]
    e = Engine(h1)
    try:
        e.set_replace_read_group("new")                                   # no RG look-up: the lines' RG ids are not the header's
        e.stage_sam(text)
        e.order_keep(fetch=False)
        want = [tagref.replace_read_group(r, "new") for r in norm]
        assert e.emit_sorted_bam().tobytes() == b"".join(want)
        f = dict(remove=["XT", "MD", "X0"])
        e.set_tag_filter(**f)
        assert e.emit_sorted_bam().tobytes() == b"".join(tagref.apply_tag_filter(r, **f) for r in want)
        e.set_tag_filter()
        verdict = [tagref.strict_keep(r) for r in recs]
        assert "panics" not in verdict and 0 < verdict.count("reject") < len(recs)
        assert e.filter_exact_strict() == verdict.count("reject")
        e.order_keep(fetch=False)
        assert e.emit_sorted_bam().tobytes() == b"".join(r for r, v in zip(want, verdict) if v == "keep")
    finally:
        e.close()


# ---- 5. refusals
GOOD = [b"a\t0\tchr1\t7\t30\t5M\t=\t9\t2\tACGTA\tIIIII\tNM:i:0", b"b\t16\t*\t0\t0\t*\t*\t0\t0\tAC\tII", b"c\t0\tchr1\t1\t1\t2M\t*\t0\t0\tAC\t!!\tXZ:Z:x"]


def _bad(**kw):
    cols = dict(qname=b"r", flag=b"0", rname=b"chr1", pos=b"7", mapq=b"30", cigar=b"5M", rnext=b"=", pnext=b"9", tlen=b"2", seq=b"ACGTA", qual=b"IIIII", opt=[])
    cols.update(kw)
    return b"\t".join([cols[k] for k in ("qname", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual")] + list(cols["opt"]))


REFUSED = [
    (b"", ELP_ERR_DATA), (b"\t".join([b"x"] * 10), ELP_ERR_DATA), (_bad(flag=b"65536"), ELP_ERR_DATA), (_bad(flag=b"-1"), ELP_ERR_DATA), (_bad(flag=b"+1"), ELP_ERR_DATA),
    (_bad(mapq=b"256"), ELP_ERR_DATA), (_bad(pos=b"2147483648"), ELP_ERR_DATA), (_bad(pos=b"x"), ELP_ERR_DATA), (_bad(pnext=b"1.0"), ELP_ERR_DATA), (_bad(tlen=b""), ELP_ERR_DATA),
    (_bad(cigar=b"5"), ELP_ERR_DATA), (_bad(cigar=b"5Q"), ELP_ERR_DATA), (_bad(cigar=b"M"), ELP_ERR_DATA), (_bad(cigar=b"2147483648M"), ELP_ERR_DATA),
    (_bad(opt=[b"XX:i"]), ELP_ERR_DATA), (_bad(opt=[b"X:i:1"]), ELP_ERR_DATA), (_bad(opt=[b"XXX:i:1"]), ELP_ERR_DATA), (_bad(opt=[b"XX:Q:1"]), ELP_ERR_DATA),
    (_bad(opt=[b"XX:A:ab"]), ELP_ERR_DATA), (_bad(opt=[b"XX:A:"]), ELP_ERR_DATA), (_bad(opt=[b"XX:i:1x"]), ELP_ERR_DATA), (_bad(opt=[b"XX:i:9223372036854775808"]), ELP_ERR_DATA),
    (_bad(opt=[b"XX:B:c"]), ELP_ERR_DATA), (_bad(opt=[b"XX:B:c,"]), ELP_ERR_DATA), (_bad(opt=[b"XX:B:q,1"]), ELP_ERR_DATA), (_bad(opt=[b"XX:B:c,128"]), ELP_ERR_DATA),
    (_bad(opt=[b"XX:B:s,-1"]), ELP_ERR_DATA), (_bad(opt=[b"XX:B:f,1,,2"]), ELP_ERR_DATA), (_bad(opt=[b"XX:f:1e39"]), ELP_ERR_DATA), (_bad(opt=[b"XX:f:abc"]), ELP_ERR_DATA),
    (_bad(opt=[b"", b"XX:i:1"]), ELP_ERR_DATA), (_bad(qname=b"x" * (1 << 20)), ELP_ERR_DATA),
    (_bad(rname=b"nochr"), ELP_ERR_UNSUPPORTED), (_bad(rnext=b"nochr"), ELP_ERR_UNSUPPORTED), (_bad(cigar=b"268435455M1M"), ELP_ERR_UNSUPPORTED),
    (_bad(cigar=b"1M1I" * 32768), ELP_ERR_UNSUPPORTED), (_bad(qual=b"IIII"), ELP_ERR_UNSUPPORTED), (_bad(qname=b"x" * 255), ELP_ERR_UNSUPPORTED),
    (_bad(qname=b"x\0y"), ELP_ERR_UNSUPPORTED), (_bad(opt=[b"XX:i:1", b"YY:i:2", b"XX:Z:a"]), ELP_ERR_UNSUPPORTED), (_bad(opt=[b"XX:i:4294967296"]), ELP_ERR_UNSUPPORTED),
    (_bad(opt=[b"XX:i:-2147483649"]), ELP_ERR_UNSUPPORTED), (_bad(opt=[b"XX:Z:a\0b"]), ELP_ERR_UNSUPPORTED), (_bad(opt=[b"XX:H:1AE3"]), ELP_ERR_UNSUPPORTED),
    (_bad(opt=[b"XX:f:0x1p3"]), ELP_ERR_UNSUPPORTED), (_bad(opt=[b"XX:f:1_0"]), ELP_ERR_UNSUPPORTED), (_bad(opt=[b"XX:B:f,1," + b"1" * 65]), ELP_ERR_UNSUPPORTED),
    (_bad(opt=[b"%c%c:i:1" % (65 + k // 26, 65 + k % 26) for k in range(246)]), ELP_ERR_UNSUPPORTED),
]


def test_one_bad_line_among_good_ones():
    cfg, b, h, refs, sites = dataset("tiny", 150, 3, 0.03)
    names = [nm.encode() for nm in h.ref_names]
    good = [ln.replace(b"chr1", names[0]) for ln in GOOD]
    want = samin_ref.records(b"\n".join(good) + b"\n", names)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        for k, (bad, code) in enumerate(REFUSED):
            bad = bad.replace(b"chr1", names[0])
            with pytest.raises(samin_ref.SamError) as ri:                 # the restatement refuses it, for the same class of reason
                samin_ref.record(bad, names)
            assert ri.value.cls == ("data" if code == ELP_ERR_DATA else "unsupported"), (k, bad[:60])
            at = 1 + k % 3
            lines = good[:at] + [bad] + good[at:]
            before = e.n
            with pytest.raises(ElpError) as ei:
                e.stage_sam(b"\n".join(lines) + b"\n")
            assert ei.value.code == code and "line %d:" % at in str(ei.value), (k, bad[:60], str(ei.value))
            assert e.n == before, (k, bad[:60])
            if k % 8 == 0:                                                # a good call afterwards succeeds
                e.stage_sam(b"\n".join(good) + b"\n")
                assert e.n == before + len(good)
        e.reset()
        e.stage_sam(b"\n".join(good))
        e.order_keep(fetch=False)
        assert e.emit_sorted_bam().tobytes() == b"".join(want)
    finally:
        e.close()


def test_call_level_refusals():
    from tests.test_gpu_replace_dictionary import Case
    cfg, b, h, refs, sites = dataset("tiny", 150, 3, 0.03)
    names = [nm.encode() for nm in h.ref_names]
    text = np.frombuffer(b"\n".join(ln.replace(b"chr1", names[0]) for ln in GOOD[1:]) + b"\n", np.uint8)

    def refused(x, handle=None):
        rc = x.L.elp_stage_sam(x.h if handle is None else handle, C.c_void_p(text.ctypes.data), text.size, 0)
        assert rc == ELP_ERR_ARG, rc

    e = Engine(h)
    try:
        raw_ctx = C.c_void_p()
        assert e.L.elp_create(0, C.byref(raw_ctx)) == 0
        refused(e, raw_ctx)                                               # no header
        e.L.elp_destroy(raw_ctx)
        e.set_read_group_ids(h.rg_ids)
        refused(e)                                                        # no names
        assert "names" in e.L.elp_last_error(e.h).decode()
        e.stage_sam(text)                                                 # (Engine.stage_sam sets the header's names)
        assert e.n == 2
        e.reset()
        e.stage(b)
        refused(e)                                                        # column-staged records
        assert "elp_stage" in e.L.elp_last_error(e.h).decode()
    finally:
        e.close()
    c = Case("one_dropped", n_pairs=300)
    e = Engine(c.h)
    try:
        e.set_read_group_ids(c.h.rg_ids)
        e.stage_bam(orc.bam_encode(c.b, c.h.rg_ids))
        e.set_reference_names()
        e.replace_reference_dictionary(c.map, c.new_h.ref_len)
        e.set_reference_names(c.new_h.ref_names)
        refused(e)                                                        # behind a dictionary replacement
        assert "replaced" in e.L.elp_last_error(e.h).decode()
    finally:
        e.close()
