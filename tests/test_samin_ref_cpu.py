"""CPU tests that pin tests/samin_ref.py, the restatement of formatBamAlignment(parseSamAlignment(line)) the GPU tests of elp_stage_sam
compare against: hand-written lines and the records they must give - worked out from sam/sam-files.go:186-410 by hand, not computed -,
the refusals, and the round trip through tests/samref.py (the other direction, pinned by test_samref_cpu.py): for the records the
seam case of test_gpu_sam_out.py and test_gpu_tag_filters._case(150, 3) build, samin_ref.record(samref.line(record)) is the record as
elp_emit_sorted_bam re-encodes it.

Exceptions to the round trip, as the reference has them: a B array without entries prints as "B:c", which parseSamNumericArray refuses
("missing entry in numeric array"); a negative entry of a B:s array prints as "-1", which its ParseUint(.., 16) refuses
(sam/sam-files.go:263-272) - the test expects the refusal for those records; a second field of a key, which SmallMap.Set would write
over the first, is refused by elp_stage_sam (expected too); NaN payloads come back as the canonical NaN."""
import struct

import pytest

import oracle as orc
from tests import samin_ref, samref, tagref
from tests.test_samref_cpu import NAMES, f32, op, record

ERR = samin_ref.SamError


def _line(**kw):
    cols = dict(qname=b"r", flag=b"0", rname=b"chr1", pos=b"7", mapq=b"30", cigar=b"5M", rnext=b"=", pnext=b"9", tlen=b"2", seq=b"ACGTA", qual=b"IIIII", opt=[])
    cols.update(kw)
    return b"\t".join([cols[k] for k in ("qname", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual")] + list(cols["opt"]))


def _bin(rec):
    return struct.unpack_from("<H", rec, 14)[0]


def _with_bin(rec, b):
    return rec[:14] + struct.pack("<H", b) + rec[16:]


# ---- hand-derived lines
def test_a_plain_line():
    """POS 7 -> pos 6; RNEXT "=" takes RNAME's refid; PNEXT 9 -> 8; bases A C G T A = nibbles 1 2 4 8 1; 'I' - 33 = 40; NM:i:0 as C;
    bin of [6, 11): both ends in the same 16 kb window -> 4681 + 0"""
    got = samin_ref.record(_line(opt=[b"NM:i:0"]), NAMES)
    want = record(b"r", 0, 0, 6, 30, [op(5, b"M")], 0, 8, 2, [1, 2, 4, 8, 1], [40] * 5, [(b"NM", b"C", b"\0")])
    assert got == _with_bin(want, 4681)


def test_cigar_merge_star_and_lower_case():
    got = samin_ref.record(_line(cigar=b"5M5M", seq=b"ACGTACGTAC", qual=b"!" * 10), NAMES)
    assert got == _with_bin(record(b"r", 0, 0, 6, 30, [op(10, b"M")], 0, 8, 2, [1, 2, 4, 8, 1, 2, 4, 8, 1, 2], [0] * 10), 4681)
    got = samin_ref.record(_line(cigar=b"*", rname=b"*", rnext=b"*", pos=b"0", pnext=b"0", flag=b"4", seq=b"*", qual=b"*"), NAMES)
    # SEQ "*" is one base N, QUAL "*" one quality of 42 - 33 = 9; POS 0 -> pos -1: bin(-1, -1) = 4681 + (-1 >> 14) = 4680 (unmapped: end = beg)
    assert got == _with_bin(record(b"r", 4, -1, -1, 30, [], -1, -1, 2, [15], [9]), 4680)
    got = samin_ref.record(_line(seq=b"acgtn", cigar=b"2m3x"), NAMES)
    assert got == _with_bin(record(b"r", 0, 0, 6, 30, [op(2, b"M"), op(3, b"X")], 0, 8, 2, [15] * 5, [40] * 5), 4681)


def test_names_and_numbers():
    got = samin_ref.record(_line(rname=b"c", rnext=b"chr1", pos=b"+1", pnext=b"-5", tlen=b"-2147483648", flag=b"65535", mapq=b"255"), NAMES)
    assert got == _with_bin(record(b"r", 65535, 1, 0, 255, [op(5, b"M")], 0, -6, -2147483648, [1, 2, 4, 8, 1], [40] * 5), 4681)   # (unmapped bit set: end = beg)
    got = samin_ref.record(_line(rname=b"=", rnext=b"="), NAMES)                  # RNAME "=" is no contig: -1, which RNEXT "=" takes
    assert struct.unpack_from("<i", got, 4)[0] == -1 and struct.unpack_from("<i", got, 24)[0] == -1
    got = samin_ref.record(_line(pos=b"-2147483648"), NAMES)                      # POS - 1 wraps
    assert struct.unpack_from("<i", got, 8)[0] == 2147483647
    got = samin_ref.record(_line(pos=b"16380", cigar=b"10M"), NAMES)              # [16379, 16389) crosses 2^14: the 128 kb level, 585 + 0
    assert _bin(got) == 585


def test_optional_fields_of_every_type():
    opt = [b"Xa:A:!", b"Xb:i:-128", b"Xc:i:-129", b"Xd:i:-32769", b"Xe:i:255", b"Xf:i:256", b"Xg:i:65536", b"Xh:i:+7", b"Xi:f:1.5", b"Xj:f:-0", b"Xk:Z:a b:c", b"Xl:Z:",
           b"Xm:B:c,-1,2", b"Xn:B:C,255", b"Xo:B:s,40000,0", b"Xp:B:S,65535", b"Xq:B:i,-2147483648", b"Xr:B:I,4294967295", b"Xs:B:f,1,nan,-inf"]
    want = [(b"Xa", b"A", b"!"), (b"Xb", b"c", b"\x80"), (b"Xc", b"s", struct.pack("<h", -129)), (b"Xd", b"i", struct.pack("<i", -32769)), (b"Xe", b"C", b"\xff"),
            (b"Xf", b"S", struct.pack("<H", 256)), (b"Xg", b"I", struct.pack("<I", 65536)), (b"Xh", b"C", b"\x07"), (b"Xi", b"f", struct.pack("<f", 1.5)),
            (b"Xj", b"f", struct.pack("<I", 0x80000000)), (b"Xk", b"Z", b"a b:c\0"), (b"Xl", b"Z", b"\0"), (b"Xm", b"B", b"c" + struct.pack("<Ibb", 2, -1, 2)),
            (b"Xn", b"B", b"C" + struct.pack("<IB", 1, 255)), (b"Xo", b"B", b"s" + struct.pack("<Ihh", 2, -25536, 0)), (b"Xp", b"B", b"S" + struct.pack("<IH", 1, 65535)),
            (b"Xq", b"B", b"i" + struct.pack("<Ii", 1, -2147483648)), (b"Xr", b"B", b"I" + struct.pack("<II", 1, 4294967295)),
            (b"Xs", b"B", b"f" + struct.pack("<IIII", 3, f32(1.0), 0x7FC00000, 0xFF800000))]
    got = samin_ref.record(_line(opt=opt), NAMES)
    assert tagref.parse_fields(got) == want
    assert samin_ref.record(_line(opt=opt) + b"\t", NAMES) == got                 # a tab behind the last field ends the line


def test_lines_of_a_text():
    assert samin_ref.split_lines(b"a\r\nb\n\nc\r") == [b"a", b"b", b"", b"c"] and samin_ref.split_lines(b"a\n") == [b"a"] and samin_ref.split_lines(b"") == []
    assert samin_ref.split_lines(b"a\r\r\n") == [b"a\r"]


@pytest.mark.parametrize("line,cls", [
    (b"", "data"), (b"\t".join([b"x"] * 10), "data"), (_line(flag=b"+1"), "data"), (_line(mapq=b"256"), "data"), (_line(pos=b"2147483648"), "data"),
    (_line(cigar=b"5"), "data"), (_line(cigar=b"M"), "data"), (_line(cigar=b"5Q"), "data"), (_line(cigar=b"2147483648M"), "data"),
    (_line(opt=[b"XX:i"]), "data"), (_line(opt=[b"X:i:1"]), "data"), (_line(opt=[b"XX:Q:1"]), "data"), (_line(opt=[b"XX:A:ab"]), "data"), (_line(opt=[b"XX:B:c"]), "data"),
    (_line(opt=[b"XX:B:c,"]), "data"), (_line(opt=[b"XX:B:s,-1"]), "data"), (_line(opt=[b"XX:B:q,1"]), "data"), (_line(opt=[b"XX:f:1e39"]), "data"),
    (_line(rname=b"nochr"), "unsupported"), (_line(rnext=b"nochr"), "unsupported"), (_line(cigar=b"268435455M1M"), "unsupported"), (_line(cigar=b"1M1I" * 32768), "unsupported"),
    (_line(qual=b"IIII"), "unsupported"), (_line(qname=b"x" * 255), "unsupported"), (_line(qname=b"x\0"), "unsupported"), (_line(opt=[b"XX:i:1", b"XX:i:1"]), "unsupported"),
    (_line(opt=[b"XX:i:4294967296"]), "unsupported"), (_line(opt=[b"XX:Z:\0"]), "unsupported"), (_line(opt=[b"XX:H:00"]), "unsupported"), (_line(opt=[b"XX:f:0x1p3"]), "unsupported"),
])
def test_refusals(line, cls):
    with pytest.raises(ERR) as ei:
        samin_ref.record(line, NAMES)
    assert ei.value.cls == cls


# ---- the round trip through samref
def _normal(rec):
    """the record as elp_emit_sorted_bam re-encodes it: integers in the smallest type, NaNs as they are - made canonical here, as text has one NaN"""
    out = []
    for key, ty, val in tagref.normalize(tagref.parse_fields(rec)):
        if ty == b"f" or (ty == b"B" and val[:1] == b"f"):
            head, words = (b"", struct.unpack("<I", val)) if ty == b"f" else (val[:5], struct.unpack_from("<%dI" % struct.unpack_from("<I", val, 1)[0], val, 5))
            val = head + b"".join(struct.pack("<I", 0x7FC00000 if (w & 0x7FFFFFFF) > 0x7F800000 else w) for w in words)
        out.append((key, ty, val))
    return tagref.with_fields(rec, out)


def _round_trip(recs, names):
    n_refused = 0
    for k, rec in enumerate(recs):
        fields = tagref.parse_fields(rec)
        empty_b = any(ty == b"B" and struct.unpack_from("<I", val, 1)[0] == 0 for _, ty, val in fields)
        negative_s = any(ty == b"B" and val[:1] == b"s" and min(struct.unpack_from("<%dh" % struct.unpack_from("<I", val, 1)[0], val, 5), default=0) < 0 for _, ty, val in fields)
        twice = len({key for key, _, _ in fields}) != len(fields)
        line = samref.line(rec, names)
        assert line.endswith(b"\n")
        if empty_b or negative_s or twice:
            with pytest.raises(ERR) as ei:
                samin_ref.record(line[:-1], names)
            assert ei.value.cls == ("data" if empty_b or negative_s else "unsupported"), k
            n_refused += 1
            continue
        got = samin_ref.record(line[:-1], names)
        want = _normal(rec)
        assert got[:14] == want[:14] and got[16:] == want[16:], k        # (the oracle's encoder and the bin field: test_gpu_cigar_ops.py)
        assert _bin(got) == _bin(want), k
    return n_refused


def test_round_trip_of_the_seam_records():
    from tests.test_gpu_sam_out import SEAM_NAMES, _seam_case
    b, h, extra = _seam_case()
    recs = tagref.records(tagref.append_fields(orc.bam_encode(b, h.rg_ids).tobytes(), extra))
    refused = _round_trip(recs, [nm.encode() for nm in SEAM_NAMES])
    assert 0 < refused < len(recs)


def test_round_trip_of_the_tag_filter_case():
    from tests.test_gpu_tag_filters import _case
    cfg, b, h, refs, sites, extra, raw = _case(150, 3)
    recs = tagref.records(raw.tobytes())
    refused = _round_trip(recs, [nm.encode() for nm in h.ref_names])
    assert 0 < refused < len(recs)
