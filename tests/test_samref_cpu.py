"""CPU tests that pin tests/samref.py, the restatement of FormatAlignment(parseBamAlignment(record)) the GPU tests of the SAM emitters
compare against: hand-written records and the lines they must give, the float form's known answers (Go's
strconv.AppendFloat(float64(v), 'g', -1, 32), stated from its definition), and the float digits against numpy's shortest-unique digits.

The hand-written lines are worked out from sam/sam-files.go:485-598 by hand, not computed: a record is built field by field below and
its line is spelled out beside it."""
import struct

import numpy as np
import pytest

from tests import samref, tagref

NAMES = [b"chr1", b"c", b"chrUn_KI270302v1_with_a_name_of_seventy_bytes_012345678901234567890123"]
assert len(NAMES[2]) == 70


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def record(qname, flag, refid, pos0, mapq, cigar, nref, pnext0, tlen, seq_nibbles, qual, fields=()):
    """a BAM record (block_size in front); cigar = uint32 operations, seq_nibbles = one code per base"""
    l_seq = len(seq_nibbles)
    assert len(qual) == l_seq
    nib = list(seq_nibbles) + [0] * (l_seq & 1)
    seq = bytes((nib[k] << 4) | nib[k + 1] for k in range(0, len(nib), 2))
    body = struct.pack("<iiBBHHHIiii", refid, pos0, len(qname) + 1, mapq, 4680, len(cigar), flag, l_seq, nref, pnext0, tlen)
    body += qname + b"\0" + struct.pack("<%dI" % len(cigar), *cigar) + seq + bytes(qual) + b"".join(k + t + v for k, t, v in fields)
    return struct.pack("<I", len(body)) + body


def op(length, c):
    return (length << 4) | b"MIDNSHP=X".index(c)


# ---- the float form
KAT = [
    (f32(1.0), b"1"), (f32(1.5), b"1.5"), (f32(0.1), b"0.1"), (f32(100000.0), b"100000"), (f32(1e6), b"1e+06"),
    (f32(1234567.0), b"1.234567e+06"), (f32(0.0001), b"0.0001"), (f32(1e-5), b"1e-05"), (f32(16777216.0), b"1.6777216e+07"),
    (f32(33554448.0), b"3.355445e+07"), (0x7F7FFFFF, b"3.4028235e+38"), (0x00800000, b"1.1754944e-38"), (0x00000001, b"1e-45"),
    (f32(2.0 ** -103), b"9.8607613e-32"),
]
SPECIAL = [(0x7FC00000, b"NaN"), (0xFFC00001, b"NaN"), (0x7F800000, b"+Inf"), (0xFF800000, b"-Inf"), (0x00000000, b"0"), (0x80000000, b"-0"),
           (f32(-1.5), b"-1.5"), (f32(-1e-5), b"-1e-05")]


@pytest.mark.parametrize("bits,text", KAT + SPECIAL)
def test_float_known_answers(bits, text):
    assert samref.float_text(bits) == text


def test_float_layout_boundaries():
    """X = -5, -4, 5, 6 with one and with several digits: the exponent form starts below -4 and at 6"""
    for x, text in ((0.00012, b"0.00012"), (0.000012, b"1.2e-05"), (123456.0, b"123456"), (999999.0, b"999999"), (1000000.0, b"1e+06"),
                    (1200000.0, b"1.2e+06"), (12.5, b"12.5"), (1200.0, b"1200"), (0.5, b"0.5"), (1e10, b"1e+10"), (1e-10, b"1e-10")):
        assert samref.float_text(f32(x)) == text, x


def _numpy_digits(bits):
    s = np.format_float_scientific(np.array([bits], np.uint32).view(np.float32)[0], unique=True, trim="-")
    mant, ex = s.split("e")
    return mant.replace(".", "").lstrip("-"), int(ex)


def _sample(seed, count):
    bits = np.random.default_rng(seed).integers(0, 2 ** 32, count, dtype=np.uint64).astype(np.uint32)
    mag = bits & 0x7FFFFFFF
    return bits[(mag > 0) & (mag < 0x7F800000)]


def test_float_digits_against_numpy():
    """numpy's unique=True is a second opinion on digits and exponent (not on the layout): all 254 powers of two, the ends of the denormal
    range, 2^16 bit patterns of a fixed seed"""
    pows = [ef << 23 for ef in range(1, 255)]
    ends = [1, 2, 3, 0x007FFFFE, 0x007FFFFF, 0x00800000, 0x00800001]
    for bits in pows + ends + _sample(20240607, 1 << 16).tolist():
        assert samref.float_digits(bits & 0x7FFFFFFF) == _numpy_digits(bits & 0x7FFFFFFF), hex(bits)


# ---- hand-written records
def test_line_every_field_type():
    rec = record(b"r1", 99, 0, 99, 60, [op(3, b"S"), op(5, b"M"), op(2, b"I"), op(1, b"D"), op(4, b"N"), op(1, b"H"), op(1, b"P"), op(2, b"="), op(1, b"X")],
                 2, 199, -150, [1, 2, 4, 8, 15, 0, 3], [0, 1, 40, 60, 93, 2, 3],
                 [(b"XA", b"A", b"q"), (b"Xc", b"c", b"\x80"), (b"XC", b"C", b"\xff"), (b"Xs", b"s", struct.pack("<h", -32768)),
                  (b"XS", b"S", struct.pack("<H", 65535)), (b"Xi", b"i", struct.pack("<i", -2147483648)), (b"XI", b"I", struct.pack("<I", 4294967295)),
                  (b"Xf", b"f", struct.pack("<f", 1.5)), (b"XZ", b"Z", b"a b\0"), (b"Xe", b"Z", b"\0"),
                  (b"Bc", b"B", b"c" + struct.pack("<I3b", 3, -128, 0, 127)), (b"BC", b"B", b"C" + struct.pack("<I2B", 2, 0, 255)),
                  (b"Bs", b"B", b"s" + struct.pack("<I2h", 2, -32768, 32767)), (b"BS", b"B", b"S" + struct.pack("<I1H", 1, 65535)),
                  (b"Bi", b"B", b"i" + struct.pack("<I2i", 2, -2147483648, 2147483647)), (b"BI", b"B", b"I" + struct.pack("<I1I", 1, 4294967295)),
                  (b"Bf", b"B", b"f" + struct.pack("<I3f", 3, 1e6, -0.0, 0.1)), (b"B0", b"B", b"c" + struct.pack("<I", 0))])
    want = (b"r1\t99\tchr1\t100\t60\t3S5M2I1D4N1H1P2=1X\t" + NAMES[2] + b"\t200\t-150\tACGTN=M\t!\"I]~#$"
            b"\tXA:A:q\tXc:i:-128\tXC:i:255\tXs:i:-32768\tXS:i:65535\tXi:i:-2147483648\tXI:i:4294967295\tXf:f:1.5\tXZ:Z:a b\tXe:Z:"
            b"\tBc:B:c,-128,0,127\tBC:B:C,0,255\tBs:B:s,-32768,32767\tBS:B:S,65535\tBi:B:i,-2147483648,2147483647\tBI:B:I,4294967295"
            b"\tBf:B:f,1e+06,-0,0.1\tB0:B:c\n")
    assert samref.line(rec, NAMES) == want


def test_line_empty_seq_star_cigar_and_missing_names():
    """l_seq 0: SEQ and QUAL are EMPTY fields (the loops write nothing); no operation: "*"; refid and next_refid below 0: "*"; POS and
    PNEXT 0 (pos0 = -1); TLEN at the int32 ends"""
    rec = record(b"q", 4, -1, -1, 0, [], -1, -1, 2147483647, [], [])
    assert samref.line(rec, NAMES) == b"q\t4\t*\t0\t0\t*\t*\t0\t2147483647\t\t\n"
    rec = record(b"q", 4, -1, -1, 255, [], 1, 0, -2147483648, [1], [7])
    assert samref.line(rec, NAMES) == b"q\t4\t*\t0\t255\t*\tc\t1\t-2147483648\tA\t(\n"


def test_line_rnext_equal_and_named_and_wrapping_pos():
    rec = record(b"q", 65535, 1, 2147483647, 7, [op(268435455, b"M")], 1, 9, 0, [8, 8], [10, 11])
    assert samref.line(rec, NAMES) == b"q\t65535\tc\t-2147483648\t7\t268435455M\t=\t10\t0\tTT\t+,\n"   # int32(pos) + 1 wraps (bam-files.go:327)
    rec = record(b"q", 0, 1, 0, 7, [op(1, b"M")], 0, 0, 0, [8], [10])
    assert samref.line(rec, NAMES) == b"q\t0\tc\t1\t7\t1M\tchr1\t1\t0\tT\t+\n"


def test_line_missing_qualities_leave_as_spaces():
    """BAM's 0xFF bytes + 33 wrap to 0x20, as `qual+33` on a byte does (sam-files.go:589-591)"""
    rec = record(b"q", 0, 0, 0, 7, [op(3, b"M")], -1, -1, 0, [1, 2, 4], [255, 255, 255])
    assert samref.line(rec, NAMES) == b"q\t0\tchr1\t1\t7\t3M\t*\t0\t0\tACG\t   \n"
    assert samref.line(record(b"q", 0, 0, 0, 7, [op(1, b"M")], -1, -1, 0, [1], [223]), NAMES).endswith(b"\tA\t\x00\n")


def test_lines_of_a_stream_and_h_fields_raise():
    a = record(b"a", 0, 0, 0, 7, [op(1, b"M")], -1, -1, 0, [1], [1])
    b = record(b"b", 16, 1, 4, 7, [op(1, b"M")], -1, -1, 0, [2], [2], [(b"NM", b"C", b"\x03")])
    assert samref.lines(a + b, ["chr1", "c"]) == b"a\t0\tchr1\t1\t7\t1M\t*\t0\t0\tA\t\"\nb\t16\tc\t5\t7\t1M\t*\t0\t0\tC\t#\tNM:i:3\n"
    with pytest.raises(ValueError):
        samref.line(tagref.with_fields(a, [(b"XH", b"H", b"1AE3\0")]), NAMES)
