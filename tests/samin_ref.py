"""SAM text IN restated in plain Python (test infrastructure: no device code, nothing of elprep_amd): one alignment line + the @SQ names
-> the BAM record formatBamAlignment(parseSamAlignment(line)) writes behind AddREFID, or the class of the refusal.  Written from the Go
sources:

    record               parseSamAlignment                     sam/sam-files.go:386-410
                         stringScanner                         sam/string-scanner.go
                         formatBamAlignment, bin, formatBamTag sam/bam-files.go:443-737
                         AddREFID                              filters/simple-filters.go:208-231
    cigar                ScanCigarString, slowScanCigarString  sam/sam-types.go:680-740
    field                parseSamOptionalField and its table   sam/sam-files.go:186-346
    split_lines          bufio.ScanLines                       behind sam/sam-files.go:617-629
    parse_int / _uint    strconv.ParseInt / ParseUint          from their documentation
    parse_float32        float32(strconv.ParseFloat(s, 32))    from its documentation, in exact rational arithmetic (fractions)

A refusal is SamError with cls "data" (the reference panics: ELP_ERR_DATA) or "unsupported" (the reference reads it, elp_stage_sam does
not: ELP_ERR_UNSUPPORTED) - the limits include/elprep_hip.h lists: names outside the dictionary, a CIGAR operation above 2^28 - 1 or more
than 65535 of them, QUAL and SEQ of different lengths, QNAME above 254 bytes or with a NUL, two fields of one key, an i value outside
[-2^31, 2^32 - 1], a NUL in a Z value, H fields, hexadecimal floats, underscores in floats, float tokens above 64 bytes, more than 245
optional fields, and a tab as a key byte or as an A value (which the reference's scanner steps over)."""
import struct
from fractions import Fraction

BASES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
MAX_LINE = 1 << 20
MAX_FIELDS = 245


class SamError(Exception):
    def __init__(self, cls, why):
        super().__init__("%s: %s" % (cls, why))
        self.cls = cls


def _data(why):
    return SamError("data", why)


def _unsupported(why):
    return SamError("unsupported", why)


def split_lines(text):
    """bufio.ScanLines: the bytes up to each newline, one trailing carriage return dropped; a last line without a newline counts"""
    text = bytes(text)
    out = text.split(b"\n")
    if out[-1] == b"":
        out.pop()
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in out]


def parse_uint(s, bits):
    if len(s) == 0 or any(c not in b"0123456789" for c in s):
        raise _data("ParseUint %r" % s)
    v = int(s)
    if v >= 1 << bits:
        raise _data("ParseUint %r: out of range" % s)
    return v


def parse_int(s, bits):
    neg = s[:1] == b"-"
    body = s[1:] if s[:1] in (b"+", b"-") else s
    if len(body) == 0 or any(c not in b"0123456789" for c in body):
        raise _data("ParseInt %r" % s)
    v = -int(body) if neg else int(body)
    if not -(1 << (bits - 1)) <= v < (1 << (bits - 1)):
        raise _data("ParseInt %r: out of range" % s)
    return v


def float32_bits(v):
    """bits of the float32 nearest the Fraction v > 0, ties to even; None beyond the largest float32"""
    e = v.numerator.bit_length() - v.denominator.bit_length()
    two = lambda k: Fraction(1 << k) if k >= 0 else Fraction(1, 1 << -k)
    if two(e) > v:
        e -= 1
    assert two(e) <= v < two(e + 1)
    if e > 127:
        return None
    q = max(e, -126) - 23                                  # the exponent of the last mantissa bit
    m = v / two(q)
    M = m.numerator // m.denominator
    rem = m - M
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and M % 2 == 1):
        M += 1
    bits = ((e + 127) << 23) + (M - (1 << 23)) if e >= -126 else M
    return None if bits >= 0x7F800000 else bits


def parse_float32(s):
    """bits of float32(strconv.ParseFloat(s, 32))"""
    s = bytes(s)
    if len(s) == 0:
        raise _data("ParseFloat: empty")
    if len(s) > 64 or b"_" in s:
        raise _unsupported("float token %r" % s)
    neg = s[:1] == b"-"
    body = s[1:] if s[:1] in (b"+", b"-") else s
    sign = 0x80000000 if neg else 0
    low = body.lower()
    if low in (b"inf", b"infinity"):
        return sign | 0x7F800000
    if s.lower() == b"nan":
        return 0x7FC00000
    if low[:2] == b"0x":
        raise _unsupported("hexadecimal float %r" % s)
    mant, exp = body, 0
    for k, c in enumerate(body):
        if c in b"eE":
            mant = body[:k]
            exp = parse_exponent(body[k + 1:])
            break
    ip, dot, fp = mant.partition(b".")
    if b"." in fp or len(ip) + len(fp) == 0 or any(c not in b"0123456789" for c in ip + fp):
        raise _data("ParseFloat %r" % s)
    digits = int(ip + fp)
    if digits == 0:
        return sign
    exp10 = max(min(exp, 100000), -100000) - len(fp)       # (strconv caps the exponent it accumulates; far outside the range either way)
    if exp10 > 100 or exp10 < -200:
        v = None if exp10 > 100 else 0
    else:
        v = Fraction(digits) * (Fraction(10) ** exp10)
    if v is None:
        raise _data("ParseFloat %r: out of range" % s)
    if v == 0:
        return sign
    if v <= Fraction(1, 1 << 150):                         # at most half the smallest denormal: 0 (the tie goes to the even 0)
        return sign
    bits = float32_bits(v)
    if bits is None:
        raise _data("ParseFloat %r: out of range" % s)
    return sign | bits


def parse_exponent(s):
    body = s[1:] if s[:1] in (b"+", b"-") else s
    if len(body) == 0 or any(c not in b"0123456789" for c in body):
        raise _data("ParseFloat: exponent %r" % s)
    return -int(body) if s[:1] == b"-" else int(body)


def cigar(s):
    """ScanCigarString: [(length, op code)] with adjacent equal operations merged"""
    if s == b"*" or s == b"":
        return []
    ops, i, last = [], 0, None
    while i < len(s):
        j = i
        while j < len(s) and s[j] in b"0123456789":
            j += 1
        if j >= len(s):
            raise _data("CIGAR ends in digits")            # cigar[j]: index out of range
        length = parse_int(s[i:j], 32)
        op = bytes([s[j]]).upper()
        if op not in (b"M", b"I", b"D", b"N", b"S", b"H", b"P", b"X", b"="):
            raise _data("invalid CIGAR operation")
        code = CIGAR_OPS.index(op)
        if code == last:
            ops[-1][0] += length
        else:
            ops.append([length, code])
        last = code
        i = j + 1
    if any(length > (1 << 28) - 1 for length, _ in ops):
        raise _unsupported("CIGAR operation longer than 2^28 - 1")
    if len(ops) > 65535:
        raise _unsupported("more than 65535 CIGAR operations")
    return [(length, code) for length, code in ops]


_B_INT = {b"c": (parse_int, 8, "<b"), b"C": (parse_uint, 8, "<B"), b"S": (parse_uint, 16, "<H"), b"i": (parse_int, 32, "<i"), b"I": (parse_uint, 32, "<I")}


def field(f):
    """one optional field's text (without its tab) -> (key, BAM type, BAM value bytes)"""
    if len(f) < 5 or b":" in f[:2] or f[2:3] != b":" or f[4:5] != b":":
        raise _data("invalid field %r" % f[:8])
    key, ty, val = f[:2], f[3:4], f[5:]
    if ty == b"A":
        if len(val) != 1:
            raise _data("A field of %d bytes" % len(val))
        return key, b"A", val
    if ty == b"i":
        v = parse_int(val, 64)
        if not -(1 << 31) <= v <= (1 << 32) - 1:
            raise _unsupported("integer field outside BAM's types")
        if v < 0:
            t, fmt = (b"c", "<b") if v >= -128 else ((b"s", "<h") if v >= -32768 else (b"i", "<i"))
        else:
            t, fmt = (b"C", "<B") if v <= 255 else ((b"S", "<H") if v <= 65535 else (b"I", "<I"))
        return key, t, struct.pack(fmt, v)
    if ty == b"f":
        return key, b"f", struct.pack("<I", parse_float32(val))
    if ty == b"Z":
        if b"\0" in val:
            raise _unsupported("NUL in a Z field")
        return key, b"Z", val + b"\0"
    if ty == b"H":
        raise _unsupported("H field")
    if ty == b"B":
        if len(val) < 2 or val[1:2] != b",":
            raise _data("missing entry in numeric array")
        sub, entries = val[:1], val[2:].split(b",")
        if sub == b"f":
            body = b"".join(struct.pack("<I", parse_float32(x)) for x in entries)
        elif sub == b"s":                                   # int16(ParseUint(entry, 10, 16)), sam/sam-files.go:263-272
            body = b"".join(struct.pack("<H", parse_uint(x, 16)) for x in entries)
        elif sub in _B_INT:
            fn, bits, fmt = _B_INT[sub]
            body = b"".join(struct.pack(fmt, fn(x, bits)) for x in entries)
        else:
            raise _data("invalid numeric array type")
        return key, b"B", sub + struct.pack("<I", len(entries)) + body
    raise _data("invalid field type %r" % ty)


def _i32(v):
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def bam_bin(flag, pos, ops):
    """Alignment.bin(), sam/bam-files.go:443-468, in int32 arithmetic"""
    beg = _i32(pos - 1)
    end = beg
    if not flag & 4:
        for length, code in ops:
            if CIGAR_OPS[code] in b"MDN=X":
                end = _i32(end + length)
        end = _i32(end - 1)
    for shift, k in ((14, 15), (17, 12), (20, 9), (23, 6), (26, 3)):
        if beg >> shift == end >> shift:
            return (((1 << k) - 1) // 7 + (beg >> shift)) & 0xFFFF
    return 0


def record(line, names):
    """the BAM record (block_size field in front) of one line (no newline, no carriage return); names: the @SQ SN strings as bytes"""
    line = bytes(line)
    if len(line) > MAX_LINE:
        raise _data("line longer than 1 MiB")
    cols = line.split(b"\t")
    if len(cols) < 11:
        raise _data("missing tabulator in SAM alignment line")
    qname, flag, rname, pos, mapq, cig, rnext, pnext, tlen, seq, qual = cols[:11]
    flag = parse_uint(flag, 16)
    pos = parse_int(pos, 32)
    mapq = parse_uint(mapq, 8)
    ops = cigar(cig)
    pnext = parse_int(pnext, 32)
    tlen = parse_int(tlen, 32)
    opt = cols[11:]
    if len(opt) > MAX_FIELDS:                              # (a tab behind the last field counts as one)
        raise _unsupported("more than %d optional fields" % MAX_FIELDS)
    if opt and opt[-1] == b"":                             # a tab behind the last field: sc.len() is 0, the loop ends
        opt.pop()
    fields = [field(f) for f in opt]
    if len({k for k, _, _ in fields}) != len(fields):
        raise _unsupported("two fields of one key")
    table = {nm: k for k, nm in enumerate(names)}

    def refid(name):
        if name == b"*":
            return -1
        if name not in table:
            raise _unsupported("reference name %r is not in the dictionary" % name)
        return table[name]

    rid = -1 if rname == b"=" else refid(rname)            # (AddREFID finds no contig of that name; only RNEXT "=" means something)
    nid = rid if rnext == b"=" else refid(rnext)
    if len(qname) > 254:
        raise _unsupported("QNAME longer than 254 bytes")
    if b"\0" in qname:
        raise _unsupported("NUL in QNAME")
    nib = [BASES.index(bytes([c])) if bytes([c]) in BASES else 15 for c in seq]
    if len(qual) != len(seq):
        raise _unsupported("QUAL and SEQ differ in length")
    packed = bytes((nib[k] << 4) | (nib[k + 1] if k + 1 < len(nib) else 0) for k in range(0, len(nib), 2))
    body = struct.pack("<iiBBHHHIiii", rid, _i32(pos - 1), len(qname) + 1, mapq, bam_bin(flag, pos, ops), len(ops), flag, len(seq), nid, _i32(pnext - 1), tlen)
    body += qname + b"\0" + b"".join(struct.pack("<I", (length << 4) | code) for length, code in ops) + packed
    body += bytes((c - 33) & 0xFF for c in qual) + b"".join(k + t + v for k, t, v in fields)
    return struct.pack("<I", len(body)) + body


def records(text, names):
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    return [record(ln, names) for ln in split_lines(text)]
