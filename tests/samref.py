"""SAM text restated in plain Python on BAM record bytes (test infrastructure: no device code, nothing of elprep_amd): one alignment
record + the @SQ names -> the line FormatAlignment(parseBamAlignment(record)) writes.  Written from the Go sources:

    line                 parseBamAlignment                     sam/bam-files.go:317-400
                         FormatAlignment                       sam/sam-files.go:563-598
    cigar_text           cigarToString                         sam/sam-files.go:548-557
    field_text           formatSamTag                          sam/sam-files.go:485-546
    float_text           strconv.AppendFloat(v, 'g', -1, 32)   from its definition, in exact rational arithmetic

A record is its bytes with the block_size field in front (tests/tagref.py); names are bytes.  H fields, which the emitters refuse, raise.

float_text.  The shortest decimal that reads back as the float32: with x the value, the rounding interval reaches half a gap to either
side of x - the lower half gap is half as wide where x is a power of two above the smallest normal exponent -, its bounds belong to it
iff the mantissa is even; n is the smallest number of digits for which some n-digit decimal lies in the interval, and of those the one
nearest x is taken.  Layout (%e / %f as strconv's 'g' chooses with the shortest form, where the precision counts as 6): with the decimal
exponent X of the first digit, X < -4 or X >= 6 gives d[.ddd]e+XX (sign always, two exponent digits at least), else positional without
trailing zeros.  NaN, +Inf, -Inf, 0 and -0 are spelled so."""
import struct
from fractions import Fraction

from tests import tagref

BASES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
_ELEM = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}


_P10 = [10 ** k for k in range(64)]


def float_digits(bits):
    """(digits as a str of n characters, X) of the finite non-zero float32 with these bits (sign ignored).  x and the interval's bounds
    are Fractions made as the definition says; the search for the digits compares their numerators over one common denominator (plain
    integers: a test asks this function about a million values)"""
    bits &= 0x7FFFFFFF
    frac, ef = bits & 0x7FFFFF, bits >> 23
    assert 0 < bits < 0x7F800000
    m, e = (frac | 0x800000, ef - 150) if ef else (frac, -149)
    x = Fraction(m << e) if e >= 0 else Fraction(m, 1 << -e)
    gap = Fraction(1 << e) if e >= 0 else Fraction(1, 1 << -e)
    hi = x + gap / 2
    lo = x - (gap / 4 if frac == 0 and ef > 1 else gap / 2)
    closed = m % 2 == 0
    D = 4 << max(-e, 0)                                  # a common denominator of x, lo and hi
    xn, ln, hn = (v.numerator * (D // v.denominator) for v in (x, lo, hi))
    # X0 = floor(log10 x), exactly: 10^X0 <= x < 10^(X0 + 1)
    X0 = len(str(xn)) - len(str(D))
    ge = lambda X: _P10[X] * D <= xn if X >= 0 else D <= xn * _P10[-X]   # 10^X <= x
    while not ge(X0):
        X0 -= 1
    while ge(X0 + 1):
        X0 += 1
    for n in range(1, 18):
        p = X0 - n + 1                                   # 10^p = the last of n digits, for decimals of x's decade
        if p >= 0:
            U, xs, ls, hs = D * _P10[p], xn, ln, hn      # a decimal c * 10^p is c * U over D
        else:
            U, xs, ls, hs = D, xn * _P10[-p], ln * _P10[-p], hn * _P10[-p]  # ... or c * D over D * 10^-p
        k = xs // U
        best = None
        for c in (k, k + 1):                             # the n-digit decimals next to x, below and above (10^n = the next decade's 1)
            v = c * U
            if (ls <= v <= hs) if closed else (ls < v < hs):
                key = (abs(v - xs), c % 2)
                if best is None or key < best[0]:
                    best = (key, c)
        if best is not None:
            c, X = best[1], X0
            if c == _P10[n]:                             # rounded up into the next decade
                c, X = _P10[n - 1], X0 + 1
            digits = str(c)
            assert len(digits) == n
            return digits.rstrip("0") or "0", X
    raise AssertionError("no decimal of 17 digits in the interval")


def float_text(bits):
    """strconv.AppendFloat(float64(v), 'g', -1, 32) of the float32 with these bits"""
    neg, mag = bits >> 31, bits & 0x7FFFFFFF
    if mag > 0x7F800000:
        return b"NaN"
    if mag == 0x7F800000:
        return b"-Inf" if neg else b"+Inf"
    sign = b"-" if neg else b""
    if mag == 0:
        return sign + b"0"
    d, X = float_digits(mag)
    if X < -4 or X >= 6:
        s = d[0] + ("." + d[1:] if len(d) > 1 else "") + "e" + ("-" if X < 0 else "+") + "%02d" % abs(X)
    elif X >= 0:
        ip = d[:X + 1].ljust(X + 1, "0")
        s = ip + ("." + d[X + 1:] if len(d) > X + 1 else "")
    else:
        s = "0." + "0" * (-X - 1) + d
    return sign + s.encode()


def cigar_text(ops):
    """ops: the uint32 operations of the record"""
    if not ops:
        return b"*"
    return b"".join(b"%d%c" % (op >> 4, CIGAR_OPS[op & 0xF]) for op in ops)


def field_text(key, ty, val):
    """one optional field (tagref's triple) with its leading tab"""
    head = b"\t" + key + b":"
    if ty == b"A":
        return head + b"A:" + val[:1]
    if ty in _ELEM:
        return head + b"i:" + b"%d" % struct.unpack(_ELEM[ty], val)[0]
    if ty == b"f":
        return head + b"f:" + float_text(struct.unpack("<I", val)[0])
    if ty == b"Z":
        assert val[-1:] == b"\0"
        return head + b"Z:" + val[:-1]
    if ty == b"B":
        sub, count = val[0:1], struct.unpack_from("<I", val, 1)[0]
        out = head + b"B:" + sub
        if sub == b"f":
            return out + b"".join(b"," + float_text(w) for w in struct.unpack_from("<%dI" % count, val, 5))
        fmt = _ELEM[sub]
        return out + b"".join(b",%d" % v for v in struct.unpack_from("<%d%s" % (count, fmt[1]), val, 5))
    raise ValueError("field type %r" % ty)


def line(rec, names):
    """the SAM line of one BAM record (block_size field in front)"""
    refid, pos0, l_name, mapq, _bin, n_cig, flag, l_seq, nref, pnext0, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 4)
    rname = b"*" if refid < 0 else names[refid]
    if nref < 0:
        rnext = b"*"
    else:
        rnext = names[nref]
        if rnext == rname:
            rnext = b"="
    p = 36
    qname = rec[p:p + l_name - 1]
    p += l_name
    ops = struct.unpack_from("<%dI" % n_cig, rec, p)
    p += 4 * n_cig
    seq = bytes(BASES[(rec[p + (k >> 1)] >> (0 if k & 1 else 4)) & 15] for k in range(l_seq))
    p += (l_seq + 1) // 2
    qual = bytes((q + 33) & 0xFF for q in rec[p:p + l_seq])
    p += l_seq
    assert p == tagref.tags_at(rec)
    i32 = lambda v: ((v + 2 ** 31) % 2 ** 32) - 2 ** 31              # int32(...) + 1 wraps
    cols = [qname, b"%d" % flag, rname, b"%d" % i32(pos0 + 1), b"%d" % mapq, cigar_text(ops), rnext, b"%d" % i32(pnext0 + 1), b"%d" % tlen, seq, qual]
    return b"\t".join(cols) + b"".join(field_text(*f) for f in tagref.parse_fields(rec)) + b"\n"


def lines(bam_bytes, names):
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    return b"".join(line(r, names) for r in tagref.records(bam_bytes))
