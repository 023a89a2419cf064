"""The oracle's computeTileInfo, distance rule and panic rule against a restatement of Go's (tests/optical_names.py):
strconv.ParseInt(s, 10, 64) on every field shape, absInt on Go's wrapping int, and which names the reference parses at all
(filters/mark-optical-duplicates.go:50-71, 327-368; internal/strconv.go:27; filters/unpedantic.go:32; filters/utils.go:62)."""
import numpy as np
import pytest

import oracle as orc
from tests import optical_names as on


def _checked(name: bytes):
    return orc.tile_info_checked(name)


# ---- parser
HAND_FIELDS = [b"", b"+", b"-", b"-0", b"+0", b"+7", b"-7", b" 7", b"7 ", b"1_0", b"0x1", b"0X1", "٣".encode(), b"+-1", b"--1", b"1-",
               b"00", b"0000000000000000000000001234", b"123456789012345678", b"-123456789012345678", b"1234567890123456789",
               b"-1234567890123456789", b"12345678901234567890", b"-12345678901234567890", b"9223372036854775807", b"+9223372036854775807",
               b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"18446744073709551615", b"18446744073709551616",
               b"99999999999999999999999", b"0000000000000000000009223372036854775807", b"-0000000000000000000009223372036854775808",
               b"0000000000000000000009223372036854775808", b"1e3", b"1.0", b"\t1", b"\x001", b"1\xff"]


@pytest.mark.parametrize("field", HAND_FIELDS, ids=lambda f: repr(f)[2:-1] or "empty")
@pytest.mark.parametrize("where", ["x7", "t7", "y7", "x5"])
def test_parse_int_hand_table(field, where):
    """One field of a 5- or 7-column name through the oracle's parser and Go's.  Fails on the parent commit's oracle for the
    range errors (19 digits over 2^63 - 1, 20+ digits: undefined behaviour, accepted) and for every syntax error, which the parent
    folded into "no tile info" with no panic flag (there was no tile_info_checked)."""
    t, x, y = b"1101", b"-42", b"+0042"
    if where[0] == "t":
        t = field
    elif where[0] == "x":
        x = field
    else:
        y = field
    nm = on.tile_name(1, int(where[1]), t, x, y)
    assert _checked(nm) == on.go_tile_info(nm)


def test_parse_int_values_at_the_range_ends():
    """±2^63, 2^63 - 1, 18 / 19 / 20 digits and 25-character zero-padded values, checked for their value, not just their status.
    Fails on the parent commit's oracle (2^63 and 20 digits were taken as valid)."""
    cases = {b"9223372036854775807": on.I64_MAX, b"-9223372036854775808": on.I64_MIN, b"9223372036854775808": None,
             b"-9223372036854775809": None, b"999999999999999999": 10 ** 18 - 1, b"1000000000000000000": 10 ** 18,
             b"-1000000000000000000": -(10 ** 18), b"10000000000000000000": None, b"0000000000000000000000042": 42,
             b"-000000000000000000000042": -42, b"+000000000000000000000042": 42, b"0000009223372036854775807": on.I64_MAX}
    for f, v in cases.items():
        assert on.go_parse_int(f) == ((v, None) if v is not None else (None, "range")), f
        got = _checked(b"a:b:1:" + f + b":" + f)
        assert got == ((1, v, v, False) if v is not None else (-1, -1, -1, True)), f


@pytest.mark.parametrize("ncol", range(1, 11))
def test_column_counts(ncol):
    """0..9 colons; empty unused columns and a trailing ':' (an empty last column).  Only 5 and 7 columns carry tile info; the
    other counts are never parsed, so a bad field there does not panic (asserts what the parent already did, plus the flag)."""
    for body in (b"", b"x", b"7"):
        nm = b":".join([body] * ncol)
        assert _checked(nm) == on.go_tile_info(nm), nm
    nm = b":".join([b"1"] * (ncol - 1)) + b":" if ncol > 1 else b""
    assert _checked(nm) == on.go_tile_info(nm)
    nm = on.tile_name(3, ncol, b"12", b"34", b"56")
    assert nm.count(b":") == ncol - 1
    assert _checked(nm) == on.go_tile_info(nm)


def sweep_names(count, seed=2026):
    """(columns, name) of `count` random names over the alphabets of the hand table (digits, signs, zero padding, spaces, '_', 'x', a
    non-ASCII digit, empty fields) with 0..9 colons"""
    rng = np.random.default_rng(seed)
    junk = [b" ", b"_", b"x", b"+", b"-", "٣".encode(), b"."]
    big = [str(v).encode() for v in on.EDGE_VALUES] + [b"9223372036854775808", b"18446744073709551616", b"-9223372036854775809"]

    def field():
        r = rng.random()
        if r < 0.35:
            s = b"".join(b"%d" % d for d in rng.integers(0, 10, int(rng.integers(1, 22))))
        elif r < 0.6:
            s = big[int(rng.integers(0, len(big)))]
        elif r < 0.7:
            s = b""
        else:
            s = b"%d" % int(rng.integers(0, 100000))
        if s[:1] != b"-" and rng.random() < 0.3:
            s = (b"+", b"-")[int(rng.integers(0, 2))] + s
        if rng.random() < 0.3:
            s = b"0" * int(rng.integers(1, 8)) + s.lstrip(b"+-") if not s.startswith((b"+", b"-")) else s[:1] + b"0" * int(rng.integers(1, 8)) + s[1:]
        if rng.random() < 0.12:
            k = int(rng.integers(0, len(s) + 1))
            s = s[:k] + junk[int(rng.integers(0, len(junk)))] + s[k:]
        return s

    for _ in range(count):
        ncol = int(rng.choice([5, 7, 5, 7, 1, 2, 3, 4, 6, 8, 9, 10]))
        yield ncol, b":".join(field() for _ in range(ncol))


def test_random_names_sweep():
    """120 000 names over the alphabets of the hand table (digits, signs, zero padding, spaces, '_', 'x', a non-ASCII digit, empty
    fields) with 0..9 colons, against the restatement.  Every class is reached: valid, syntax error, range error, 5 columns, 7
    columns, other counts.  Fails on the parent commit's oracle (range errors, panic flag)."""
    seen = {"valid": 0, "syntax": 0, "range": 0, "5": 0, "7": 0, "other": 0}
    for ncol, nm in sweep_names(120_000):
        want = on.go_tile_info(nm)
        assert _checked(nm) == want, nm
        seen[str(ncol) if ncol in (5, 7) else "other"] += 1
        if ncol in (5, 7):
            errs = [on.go_parse_int(f)[1] for f in nm.split(b":")[-3:]]
            for e in errs:
                seen[e or "valid"] += 1
    assert min(seen.values()) > 1000, seen


# ---- distance
DISTS = [0, 1, 100, 2500, (1 << 31) - 1, -5, -(1 << 31)]


def _pair_case(uid, t, a, b, dist):
    """a set of two pairs (the origin and one duplicate, both listed forward, one RG): optical count 1 iff the tiles are close"""
    rng = np.random.default_rng(uid)
    names = [on.tile_name(2 * uid + k, 7, b"%d" % t, on.spell(p[0], rng), on.spell(p[1], rng)) for k, p in enumerate((a, b))]
    return on.Pile(names, [True, True], [0, 0])


def _distance_cases(dist):
    cases = []
    for base in (0, 5000, on.I64_MAX, on.I64_MIN, on.I64_MAX - 3, on.I64_MIN + 3, -(1 << 62), 1 << 62):
        for dx in (0, dist, -dist, dist + 1, -dist - 1, 1, -1):
            for dy in (0, dist, dist + 1, -dist):
                cases.append(((base, 7), (on.wrap64(base + dx), on.wrap64(7 + dy))))
    # differences that overflow int64, and the one that leaves absInt negative (MinInt64)
    for a, b in ((on.I64_MAX, on.I64_MIN), (on.I64_MIN, on.I64_MAX), (on.I64_MAX, -1), (-2, on.I64_MAX), (0, on.I64_MIN), (on.I64_MIN, 0),
                 (-1, on.I64_MAX), (on.I64_MAX, on.I64_MIN + 1), (1 << 62, -(1 << 62)), ((1 << 62) + 1, -(1 << 62))):
        cases += [((a, 0), (b, 0)), ((0, a), (0, b)), ((a, a), (b, b))]
    return cases


@pytest.mark.parametrize("dist", DISTS)
def test_distance_predicate(dist):
    """isOpticalDuplicateShort on Go's int: x1 - x2 wraps mod 2^64 and absInt(MinInt64) stays negative, so a difference of exactly
    2^63 counts as close for every distance >= -2^63.  Each case is a set of two through orc.dup_metrics; the restatement decides
    with Python ints reduced mod 2^64.  Asserts what the parent commit's oracle already computed: its signed overflow was undefined
    behaviour that the host compiler happened to wrap; the subtraction is now defined to wrap."""
    h = on.header(1)
    for k, (a, b) in enumerate(_distance_cases(dist)):
        want = on.go_short_close((7,) + a, (7,) + b, dist)
        p = _pair_case(k, 7, a, b, dist)
        assert p.expected(dist)[0] == int(want)
        _, ctr, _ = orc.dup_metrics(on.batch([p]), h, None, dist)
        assert ctr[0, 6] == int(want), (dist, a, b)
    assert on.go_short_close((1, on.I64_MIN, 0), (1, 0, 0), 0) and on.go_abs(on.I64_MIN) == on.I64_MIN


def test_tile_minus_one_is_no_tile():
    """A tile field that parses to -1 is "no tile info" in Go (isOpticalDuplicate compares t with -1; countOpticalDuplicatesWithGraph
    skips it): such members are never optical duplicates, though they do not panic.  Asserts what the parent already did."""
    h = on.header(1)
    for n in (2, 3, 4, 6):
        names = [on.tile_name(k, 5, b"-1", b"10", b"10") for k in range(n)]
        p = on.Pile(names, [True] * n, [0] * n)
        assert p.expected(100) == (0, n, False)
        _, ctr, _ = orc.dup_metrics(on.batch([p]), h, None, 100)
        assert ctr[0, 6] == 0
        names = [on.tile_name(k, 5, b"-00001", b"10", b"10") for k in range(n)]
        _, ctr, _ = orc.dup_metrics(on.batch([on.Pile(names, [True] * n, [0] * n)]), h, None, 100)
        assert ctr[0, 6] == 0


# ---- which names the reference parses
BAD = [b"12x", b"9223372036854775808", b"", b"+", b"1 "]


def _set(n, bad_at, fwd, rg=None, uid0=0, bad=b"12x"):
    names = [on.tile_name(uid0 + k, 7, b"1101", b"%d" % (1000 + 10 * k), b"2000") for k in range(n)]
    for k in bad_at:
        names[k] = on.tile_name(uid0 + k, 7, b"1101", bad, b"2000")
    return on.Pile(names, fwd, [0] * n if rg is None else rg)


@pytest.mark.parametrize("bad", BAD, ids=lambda f: repr(f)[2:-1] or "empty")
def test_panic_rule_on_hand_built_sets(bad):
    """A bad field panics the reference exactly where computeTileInfo runs: on a member of a strand list of 2 to 300000 entries.
    A bad name in a list of 2, 3 or 5 raises; alone on its strand (the other members listed on the other strand), or on a pair that
    is in no duplicate set, it does not, and the counts are those of the restatement.  Fails on the parent commit's oracle (a bad
    field there was "no tile info" everywhere: nothing raised)."""
    h = on.header(2)
    for n, at in ((2, 0), (2, 1), (3, 2), (5, 3), (5, 0)):
        p = _set(n, [at], [True] * n, bad=bad)
        assert p.expected(100)[2]
        with pytest.raises(RuntimeError, match="reference would panic"):
            orc.dup_metrics(on.batch([p]), h, None, 100)
        with pytest.raises(RuntimeError, match="reference would panic"):
            orc.dup_metrics_mt(on.batch([p]), h, None, 100, 3)
    # alone on its strand: fwd list of one (the bad member), reverse list of n - 1 valid members
    piles = []
    for s, (n, at) in enumerate(((2, 0), (3, 1), (5, 4), (6, 0))):
        fwd = [False] * n
        fwd[at] = True
        piles.append(_set(n, [at], fwd, rg=[0, 1] * (n // 2) + [0] * (n % 2), uid0=100 * s, bad=bad))
    singles = [(on.tile_name(900, 7, b"1", bad, b"1"), 1), (on.tile_name(901, 5, bad, bad, bad), 0)]
    b = on.batch(piles, singles)
    opt, hist, panics = on.expected_metrics(piles, 100, 8)
    assert not panics
    flags, ctr, ohist = orc.dup_metrics(b, h, None, 100, hist_len=8)
    assert ctr[0, 6] == opt and opt > 0
    assert np.array_equal(ohist[0, :, :][:, 2:], hist[:, 2:])  # (bin 1 also holds the origins without duplicates: the singles)
    assert np.array_equal(orc.dup_metrics_mt(b, h, None, 100, 3)[1], ctr)
