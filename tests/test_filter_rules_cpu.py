"""The filters' per-record rules, run on the CPU: elprep_amd/csrc/filter_rules.hpp is host-and-device code, and
tests/filter_rules_host.cpp builds it with the host compiler - the functions the kernels of filter.hip, clean_sam.hip, split_merge.hip
and split.hip run.  Every comparison is against the oracle's restatement (oracle/simple_filters.py, tests/tagref.py) or a value worked
out by hand, never against the code under test."""
import ctypes as C
import itertools
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from elprep_amd.batch import batch_from_records, parse_cigar
from oracle import simple_filters as sf
from tests import tagref
from tests.test_clean_sam_kat import CASES, LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libfilter_rules_host.so")
CSRC = os.path.join(ROOT, "elprep_amd", "csrc")
I32P, U32P, U64P, I64P = (C.POINTER(t) for t in (C.c_int32, C.c_uint32, C.c_uint64, C.c_int64))


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "filter_rules_host.cpp")
    hdrs = [os.path.join(CSRC, "filter_rules.hpp"), os.path.join(CSRC, "bamtag_read.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src])
    L = C.CDLL(SO)
    L.fr_merge_key.restype = L.fr_merge_upper_bound.restype = C.c_uint64
    L.fr_merge_key.argtypes = [C.c_int32, C.c_int32]
    L.fr_merge_upper_bound.argtypes = [U64P, C.c_uint64, C.c_uint64]
    L.fr_overlap.argtypes = [I32P, C.c_int64, C.c_int32, C.c_int32]
    L.fr_clean_cigar.argtypes = [U32P, C.c_int, C.c_uint16, C.c_int32, C.c_int32, U32P, C.POINTER(C.c_int)]
    L.fr_clean_length.argtypes = [I32P, C.c_int32, C.c_int32]
    L.fr_record_rejected.argtypes = [C.POINTER(C.c_int), C.c_uint16, C.c_int32, C.c_int32, C.c_uint8, U32P, C.c_uint64, C.c_int32, I32P, I64P,
                                     C.POINTER(C.c_int)]
    L.fr_split_route.argtypes = [C.c_int32, C.c_int32, I32P, C.c_int32, I32P]
    L.fr_strict.argtypes = [C.c_char_p]
    return L


def _p(a, t):
    return a.ctypes.data_as(t)


# ---- clean_cigar

def _clean(L, ops, flag, pos, length):
    """-> (return code, new ops or None, changed); the count-only call must agree with the writing one"""
    ops = np.ascontiguousarray(ops, np.uint32)
    changed, changed0 = C.c_int(-1), C.c_int(-1)
    n0 = L.fr_clean_cigar(_p(ops, U32P), ops.size, flag, pos, length, None, C.byref(changed0))
    if n0 < 0:  # (the write pass runs only once the count pass has shown that no record fails)
        return n0, None, bool(changed0.value)
    out = np.full(n0 + 1, 0xDEADBEEF, np.uint32)  # exactly the count, and a word behind it that must stay
    n = L.fr_clean_cigar(_p(ops, U32P), ops.size, flag, pos, length, _p(out, U32P), C.byref(changed))
    assert n == n0 and changed.value == changed0.value and out[-1] == 0xDEADBEEF
    return n, (out[:n].copy() if n >= 0 else None), bool(changed.value)


def test_clean_cigar_known_answers(lib):
    """Every row of the hand-derived table of tests/test_clean_sam_kat.py: the rewritten CIGAR, the row where the reference panics
    (-1), the two rows with RNAME '*' (length 0 from the lookup beside clean_cigar)."""
    ref_len = np.array([LN], np.int32)
    for rec, want in CASES:
        cig, pos, flag = rec[0], rec[1], rec[2]
        refid = rec[4] if len(rec) > 4 else 0
        length = lib.fr_clean_length(_p(ref_len, I32P), 1, refid)
        assert length == (LN if refid == 0 else 0)
        n, out, changed = _clean(lib, parse_cigar(cig), flag, pos, length)
        if want is None:
            assert n == -1, rec
        else:
            assert n == len(parse_cigar(want[0])) and np.array_equal(out, parse_cigar(want[0])), (rec, out)
            assert changed == (want[0] != cig)
    assert lib.fr_clean_length(_p(ref_len, I32P), 1, 1) == 0 and lib.fr_clean_length(_p(ref_len, I32P), 1, -1) == 0


def test_clean_cigar_at_the_28_bit_limit(lib):
    """One operation xM at POS 901 on a reference of 1000: End = 900 + x > 1000; clipFrom = 1000 - 901 + 1 = 100 -> 99; the operation
    ends at x >= 99 with relative position 99: 99M, then S of ReadLength + clipFrom = x + 99.  x = 2^28 - 100 gives S of 2^28 - 1, the
    largest length the field holds; x = 2^28 - 99 gives 2^28: -2."""
    top = (1 << 28) - 1
    n, out, changed = _clean(lib, [((top - 99) << 4) | 0], 0, 901, 1000)
    assert n == 2 and changed and out.tolist() == [(99 << 4) | 0, (top << 4) | 4]
    assert _clean(lib, [((top - 98) << 4) | 0], 0, 901, 1000)[0] == -2


def _oracle_clean(ops, flag, pos, refid, ref_len):
    """oracle.simple_filters.clean_sam on the one record: the new ops, or -1 where it raises the reference's panic, or -2 where the
    clip's length is negative - a number no CIGAR field holds, which numpy refuses to store in the uint32 column (OverflowError)"""
    b = batch_from_records([dict(qname="r", flag=flag, refid=refid, pos=pos, mapq=9, cigar=np.asarray(ops, np.uint32), rgid=0)])
    try:
        out, changed = sf.clean_sam(b, ref_len)
    except ValueError:
        return -1, None
    except OverflowError:
        return -2, None
    return out.cigar.copy(), bool(changed)


def test_clean_cigar_sweep_against_the_oracle(lib):
    """4000 CIGARs of 1..6 operations over all nine operators, zero-length operations included, on a reference of 100 bases (contig
    0; refid -1 and 1 have none: length 0), with POS placing End three bases in front of LN .. far behind it, and anywhere."""
    rng = np.random.default_rng(20240611)
    ref_len = np.array([100], np.int32)
    seen = dict(same=0, clipped=0, panics=0, negative=0, unmapped=0, no_ref=0)
    for k in range(4000):
        nop = int(rng.integers(1, 7))
        lens = np.where(rng.random(nop) < 0.15, 0, rng.integers(1, 31, nop))
        ops = ((lens.astype(np.uint32) << 4) | rng.integers(0, 9, nop).astype(np.uint32)).astype(np.uint32)
        span = int(sum(int(c) >> 4 for c in ops if (int(c) & 15) in sf.CONSUMES_REF))
        if k % 3 == 0:
            pos = int(rng.integers(0, 160))
        else:
            pos = max(0, 100 + int(rng.choice([-3, -1, 0, 1, 2, 5, 17, 40])) - span + 1)  # End = LN + d
        flag = int(rng.choice([0, 0, 0, 0x10, 0x4, 0x400]))
        refid = int(rng.choice([0, 0, 0, 0, -1, 1]))
        want, want_changed = _oracle_clean(ops, flag, pos, refid, ref_len)
        n, out, changed = _clean(lib, ops, flag, pos, lib.fr_clean_length(_p(ref_len, I32P), 1, refid))
        if isinstance(want, int):
            assert n == want, (ops, flag, pos, refid)
            seen["panics" if want == -1 else "negative"] += 1
        else:
            assert n == want.size and np.array_equal(out, want) and changed == want_changed, (ops, flag, pos, refid, out, want)
            seen["clipped" if changed else "same"] += 1
            seen["unmapped"] += bool(flag & 4)
            seen["no_ref"] += refid != 0 and changed
    assert min(seen.values()) >= 20, seen


# ---- overlap, record_rejected

REGIONS = [[], [(100, 200)], [(100, 200), (300, 400)]]  # contigs with 0, 1 and 2 intervals
N_REF = len(REGIONS)
MIN_MAPQ = 30


def _flat_regions():
    flat = np.array([v for iv in REGIONS for se in iv for v in se] + [0, 0], np.int32)
    off = np.cumsum([0] + [len(iv) for iv in REGIONS]).astype(np.int64)
    return flat, off


def test_overlap_against_the_oracle(lib):
    """intervals.Overlap on tables of 0, 1 and 2 intervals, for every (start, end) around each Start and End and for end < start."""
    edges = [0, 1, 99, 100, 101, 102, 199, 200, 201, 202, 299, 300, 301, 302, 399, 400, 401, 402, 1000]
    for iv in REGIONS + [[(5, 5)], [(1, 2), (2, 3), (3, 4)]]:
        a = np.array([v for se in iv for v in se] + [0, 0], np.int32)
        for s, e in itertools.product(edges + [4, 5, 6, 2, 3], repeat=2):
            assert bool(lib.fr_overlap(_p(a, I32P), len(iv), s, e)) == sf.overlap(iv, s, e), (iv, s, e)


def _edge_records():
    """FLAG with and without 0x4 and 0x400, POS 0, refid -1 and N_REF, MAPQ around the bound, the empty CIGAR and non-exact ones; then
    reads of 50 reference bases that end one base before, on and after every interval's Start and start one before, on and after its
    End (with 50M: End() = POS + 49), mapped and unmapped (an unmapped read's end is its POS)"""
    recs = []
    cigars = [[], parse_cigar("50M"), parse_cigar("10S40M"), parse_cigar("20M5I20M"), parse_cigar("0M"), parse_cigar("20M10D20M"), parse_cigar("5H45M")]
    for flag, pos, refid, mapq, cig in itertools.product([0, 0x4, 0x400, 0x404], [0, 150], [-1, 0, 1, 2, N_REF], [0, MIN_MAPQ - 1, MIN_MAPQ, 255], cigars):
        recs.append((flag, pos, refid, mapq, cig))
    for refid in range(N_REF):
        for start_or_end in (100, 200, 300, 400):
            for d in (-1, 0, 1):
                recs.append((0, start_or_end + d - 49, refid, 60, parse_cigar("50M")))   # ends at the edge + d
                recs.append((0, start_or_end + d, refid, 60, parse_cigar("50M")))        # starts at the edge + d
                recs.append((0x4, start_or_end + d, refid, 60, parse_cigar("50M")))
    return recs


def test_record_rejected_against_keep_mask(lib):
    """The cross product of the six switches (min_mapq 0, a bound, and 256: everything rejected) on the edge records.  A refid the
    header does not hold has no intervals (ivals[name] is nil in the reference): the oracle's table gets an empty row for it.  The
    fetchers run only where the rule reads them: MAPQ under a bound of 1..255, the CIGAR on records the four fixed-field predicates kept
    when the exact-mapping or the region predicate is selected."""
    recs = _edge_records()
    cig_off = np.cumsum([0] + [len(r[4]) for r in recs]).astype(np.uint64)
    b = SimpleNamespace(n=len(recs), flag=np.array([r[0] for r in recs], np.uint16), pos=np.array([r[1] for r in recs], np.int32),
                        refid=np.array([r[2] for r in recs], np.int32), mapq=np.array([r[3] for r in recs], np.uint8), cigar_off=cig_off,
                        cigar=np.concatenate([np.asarray(r[4], np.uint32) for r in recs]))
    flat, off = _flat_regions()
    cigs = [np.ascontiguousarray(np.asarray(r[4], np.uint32)) for r in recs]
    rejected = 0
    for ru, rus, mq, rne, rd, reg in itertools.product([0, 1], [0, 1], [0, MIN_MAPQ, 256], [0, 1], [0, 1], [0, 1]):
        fixed = dict(remove_unmapped=bool(ru), remove_unmapped_strict=bool(rus), min_mapq=mq, remove_duplicates=bool(rd))
        want = sf.keep_mask(b, remove_non_exact=bool(rne), regions=(REGIONS + [[]]) if reg else None, **fixed)
        kept_by_fixed = sf.keep_mask(b, **fixed)
        sw = (C.c_int * 6)(ru, rus, mq, rne, rd, reg)
        for i, (flag, pos, refid, mapq, _) in enumerate(recs):
            fetched = (C.c_int * 2)(0, 0)
            got = lib.fr_record_rejected(sw, flag, refid, pos, mapq, _p(cigs[i], U32P), cigs[i].size, N_REF, _p(flat, I32P), _p(off, I64P), fetched)
            assert bool(got) == (not want[i]), (ru, rus, mq, rne, rd, reg, recs[i])
            assert fetched[0] == (1 if 0 < mq <= 255 else 0) and fetched[1] == (1 if kept_by_fixed[i] and (rne or reg) else 0), (fetched[:], recs[i])
            rejected += bool(got)
    assert 0 < rejected < 96 * len(recs)


# ---- the strict rule

def _bam_record(fields):
    """a record of three bases, one CIGAR operation and the name "r", with these optional fields"""
    body = struct.pack("<iiBBHHHIiii", 0, 99, 2, 60, 4680, 1, 0, 3, -1, -1, 0) + b"r\0" + struct.pack("<I", (3 << 4) | 0) + b"\x12\x40" + b"\x1e\x1e\x1e"
    return tagref.with_fields(struct.pack("<I", len(body)) + body, fields)


KEYS = (b"X0", b"X1", b"XM", b"XO", b"XG")
GOOD = [tagref.int_field(k, b"C", 1 if k == b"X0" else 0) for k in KEYS]
VERDICT = {"keep": 0, "reject": 1, "panics": 2}


def _strict(L, fields):
    rec = _bam_record(fields)
    assert tagref.parse_fields(rec) == list(fields)
    got = L.fr_strict(rec)
    assert got == VERDICT[tagref.strict_keep(rec)], fields
    return got


def test_strict_rule_against_tagref(lib):
    """Each of the five keys missing, wrong-valued, present twice (the first decides) and no integer - alone, and with another key that
    rejects in front of it (reject) or behind it (panics); every integer type; a Z and a B field between the keys; no fields at all."""
    z, barr = (b"ZZ", b"Z", b"X0 X1\0"), (b"BB", b"B", b"S" + struct.pack("<I", 3) + b"\1\0\2\0\3\0")
    seen = set()
    seen.add(_strict(lib, GOOD))
    seen.add(_strict(lib, []))
    seen.add(_strict(lib, [z, barr]))
    for w, key in enumerate(KEYS):
        ok = 1 if w == 0 else 0
        others = lambda: [f for f in GOOD if f[0] != key]
        seen.add(_strict(lib, others()))                                                       # missing
        for ty, bad in ((b"C", ok + 1), (b"c", -1), (b"S", 256), (b"s", -32768), (b"I", 1 << 31), (b"i", -(1 << 31))):
            wrong = tagref.int_field(key, ty, bad)
            seen.add(_strict(lib, GOOD[:w] + [wrong] + GOOD[w + 1:]))                          # wrong-valued, in every integer type
            seen.add(_strict(lib, GOOD[:w] + [tagref.int_field(key, ty, ok)] + GOOD[w + 1:]))  # right-valued in that type
            seen.add(_strict(lib, GOOD + [wrong]))                                             # twice: the first (good) decides
            seen.add(_strict(lib, [wrong] + GOOD))                                             # twice: the first (wrong) decides
        for no_int in ((key, b"Z", b"%d\0" % ok), (key, b"A", b"%d" % ok), (key, b"f", struct.pack("<f", ok)), (key, b"H", b"00\0"),
                       (key, b"B", b"C" + struct.pack("<I", 1) + bytes([ok]))):
            one = GOOD[:w] + [no_int] + GOOD[w + 1:]
            assert _strict(lib, one) == 2
            assert _strict(lib, [z] + one[:3] + [barr] + one[3:]) == 2
            assert _strict(lib, [no_int] + GOOD) == 2 and _strict(lib, GOOD + [no_int]) == 0   # twice: the first decides
            for v, other in enumerate(KEYS):
                if v == w:
                    continue
                wrong_other = [tagref.int_field(other, b"C", 7) if f[0] == other else f for f in one]
                missing_other = [f for f in one if f[0] != other]
                for fields in (wrong_other, missing_other, list(reversed(wrong_other)), [z] + missing_other + [barr]):
                    assert _strict(lib, fields) == (1 if v < w else 2), fields              # the ORDER OF THE KEYS decides, not of the fields
    for perm in itertools.permutations(range(5)):
        assert _strict(lib, [z] + [GOOD[k] for k in perm[:2]] + [barr] + [GOOD[k] for k in perm[2:]]) == 0
    assert seen == {0, 1}


# ---- split_route, merge_upper_bound

def test_split_route_against_split_records(lib):
    """Every (refid, next_refid) of -1 .. n_ref + 1 for n_ref = 0, 1, 4 and group tables with equal and different groups.  A refid
    the header does not hold routes like "*" (group 0) but still counts as mapped in the spread test; the oracle, which indexes the table,
    gets zeros behind the table's end for them."""
    for gof in ([], [1], [1, 1, 2, 3], [2, 1, 2, 1]):
        n_ref = len(gof)
        ids = list(range(-1, n_ref + 2))
        pairs = list(itertools.product(ids, ids))
        b = SimpleNamespace(n=len(pairs), refid=np.array([p[0] for p in pairs], np.int32), next_refid=np.array([p[1] for p in pairs], np.int32))
        split, spread = sf.split_records(b, gof + [0, 0])
        table = np.array(gof + [77, 77], np.int32)  # (entries behind n_ref must not be read)
        for i, (r, nr) in enumerate(pairs):
            g = C.c_int32(-5)
            sp = lib.fr_split_route(r, nr, _p(table, I32P), n_ref, C.byref(g))
            assert (g.value, sp) == (int(split[i]), int(spread[i])), (gof, r, nr)


def test_merge_key_and_upper_bound_against_merge_slots(lib):
    """merge_key by hand: refid in the high word, POS in the low one, refid -1 behind every contig.  Then slot j = merge_upper_bound(kg,
    key j) + j against the merge loop: empty groups, empty spread, runs of equal keys on both sides, unmapped reads, random lists."""
    assert lib.fr_merge_key(0, 0) == 0 and lib.fr_merge_key(1, 2) == (1 << 32) | 2 and lib.fr_merge_key(-1, 0) == 0xFFFFFFFF00000000
    assert lib.fr_merge_key(0x7FFFFFFF, 0x7FFFFFFF) == 0x7FFFFFFF7FFFFFFF < lib.fr_merge_key(-1, 0) and lib.fr_merge_key(3, -1) == 0x3FFFFFFFF
    rng = np.random.default_rng(7)
    cases = [([], []), ([], [(0, 1), (0, 1), (-1, 0)]), ([(0, 1), (2, 5)], []), ([(0, 5)] * 4, [(0, 5)] * 3), ([(0, 5)] * 4, [(0, 4), (0, 5), (0, 6)]),
             ([(0, 1), (1, 1), (-1, 0), (-1, 0)], [(0, 0), (1, 1), (1, 2), (-1, 0), (-1, 0)])]
    for _ in range(40):
        mk = lambda n: sorted(((int(r), int(p)) for r, p in zip(rng.integers(-1, 3, n), rng.integers(0, 6, n))), key=lambda k: (k[0] & 0xFFFFFFFF, k[1]))
        cases.append((mk(int(rng.integers(0, 30))), mk(int(rng.integers(0, 30)))))
    for gk, sk in cases:
        kg = np.array([lib.fr_merge_key(r, p) for r, p in gk] + [0], np.uint64)  # (a word behind the keys that sorts in front of all)
        got = [lib.fr_merge_upper_bound(_p(kg, U64P), len(gk), lib.fr_merge_key(r, p)) + j for j, (r, p) in enumerate(sk)]
        want = sf.merge_slots([(r & 0xFFFFFFFF, p) for r, p in gk], [(r & 0xFFFFFFFF, p) for r, p in sk])
        assert got == want.tolist(), (gk, sk)


# ---- the layouts of scratch slot 5 and the grids

def _check_parts(parts, total, eight):
    """parts: name -> (offset, bytes)"""
    for name, (at, size) in parts.items():
        assert at + size <= total, (name, parts, total)
        if name in eight:
            assert at % 8 == 0, (name, parts)
    for (a, (a0, an)), (b, (b0, bn)) in itertools.combinations(parts.items(), 2):
        assert a0 + an <= b0 or b0 + bn <= a0, (a, b, parts)


def test_region_layout(lib):
    """pool | pointer table | counts.  By hand, with today's total * 8 + n_ref * 16 + 64 and pointers at the pool's end rounded up to
    16: 1 interval, 3 contigs -> 8 + 48 + 64 = 120 bytes, pointers at 16, counts at 16 + 24 = 40; nothing at all -> 64, 0, 0."""
    out = (C.c_uint64 * 4)()
    lib.fr_region_layout(C.c_uint64(1), 3, out)
    assert out[:] == [0, 16, 40, 120]
    lib.fr_region_layout(C.c_uint64(0), 0, out)
    assert out[:] == [0, 0, 0, 64]
    for n_ref, total in itertools.product(range(6), (0, 1, 2, 3, 1000)):
        lib.fr_region_layout(C.c_uint64(total), n_ref, out)
        assert out[3] == total * 8 + n_ref * 16 + 64
        _check_parts(dict(pool=(out[0], total * 8), ptr=(out[1], n_ref * 8), cnt=(out[2], n_ref * 8)), out[3], {"ptr", "cnt"})


def test_classify_layout(lib):
    """group_of_ref | counts | split | spread.  By hand, with today's n_ref * 4 + (n_groups + 2) * 8 + n * 3 + 64, the counts at the
    table's end rounded up to 16, the split ids behind them and the spread bytes behind n + 8 split ids: one record, one contig, one group
    -> 4 + 24 + 3 + 64 = 95 bytes, counts at 16, split at 40, spread at 40 + 18 = 58; 257 records, 5 contigs, 8000 groups ->
    20 + 64016 + 771 + 64 = 64871 bytes, counts at 32, split at 64048, spread at 64048 + 530 = 64578."""
    out = (C.c_uint64 * 6)()
    lib.fr_classify_layout(C.c_uint64(1), 1, 1, out)
    assert out[:] == [0, 16, 40, 58, 95, 3]
    lib.fr_classify_layout(C.c_uint64(257), 5, 8000, out)
    assert out[:] == [0, 32, 64048, 64578, 64871, 8002]
    for n_ref, n_groups, n in itertools.product(range(6), (0, 1, 8000), (0, 1, 257)):
        lib.fr_classify_layout(C.c_uint64(n), n_ref, n_groups, out)
        nc = n_groups + 2
        assert out[4] == n_ref * 4 + nc * 8 + n * 3 + 64 and out[5] == nc
        _check_parts(dict(gof=(out[0], n_ref * 4), counts=(out[1], nc * 8), split=(out[2], (n + 8) * 2), spread=(out[3], n)), out[4], {"counts"})


def test_dictionary_layout_and_grids(lib):
    """counters | map: n_old * 4 + 64 bytes, two 64-bit counters in front, the map at 16 - no contigs: 64; five: 84.  The grids by hand:
    clear_duplicate_flag max(1, min(ceil(ceil(n / 8) / 256), 8 n_cu)), the dictionary max(1, min(ceil(n / 256), 16 n_cu)), classify
    min(ceil(n / 256), 2048)."""
    out = (C.c_uint64 * 3)()
    lib.fr_dictionary_layout(0, out)
    assert out[:] == [0, 16, 64]
    lib.fr_dictionary_layout(5, out)
    assert out[:] == [0, 16, 84]
    for n_old in range(6):
        lib.fr_dictionary_layout(n_old, out)
        _check_parts(dict(counters=(out[0], 16), map=(out[1], n_old * 4)), out[2], {"counters"})
    g = (C.c_uint * 3)()
    for n, n_cu, want in ((0, 256, [1, 1, 0]), (1, 256, [1, 1, 1]), (2048, 256, [1, 8, 8]), (2049, 256, [2, 9, 9]), (256 * 2047, 256, [256, 2047, 2047]),
                          (256 * 2047 + 1, 256, [256, 2048, 2048]), (256 * 5000, 256, [625, 4096, 2048]), (8 * 256 * 3000, 256, [2048, 4096, 2048]),
                          (8 * 256 * 3000, 1, [8, 16, 2048]), (1000, 0, [1, 1, 4]), ((1 << 32) - 1, 304, [2432, 4864, 2048])):
        lib.fr_grids(C.c_uint64(n), n_cu, g)
        assert g[:] == want, (n, n_cu, g[:])


# ---- sanitizers

def test_filter_rules_under_the_sanitizers(tmp_path):
    """tests/filter_rules_asan.cpp: clean_cigar writing into a buffer of exactly the count it returned, the strict walk over records
    whose buffer ends with the record, the layouts.  A program of its own: the sanitizers' runtimes are linked into it where the
    compiler has them as archives, so that nothing has to stand in front of them in the list of libraries."""
    src = os.path.join(ROOT, "tests", "filter_rules_asan.cpp")
    exe = str(tmp_path / "filter_rules_asan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src]
    if subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "filter_rules_asan: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (
        r.returncode, r.stdout, r.stderr[-2000:])
