"""GPU tests of elp_sw_align / elp_sw_align_reads (elprep_amd/csrc/sw.hip): every result bit for bit against tests/swref_c.c, the C
restatement of runSmithWaterman (filters/sw.go:110-316), on the smallest shapes at which each mechanism of the kernels can go wrong - the
lanes' strips and the tiles of 256 columns, the sweep's fill and drain, the order of the ties, the end search, the shortcut, gaps and
diagonal runs across the traceback's 64-cell fetch, the clamp, the assembly, batches and chunks, staged reads, refusals.  Every test
runs on a fresh and on a reused context (tests/conftest.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch
from elprep_amd.engine import ElpError, Engine
from tests import sw_cases, swref
from tools import synth

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5
CFG = synth.config("tiny")
H = CFG.header()


def _engine():
    return Engine(H, 0)


def _run(e, case):
    return e.sw_align(case.refs, case.alts, case.ref_of, case.alt_of, case.params, case.strategy)


def _check(e, case, want=None):
    got = _run(e, case)
    want = want or sw_cases.expected(case)
    for g, w, what in zip(got, want, ("cigar_off", "cigar", "offset")):
        if not np.array_equal(g, w):
            m = min(len(g), len(w))
            bad = np.flatnonzero(np.asarray(g[:m]) != np.asarray(w[:m]))
            raise AssertionError("%s: %s differs (%d entries against %d), first at %s" % (case.name, what, len(g), len(w), bad[:1]))


def _check_all(cases):
    e = _engine()
    try:
        for case in cases:
            _check(e, case)
    finally:
        e.close()


def test_lanes_and_strips(engine_mode):
    """alternate lengths 1, 2, 63, 64, 65, 127, 128, 129 and 255, 256, 257, 513 (tile width 256) x reference lengths 1, 2, 63, 64, 65, 130,
    two letters and ACGT, every strategy and parameter set"""
    _check_all(sw_cases.lanes_and_strips())


def test_tie_order_end_search_and_assembly(engine_mode):
    _check_all(sw_cases.tie_order() + sw_cases.end_search() + sw_cases.assembly() + sw_cases.small_random())


def test_shortcut(engine_mode):
    _check_all(sw_cases.shortcut())


def test_gaps_and_runs(engine_mode):
    _check_all(sw_cases.gaps_and_runs())


def test_clamp(engine_mode):
    """leadingIndel with gap_extend = -60000 on 2000 x 2000: the first row and column pass -100000000 unclamped (-110 - 1999 * 60000 =
    -119940110), the interior is clamped"""
    rng = np.random.default_rng(9)
    ref = sw_cases.rand_seq(rng, 2000)
    alt = bytearray(ref)
    for at in rng.integers(0, 2000, 50):
        alt[int(at)] = ord("A")
    _check_all([sw_cases._pairs("clamp", [(ref, bytes(alt))], (25, -50, -110, -60000), swref.LEADING_INDEL)])


def test_batches(engine_mode):
    """n = 0, 1, 65 and 5000 problems with shared references and shared alternates"""
    big = sw_cases.mixed_batch()
    e = _engine()
    try:
        for n in (0, 1, 65):
            _check(e, big._replace(name="mixed %d" % n, ref_of=big.ref_of[:n], alt_of=big.alt_of[:n]))
        _check(e, big)
        off, cig, o = e.sw_align([], [], [], [], swref.P1, swref.SOFTCLIP)
        assert off.tolist() == [0] and cig.size == 0 and o.size == 0
    finally:
        e.close()


def _launches(e, name):
    return e.profile().get(name, (0, 0.0))[0]


def test_chunks_under_a_small_scratch_budget(engine_mode):
    """sw_scratch_bytes = 60000: a 60 x 45 problem takes (60 + 11) * 12 * 4 cells of 2 bytes + 110 words = 7256 bytes (sw_plan.hpp:
    sw_need), the largest here, 120 x 60, (120 + 14) * 15 * 4 * 2 + 184 * 4 = 16816 - so the problems that miss the shortcut run in dozens of chunks; problem 100 is 400 x 300
    (two tiles: (400 + 63) * 256 + (400 + 10) * 11 * 4 cells = 273136 bytes of backtrack alone), larger than the budget - a chunk of
    its own.  The results equal the one-chunk run's."""
    case = sw_cases.mixed_batch(300, 8)
    rng = np.random.default_rng(3)
    ref = sw_cases.rand_seq(rng, 400)
    case.refs.append(ref)
    case.alts.append(sw_cases.derived(rng, ref, 300))
    case.ref_of[100], case.alt_of[100] = len(case.refs) - 1, len(case.alts) - 1
    want = sw_cases.expected(case)
    e = _engine()
    try:
        e.profile_enable(True)
        e.profile_reset()
        _check(e, case, want)
        assert _launches(e, "sw_dp") == 1
        e.set_tuning("sw_scratch_bytes", 60000)
        e.profile_reset()
        _check(e, case, want)
        assert _launches(e, "sw_dp") >= 3
        e.profile_enable(False)
    finally:
        e.set_tuning("sw_scratch_bytes", 0)
        e.close()


def test_all_hit_and_none_hit(engine_mode):
    """a batch in which every problem hits the shortcut runs no DP kernel; one in which none does runs no problem twice"""
    rng = np.random.default_rng(11)
    refs = [sw_cases.rand_seq(rng, 200) for _ in range(5)]
    hits = [refs[k % 5][k % 50:k % 50 + 100] for k in range(200)]
    e = _engine()
    try:
        e.profile_enable(True)
        e.profile_reset()
        _check(e, sw_cases.Case("all hit", refs, hits, np.arange(200) % 5, np.arange(200), swref.P1, swref.SOFTCLIP))
        assert _launches(e, "sw_dp") == 0 and _launches(e, "sw_shortcut") == 1
        e.profile_reset()
        _check(e, sw_cases.Case("none hits", refs, hits, (np.arange(200) + 1) % 5, np.arange(200), swref.P1, swref.IGNORE))
        assert _launches(e, "sw_dp") == 1
        e.profile_enable(False)
    finally:
        e.close()


# ---- staged reads
NIBBLES = b"=ACMGRSVTWYHKDBN"


def _read_set():
    """synthetic reads whose SEQ holds every nibble code; every seventh read is cut to one base, the two behind it by two bases and by one: odd and even lengths"""
    b = synth.generate(CFG, 0, 150)
    rng = np.random.default_rng(21)
    l_seq, cig, seq, qual = [], [], [], []
    for i in range(b.n):
        ops = b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])]
        L = int(b.l_seq[i])
        if i % 7 == 0:
            L = 1
        elif i % 7 == 1:
            L -= 2
        elif i % 7 == 2:
            L -= 1
        if L != int(b.l_seq[i]) and ops.size:
            ops = np.array([(L << 4) | 0], dtype=np.uint32)
        nib = rng.integers(0, 16, L + (L & 1)).astype(np.uint8)
        if L & 1:
            nib[-1] = 0
        l_seq.append(L)
        cig.append(ops)
        seq.append((nib[0::2] << 4) | nib[1::2])
        qual.append(b.qual[int(b.qual_off[i]):int(b.qual_off[i]) + L])
    cols = {k: getattr(b, k) for k in ("refid", "pos", "next_refid", "pnext", "tlen", "flag", "mapq", "rgid", "has_sr", "qname_off", "qname", "split")}
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    return Batch(l_seq=np.asarray(l_seq, np.uint32), cigar_off=off(cig), cigar=np.concatenate(cig).astype(np.uint32), seq_off=off(seq), seq4=np.concatenate(seq),
                 qual_off=off(qual), qual=np.concatenate(qual), **cols)


def test_staged_reads(engine_mode):
    """elp_sw_align_reads equals elp_sw_align on the decoded strings (odd and even lengths, length 1, all sixteen codes; read_idx with
    repeats, in no order), leaves FLAG, QUAL, the permutation and elp_num_sorted alone, and the context still sorts and marks as the oracle"""
    b = _read_set()
    assert {int(v) for v in b.l_seq} >= {1} and any(int(v) % 2 for v in b.l_seq) and any(int(v) % 2 == 0 for v in b.l_seq)
    strings = [b.seq_of(i).encode() for i in range(b.n)]
    assert set(b"".join(strings)) == set(NIBBLES)
    rng = np.random.default_rng(5)
    refs = [sw_cases.rand_seq(rng, int(rng.integers(40, 90)), NIBBLES + b"acgtn") for _ in range(6)] + [strings[2] + b"AC", b"GG" + strings[9].replace(b"R", b"r")]
    read_idx = np.concatenate([rng.integers(0, b.n, 400), [0, 0, b.n - 1, 7, 7]]).astype(np.uint32)
    ref_of = rng.integers(0, len(refs), read_idx.size).astype(np.uint32)
    ref_of[-3:] = [6, 7, 6]
    e = _engine()
    try:
        e.set_read_group_ids(H.rg_ids)
        e.stage_bam(orc.bam_encode(b, H.rg_ids))
        e.mark_duplicates(True)
        perm, flags, qual, n_sorted = e.sort_coordinate(), e.flags(), e.qual(), e.n_sorted
        for strategy in sw_cases.STRATEGIES:
            got = e.sw_align_reads(refs, ref_of, read_idx, swref.P1, strategy)
            want = sw_cases.expected(sw_cases.Case("reads", refs, strings, ref_of, read_idx, swref.P1, strategy))
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
            same = e.sw_align(refs, strings, ref_of, read_idx, swref.P1, strategy)
            for g, w in zip(got, same):
                assert np.array_equal(g, w)
        assert np.array_equal(e.permutation(), perm) and np.array_equal(e.flags(), flags) and np.array_equal(e.qual(), qual) and e.n_sorted == n_sorted
        with pytest.raises(ElpError) as ei:
            e.sw_align_reads(refs, [0], [b.n], swref.P1, swref.SOFTCLIP)
        assert ei.value.code == ERR_ARG
        oflags = orc.mark_duplicates(b, H)
        assert np.array_equal(e.mark_duplicates(True), oflags)
        assert np.array_equal(e.sort_coordinate(), orc.sort_coordinate(b, oflags))
    finally:
        e.close()


def test_column_staged_reads_are_refused(engine_mode):
    """column staging keeps A, C, G, T and "other" of SEQ: the strings are not there, ELP_ERR_ARG"""
    e = _engine()
    try:
        e.stage(synth.generate(CFG, 0, 20))
        with pytest.raises(ElpError) as ei:
            e.sw_align_reads([b"ACGT"], [0], [0], swref.P1, swref.SOFTCLIP)
        assert ei.value.code == ERR_ARG
    finally:
        e.close()


# ---- refusals
def test_refusals(engine_mode):
    """length 0 and 4096, a parameter of 65536, strategy 4, an index outside a pool, a cigar_cap one short; after each the next valid call
    on the context is correct"""
    good = sw_cases._pairs("good", [(b"ACGTACGTTTGACCAGTACA", b"ACGTACGTACCAGTACA"), (b"ACG", b"TACGT")], swref.P2, swref.LEADING_INDEL)
    want = sw_cases.expected(good)
    long_ok, too_long = b"A" * 4095, b"A" * 4096
    bad = [
        (sw_cases._pairs("empty alternate", [(b"ACGT", b"")], swref.P1, swref.SOFTCLIP), ERR_ARG),
        (sw_cases._pairs("empty reference", [(b"", b"ACGT")], swref.P1, swref.INDEL), ERR_ARG),
        (sw_cases._pairs("4096", [(too_long, b"ACGT")], swref.P1, swref.SOFTCLIP), ERR_UNSUPPORTED),
        (sw_cases._pairs("4096 alt", [(b"ACGT", too_long)], swref.P1, swref.SOFTCLIP), ERR_UNSUPPORTED),
        (sw_cases._pairs("65536", [(b"ACGT", b"ACGA")], (65536, -1, -1, -1), swref.SOFTCLIP), ERR_UNSUPPORTED),
        (sw_cases._pairs("-65536", [(b"ACGT", b"ACGA")], (1, -1, -65536, -1), swref.SOFTCLIP), ERR_UNSUPPORTED),
        (sw_cases._pairs("strategy 4", [(b"ACGT", b"ACGA")], swref.P1, 4), ERR_ARG),
        (sw_cases.Case("ref_of", [b"ACGT"], [b"ACGA"], [1], [0], swref.P1, swref.SOFTCLIP), ERR_ARG),
        (sw_cases.Case("alt_of", [b"ACGT"], [b"ACGA"], [0], [1], swref.P1, swref.SOFTCLIP), ERR_ARG),
    ]
    e = _engine()
    try:
        _check(e, sw_cases._pairs("4095", [(long_ok, b"ACGT"), (b"ACGT", long_ok)], swref.P1, swref.INDEL))
        _check(e, sw_cases._pairs("65535", [(b"ACGTAC", b"ACTTAC")], (65535, -65535, -65535, -65535), swref.INDEL))
        for case, code in bad:
            with pytest.raises(ElpError) as ei:
                _run(e, case)
            assert ei.value.code == code, case.name
            _check(e, good, want)
        # a cigar_cap one short: ELP_ERR_ARG with the need, and the same call with that cap succeeds
        a, a_off = sw_cases.flat_pool(good.refs)
        b, b_off = sw_cases.flat_pool(good.alts)
        idx = np.arange(2, dtype=np.uint32)
        need_ops = int(want[0][-1])
        for cap, rc_want in ((need_ops - 1, ERR_ARG), (need_ops, 0)):
            cig, coff, off, need = np.zeros(need_ops, np.uint32), np.zeros(3, np.uint64), np.zeros(2, np.int32), C.c_uint64()
            rc = e.L.elp_sw_align(e.h, 2, a.ctypes.data, a_off.ctypes.data, 2, b.ctypes.data, b_off.ctypes.data, 2, idx.ctypes.data, idx.ctypes.data, *good.params,
                                  good.strategy, cig.ctypes.data, cap, coff.ctypes.data, off.ctypes.data, C.byref(need))
            assert rc == rc_want and need.value == need_ops
        assert np.array_equal(coff, want[0]) and np.array_equal(cig, want[1]) and np.array_equal(off, want[2])
        _check(e, good, want)
    finally:
        e.close()
