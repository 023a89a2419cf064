"""Case lists for the Smith-Waterman operator, shared by the CPU emulation of its kernels (tests/test_sw_core_cpu.py) and the GPU tests
(tests/test_gpu_sw.py), and the loader of the C restatement (tests/swref_c.c) that gives every case its expected value.

A case is a `Case`: two pools of sequences, the index pairs, the four parameters and the strategy - the flat form of elp_sw_align.
Every list is made from fixed seeds, so the two users see the same problems."""
import ctypes as C
import os
import subprocess
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import swref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "libswref_c.so")
TILE = 256  # columns of one sweep of the wave: 64 lanes x 4 columns (sw_plan.hpp SW_TILE)
STRATEGIES = (swref.SOFTCLIP, swref.INDEL, swref.LEADING_INDEL, swref.IGNORE)
PARAMS = (swref.P1, swref.P2, swref.P3)

Case = namedtuple("Case", "name refs alts ref_of alt_of params strategy")

_lib = None


def swref_c():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "swref_c.c")
        if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(src):
            subprocess.check_call(["cc", "-O2", "-std=c11", "-Wall", "-shared", "-fPIC", "-o", SO, src])
        L = C.CDLL(SO)
        L.swref_last_index.restype = C.c_int32
        L.swref_last_index.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32]
        L.swref_run.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32] + [C.c_int32] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
        L.swref_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint64] * 2 + [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_int] + [C.c_void_p] * 4
        _lib = L
    return _lib


def run_c(ref: bytes, alt: bytes, params, strategy):
    """one problem through swref_c: (cigar as [(length, op)], offset)"""
    out = (C.c_uint32 * (len(ref) + len(alt) + 3))()
    off = C.c_int32()
    n = swref_c().swref_run(ref, len(ref), alt, len(alt), *params, strategy, out, C.byref(off))
    assert n >= 0
    return swref.decode(out[:n]), off.value


def flat_pool(seqs):
    """a list of bytes as (bytes, offsets): the pools of elp_sw_align"""
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), off


def expected(case: Case, threads: int = 8):
    """(cigar_off, cigar, offset) of a case by swref_c, as elp_sw_align returns them"""
    return run_batch(swref_c().swref_batch, case, threads)


def run_batch(batch_fn, case: Case, threads: int = 8):
    """a case through a C function of swref_batch's form (tests/swref_c.c; tests/sw_host.cpp has the same)"""
    a, a_off = flat_pool(case.refs)
    b, b_off = flat_pool(case.alts)
    ref_of = np.ascontiguousarray(case.ref_of, dtype=np.uint32)
    alt_of = np.ascontiguousarray(case.alt_of, dtype=np.uint32)
    n = ref_of.size
    la = (a_off[1:] - a_off[:-1])[ref_of] if n else np.zeros(0, np.uint64)
    lb = (b_off[1:] - b_off[:-1])[alt_of] if n else np.zeros(0, np.uint64)
    slot = np.zeros(n + 1, dtype=np.uint64)
    slot[1:] = np.cumsum(la + lb + 3, dtype=np.uint64)
    raw = np.zeros(int(slot[-1]) + 1, dtype=np.uint32)
    n_ops = np.zeros(n, dtype=np.uint32)
    offset = np.zeros(n, dtype=np.int32)
    a_p, b_p = np.concatenate([a, np.zeros(1, np.uint8)]), np.concatenate([b, np.zeros(1, np.uint8)])  # (never empty arrays)

    def part(k0, k1):
        return batch_fn(a_p.ctypes.data, a_off.ctypes.data, b_p.ctypes.data, b_off.ctypes.data, k0, k1, ref_of.ctypes.data, alt_of.ctypes.data,
                             *case.params, case.strategy, raw.ctypes.data, slot.ctypes.data, n_ops.ctypes.data, offset.ctypes.data)
    if n:
        threads = max(1, min(threads, n))
        cuts = [n * t // threads for t in range(threads + 1)]
        with ThreadPoolExecutor(threads) as ex:
            assert all(r == 0 for r in ex.map(lambda t: part(cuts[t], cuts[t + 1]), range(threads)))
    cigar_off = np.zeros(n + 1, dtype=np.uint64)
    cigar_off[1:] = np.cumsum(n_ops, dtype=np.uint64)
    cigar = np.zeros(int(cigar_off[-1]), dtype=np.uint32)
    for k in range(n):
        cigar[int(cigar_off[k]):int(cigar_off[k + 1])] = raw[int(slot[k]):int(slot[k]) + int(n_ops[k])]
    return cigar_off, cigar, offset


# ---- sequences
def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n).tolist())


def derived(rng, ref: bytes, n: int, alphabet=b"ACGT"):
    """`n` bytes that follow a stretch of `ref` with a few substitutions and one indel: an alignment with long diagonal runs"""
    start = int(rng.integers(0, max(len(ref) - n, 0) + 1))
    s = bytearray(ref[start:start + n])
    for _ in range(int(rng.integers(0, 4))):
        if s:
            s[int(rng.integers(0, len(s)))] = int(rng.choice(np.frombuffer(alphabet, dtype=np.uint8)))
    if len(s) > 4 and rng.random() < 0.7:
        at, g = int(rng.integers(1, len(s) - 1)), int(rng.integers(1, 6))
        if rng.random() < 0.5:
            del s[at:at + g]
        else:
            s[at:at] = rand_seq(rng, g, alphabet)
    while len(s) < n:
        s += rand_seq(rng, n - len(s), alphabet)
    return bytes(s[:n])


def _pairs(name, pairs, params, strategy):
    refs, alts = [p[0] for p in pairs], [p[1] for p in pairs]
    return Case(name, refs, alts, np.arange(len(pairs), dtype=np.uint32), np.arange(len(pairs), dtype=np.uint32), tuple(params), strategy)


# ---- the lists
ALT_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
REF_LENGTHS = (1, 2, 63, 64, 65, 130)


def lanes_and_strips():
    """every alternate length around the lanes' strips and the tile, crossed with the reference lengths of the sweep's fill and drain; a
    two-letter alphabet (dense ties) and ACGT with the alternate following the reference; one case per strategy and parameter set"""
    rng = np.random.default_rng(20260)
    pairs = []
    for m in REF_LENGTHS:
        for n in ALT_LENGTHS:
            pairs.append((rand_seq(rng, m, b"AC"), rand_seq(rng, n, b"AC")))
            ref = rand_seq(rng, m)
            pairs.append((ref, derived(rng, ref, n)))
    return [_pairs("strips s%d p%d" % (s, pi), pairs, p, s) for s in STRATEGIES for pi, p in enumerate(PARAMS)]


def small_random(n=3000, seed=77):
    """short problems over two letters with small parameters, zero and positive ones among them: every order of the three candidates'
    ties, equal maxima in the last column and in the bottom row, zero-length segments and equal neighbours in the assembly"""
    rng = np.random.default_rng(seed)
    out = []
    for s in STRATEGIES:
        for pi in range(6):
            params = PARAMS[pi] if pi < 3 else tuple(int(v) for v in (rng.integers(-2, 4), rng.integers(-4, 2), rng.integers(-5, 2), rng.integers(-3, 2)))
            pairs = [(rand_seq(rng, int(rng.integers(1, 15)), b"AC"), rand_seq(rng, int(rng.integers(1, 15)), b"AC")) for _ in range(n // 24)]
            out.append(_pairs("small s%d %r" % (s, params), pairs, params, s))
    return out


def tie_order():
    """(0, 0, 0, 0): the three candidates are equal in every cell, the diagonal wins.  (0, -10, 0, 0) on sequences without a common letter:
    right = down = 0 > diagonal, right wins.  A deletion inside matching flanks: down alone wins in the cells under the gap."""
    out = []
    for s in STRATEGIES:
        out.append(_pairs("all equal s%d" % s, [(b"ACCA", b"CAAC"), (b"AAAAAAA", b"CCC"), (b"ACACACACAC" * 7, b"CACA" * 40)], (0, 0, 0, 0), s))
        out.append(_pairs("right = down s%d" % s, [(b"AAAA", b"CCCC"), (b"A" * 70, b"C" * 9), (b"A" * 9, b"C" * 70)], (0, -10, 0, 0), s))
        out.append(_pairs("down alone s%d" % s, [(b"AAGGGAA", b"AAAA"), (b"ACGTACGT" + b"GGGGG" + b"TGCATGCA", b"ACGTACGTTGCATGCA")], swref.P2, s))
    return out


def end_search():
    """equal maxima in the last column (ACCTA ends equally well at row 5 and row 13 of ACGTAGGGACGTA..: the lower row wins), with and without
    rows below it; a bottom row that holds the best score again; leadingIndel leaves the bottom row alone, indel starts at the corner"""
    pairs = [(b"ACGTAGGGACGTA", b"ACCTA"), (b"ACGTAGGGACGTATT", b"ACCTA"), (b"ACGTA", b"ACCTAACCTA"), (b"ACGTAC", b"ACCTACACCTAC"),
             (b"GGACGT", b"ACGTTTTT"), (b"GGACGT", b"TTACGTAC"), (b"CACA", b"ACACACAC"), (b"ACAC", b"CACACACA"), (b"AACC", b"CCAACCAA")]
    return [_pairs("end search s%d p%d" % (s, pi), pairs, p, s) for s in STRATEGIES for pi, p in enumerate(PARAMS)]


def shortcut():
    """the exact-substring shortcut and its misses: several occurrences, one at offset 0 and one at the very end, lower case and IUPAC in
    the reference (hits), lower case and R in the alternate (misses), an alternate longer than the reference; every strategy - under
    indel and leadingIndel the same pairs go through the DP"""
    pairs = [(b"ACGTACGT", b"ACGT"), (b"ACGTTTTT", b"ACGT"), (b"TTTTACGT", b"ACGT"), (b"acgt", b"ACGT"), (b"acgt", b"acgt"), (b"ARGT", b"ANGT"),
             (b"ARGT", b"ARGT"), (b"ACGT", b"ACGTA"), (b"TTACGTACGTACGTAA" * 9, b"ACGTACGT"), (b"nnryACGT", b"NNNNACGT"), (b"ACGT" * 70, b"ACGT" * 33),
             (b"ACGT" * 70, b"CGTA" * 33 + b"C"), (b"ACGT" * 70, b"ACGT" * 33 + b"G"), (b"A", b"A"), (b"A", b"C"), (b"AC*GT", b"AC*GT")]
    return [_pairs("shortcut s%d" % s, pairs, swref.P1, s) for s in STRATEGIES]


def gaps_and_runs():
    """a deletion and an insertion of 300 (a backtrack value beyond a byte); diagonal runs of 63, 64, 65, 128 and 129 cells between two gaps
    (the seams of the traceback's 64-cell fetch); an insertion right behind a deletion; a gap at the first and at the last cell"""
    rng = np.random.default_rng(4242)
    pairs = []
    f0, f1 = rand_seq(rng, 40), rand_seq(rng, 40)
    pairs.append((f0 + rand_seq(rng, 300) + f1, f0 + f1))
    pairs.append((f0 + f1, f0 + rand_seq(rng, 300) + f1))
    for run in (1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130):
        r = rand_seq(rng, run)
        pairs.append((f0 + rand_seq(rng, 10, b"A") + r + f1, f0 + r + rand_seq(rng, 10, b"C") + f1))
        pairs.append((f0 + r + rand_seq(rng, 7, b"G") + f1, f0 + rand_seq(rng, 9, b"T") + r + f1))
    pairs.append((f0 + b"A" * 12 + f1, f0 + b"C" * 12 + f1))
    pairs.append((b"GGG" + f0, f0 + b"TTT"))
    pairs.append((f0 + b"GGG", b"TTT" + f0))
    return [_pairs("gaps s%d p%d" % (s, pi), pairs, p, s) for s in STRATEGIES for pi, p in enumerate(PARAMS)]


def assembly():
    """a soft clip on both sides, its indel form, the folding of `ignore` with a negative offset, an alternate that overhangs the reference
    on either side"""
    pairs = [(b"ACG", b"TACGT"), (b"ACGTACGT", b"GGACGTAC"), (b"ACGTACGT", b"GTACGTCC"), (b"CCACGT", b"TTTTACGTAA"), (b"A", b"C"), (b"A", b"CCCC"),
             (b"AAAA", b"C"), (b"ACGTTGCA", b"TTTTTTTTACGTTGCATTTT"), (b"GATTACA", b"TTACAGG"), (b"GATTACA", b"CCGATT")]
    return [_pairs("assembly s%d p%d" % (s, pi), pairs, p, s) for s in STRATEGIES for pi, p in enumerate(PARAMS)]


def mixed_batch(n=5000, seed=5, n_refs=12, n_alts=700):
    """a batch with shared references (one haplotype for hundreds of reads) and shared alternates, exact copies among them"""
    rng = np.random.default_rng(seed)
    refs = [rand_seq(rng, int(rng.integers(60, 121))) for _ in range(n_refs)]
    alts = []
    for q in range(n_alts):
        ref = refs[q % n_refs]
        ln = int(rng.integers(30, 61))
        alts.append(ref[5:5 + ln] if q % 3 == 0 else derived(rng, ref, ln))
    alt_of = rng.integers(0, n_alts, n).astype(np.uint32)
    ref_of = np.where(rng.random(n) < 0.9, alt_of % n_refs, rng.integers(0, n_refs, n)).astype(np.uint32)
    return Case("mixed %d" % n, refs, alts, ref_of, alt_of, swref.P1, swref.SOFTCLIP)


def core_cases():
    """what the CPU emulation walks"""
    return lanes_and_strips() + small_random(24000) + tie_order() + end_search() + shortcut() + gaps_and_runs() + assembly() + [mixed_batch(300, 6)]
