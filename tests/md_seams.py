"""Read sets that stand on every lane and workgroup seam of mark duplicates' front pass (k_md_front, csrc/markdup.hip).

The kernel's workgroup covers WG = 312 records: wave w, lane l holds record base - 2 + 63 w + l, the neighbour test is one DPP move inside a
wave, its results go through LDS (u = 2 .. 313 are the workgroup's own records, u = 0, 1 and 314 halos) and the pairs' entries go to slots
i >> 1.  A motif of p records, p coprime to 312, repeated 312 times puts every record of the motif once at every phase i mod 312 - on both
sides of every wave seam and of the workgroup seam, and at both parities.  Positions, strands, CIGARs and uniform qualities come from a small
pool per contig, so that many pairs and fragments share keys with different scores and the duplicate flags are not trivial.

Shared by tests/test_md_seams_cpu.py (the read sets are what they claim: oracle only) and tests/test_gpu_md_seams.py (device against oracle).
"""
import functools
import zlib

import numpy as np

import oracle as orc
from elprep_amd.batch import Batch, Header, batch_from_records
from tests.kat_cases import Q20, Q40, _rec

WG = 312                       # MF_RECS
WAVE_SEAMS_U = (62, 125, 188, 251)  # u of the last record a wave tests against its lane 63 (phase = u - 2)
MAX_QNAME = 1000               # elp_ctx::MAX_QNAME (csrc/common.hpp): the longest name the staging call accepts
# mask regimes of the name comparison (8, 16, 24, 32 bytes, then the loop), BAM's longest name and the staging call's
LENGTHS = (3, 7, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 254, MAX_QNAME)
REPS = WG
PREFIX_NS = (1, 2, 3, 4, 62, 63, 64, 65, 310, 311, 312, 313, 314, 315, 623, 624, 625, 626)
PREFIX_L = 33
SHORT_LENGTHS = (1, 2)
SHORT_SLIDES = tuple(range(0, 8)) + tuple(range(306, 319))

# the pool: first ends, mates and a few fragment-only places; the toggling cases' 100 / 300 / 700 are kept out of it (clips included)
POOL_FIRST = (400, 420, 440, 460, 480, 500)
POOL_MATE = (610, 630, 650, 670)
POOL_FRAG_ONLY = (800, 820)
POOL_CIGAR = ("10M", "10M", "3S7M", "7M3S")
POOL_QUAL = (20, 30, 40)

_DIGITS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
_SHORT_ALPHABET = [chr(c) for c in range(33, 127) if chr(c) not in "@:"]  # QNAME's characters, without the tile separator


def header():
    """two contigs, two read groups of two libraries"""
    return Header(ref_len=np.array([2000, 2000], np.int32), rg_lib=np.array([0, 1], np.uint16), rg_cov=np.array([0, 1], np.uint16))


def qname(k: int, L: int, first: str = "Q") -> str:
    """A constant prefix with the counter in the last (at most four) bytes: for L >= 36 two names agree in their first 32 bytes.  k and
    k ^ 1 differ in the last byte only (the base is even)."""
    w = min(L, 4)
    d = ""
    for _ in range(w):
        d = _DIGITS[k % 36] + d
        k //= 36
    assert k == 0
    return (first + "n" * L)[:L - w] + d


class _Names:
    """hands out even counters: k + 1 is the twin that differs in the last byte"""

    def __init__(self, L):
        self.L, self.k = L, 0

    def new(self):
        self.k += 2
        return self.k - 2

    def s(self, k, first="Q"):
        return qname(k, self.L, first)


def _pair(rng, name, name2=None, rg=0, rg2=None, split=0, split2=None):
    """a true pair out of the pool -> [first end, second end]"""
    c = int(rng.integers(0, 2))
    p1, p2 = int(rng.choice(POOL_FIRST)), int(rng.choice(POOL_MATE))
    rev1 = bool(rng.integers(0, 2))
    f1 = 0x1 | 0x2 | 0x40 | (0x10 if rev1 else 0x20)
    f2 = 0x1 | 0x2 | 0x80 | (0x20 if rev1 else 0x10)
    q1, q2 = int(rng.choice(POOL_QUAL)), int(rng.choice(POOL_QUAL))
    c1, c2 = str(rng.choice(POOL_CIGAR)), str(rng.choice(POOL_CIGAR))
    tlen = p2 + 10 - p1
    return [_rec(name, f1, c, p1, c, p2, tlen, qual=[q1] * 10, cigar=c1, rgid=rg, split=split),
            _rec(name if name2 is None else name2, f2, c, p2, c, p1, -tlen, qual=[q2] * 10, cigar=c2, rgid=rg if rg2 is None else rg2,
                 split=split if split2 is None else split2)]


def _frag(rng, name, on=None):
    """a single-end fragment out of the pool; `on`: a record whose fragment key it takes (the pairs' fbest look-up finds it)"""
    q = int(rng.choice(POOL_QUAL))
    if on is not None:
        return _rec(name, on["flag"] & 0x10, on["refid"], on["pos"], qual=[q] * 10, cigar=on["cigar"], rgid=on["rgid"], split=on["split"])
    pos = int(rng.choice(POOL_FIRST + POOL_MATE + POOL_FRAG_ONLY))
    return _rec(name, 0x10 if rng.integers(0, 2) else 0, int(rng.integers(0, 2)), pos, qual=[q] * 10, cigar=str(rng.choice(POOL_CIGAR)))


def _moved(rng, rec):
    """a second copy of a record at another place of the pool (the toggling cases' t2)"""
    pool = POOL_FIRST if rec["pos"] in POOL_FIRST else POOL_MATE
    pos = int(rng.choice([p for p in pool if p != rec["pos"]]))
    return dict(rec, pos=pos, qual=[int(rng.choice(POOL_QUAL))] * 10)


def _toggling(name, name_a, c):
    """kat_cases.toggling_cases' records on contig c -> (a, t0, t1, t2): pair a (score 800) holds the key of (t0, t1) (score 400)"""
    a = [_rec(name_a, 99, c, 100, c, 300, 210, qual=Q40), _rec(name_a, 147, c, 300, c, 100, -210, qual=Q40)]
    t0, t1 = _rec(name, 99, c, 100, c, 300, 210, qual=Q20), _rec(name, 147, c, 300, c, 100, -210, qual=Q20)
    t2 = _rec(name, 99, c, 700, c, 300, -410, qual=Q20)
    return a, t0, t1, t2


# ---- the motifs: f(rng, r, nm, li) -> the records of repetition r.  nm: the names, li: the index of the name length (it shifts rotations, so
# that what rotates over the repetitions meets every phase over the lengths)
def _plain(rng, r, nm, li):
    """pair, fragment, pair: p = 5 puts the pairs at even and odd parity in alternate repetitions"""
    a, b = _pair(rng, nm.s(nm.new())), _pair(rng, nm.s(nm.new()), rg=int(rng.integers(0, 4) == 0))
    f = _frag(rng, nm.s(nm.new()), on=a[0] if r % 4 == 0 else None)
    return a + [f] + b


def _triple(rng, r, nm, li):
    """t0 t1 t2 of one name in both arrival orders, then two pairs (p = 7); the first two repetitions are the toggling cases themselves"""
    if r < 2:
        a, t0, t1, t2 = _toggling(nm.s(nm.new()), nm.s(nm.new()), 0)
        return [t0, t1, t2] + a + _pair(rng, nm.s(nm.new())) if r == 0 else [t2, t0, t1] + _pair(rng, nm.s(nm.new())) + _pair(rng, nm.s(nm.new()))
    t0, t1 = _pair(rng, nm.s(nm.new()))
    t2 = _moved(rng, t0)
    return ([t0, t1, t2] if r % 2 == 0 else [t2, t0, t1]) + _pair(rng, nm.s(nm.new())) + _pair(rng, nm.s(nm.new()))


def _quad(rng, r, nm, li):
    """t0 t1 t2 t1' of one name, a pair, a fragment (p = 7); the first two repetitions are the toggling cases' four records, on contig 0
    and - in the other arrival order - on contig 1"""
    if r < 2:
        a, t0, t1, t2 = _toggling(nm.s(nm.new()), nm.s(nm.new()), r)
        return ([t0, t1, t2, dict(t1)] if r == 0 else [t2, dict(t1), t0, t1]) + a + [_rec(nm.s(nm.new()), 0, r, 900)]
    t0, t1 = _pair(rng, nm.s(nm.new()))
    # t2 at a place of its own: (t2, t1') is never a duplicate.  Were both pairs flagged, the reference's metrics pass - which pairs the
    # flagged reads up again in SORTED order (markOpticalDuplicatesPair) - would pair t0 with t2 and panic ("origin ... unknown")
    t2, t3 = dict(t0, pos=1000 + 2 * r), dict(t1)
    return ([t0, t1, t2, t3] if r % 2 == 0 else [t2, t3, t0, t1]) + _pair(rng, nm.s(nm.new())) + [_frag(rng, nm.s(nm.new()))]


def _near(rng, r, nm, li, kind, interleaved):
    """Two neighbouring records X0 X1 of one name that do not join, their mates X0' X1' in the same order, a fragment (p = 5).
    block:        X0 X1 X0' X1' F   a run of four whose every neighbour test must fail
    interleaved:  X0 X1 F X0' X1'   two runs of exactly two: a test that joins them makes a neighbour pair of two strangers
    What sets X0 and X1 apart rotates: library, split, X1 no mate candidate (secondary / mate unmapped) for kind "keys"; one byte of the
    name (the last, or the first where the name has a prefix) for kind "names"."""
    k = nm.new()
    x = _pair(rng, nm.s(k))
    if kind == "names":
        twin = nm.s(k + 1) if (r + li) % 3 or nm.L <= 4 else nm.s(k, first="R")
        y = _pair(rng, twin)
    else:
        v = (r + li) % 4
        if v == 0:
            y = _pair(rng, nm.s(k), rg=1)
        elif v == 1:
            y = _pair(rng, nm.s(k), split=1)
        elif v == 2:  # a secondary alignment and another one
            y = _pair(rng, nm.s(k))
            y[0]["flag"] |= 0x100
            y[1]["flag"] |= 0x100
        else:         # a read whose mate is unmapped (a true fragment: a candidate, but of no pair), then that mate
            y = _pair(rng, nm.s(k))
            y[0]["flag"] = 0x1 | 0x8 | 0x40 | (y[0]["flag"] & 0x10)
            y[1] = _rec(nm.s(k), 0x1 | 0x4 | 0x80 | ((y[0]["flag"] & 0x10) << 1), y[0]["refid"], y[0]["pos"], y[0]["refid"], y[0]["pos"],
                        qual=y[1]["qual"])
    f = _frag(rng, nm.s(nm.new()))
    return [x[0], y[0], f, x[1], y[1]] if interleaved else [x[0], y[0], x[1], y[1], f]


def _separated(rng, r, nm, li):
    """X Y X' Y' F: mates at distance 2, every candidate on the table path next to neighbours that are not its mate"""
    x, y = _pair(rng, nm.s(nm.new())), _pair(rng, nm.s(nm.new()))
    return [x[0], y[0], x[1], y[1], _frag(rng, nm.s(nm.new()))]


ANNOUNCE_AHEAD = 100  # repetitions between a pair and the third record of its name: 1100 records


def _announced(rng, r, nm, li):
    """Four ordinary pairs, one more record, a neighbour pair Z Z' (p = 11).  The one more record is a fragment in every third repetition;
    in the others it is a third candidate with the name of the Z pair 100 repetitions further on (212 back, at the stream's end): that
    pair's key is announced in the Bloom filter and the call falls back from the fixed slots, while the other Z pairs stay neighbours."""
    out = []
    for _ in range(4):
        out += _pair(rng, nm.s(nm.new()))
    if r % 3 == 0:
        out.append(_frag(rng, nm.s(nm.new())))
    else:
        z = _pair(rng, _z_name(nm, (r + ANNOUNCE_AHEAD) % REPS))[0]
        out.append(z)
    return out + _pair(rng, _z_name(nm, r))


def _z_name(nm, r):
    return nm.s(2 * r, first="Z") if nm.L > 4 else nm.s(2 * (20000 + r))  # (short names have no prefix: counters no ordinary pair reaches)


MOTIFS = {
    "plain": (5, _plain),
    "triple": (7, _triple),
    "quad": (7, _quad),
    "near_keys": (5, functools.partial(_near, kind="keys", interleaved=False)),
    "near_names": (5, functools.partial(_near, kind="names", interleaved=False)),
    "near_keys_interleaved": (5, functools.partial(_near, kind="keys", interleaved=True)),
    "near_names_interleaved": (5, functools.partial(_near, kind="names", interleaved=True)),
    "separated": (5, _separated),
    "announced": (11, _announced),
}
# slots of a motif by what stands there (the toggling repetitions of triple and quad have the same layout as the others, but for r odd
# the same-name run is in the other order: the slots below hold for both)
SLOTS = {
    "plain": dict(pair=(0, 1, 3, 4), frag=(2,)),
    "triple": dict(run=(0, 1, 2), pair=(3, 4, 5, 6)),
    "quad": dict(run=(0, 1, 2, 3), pair=(4, 5), frag=(6,)),
    "near_keys": dict(run=(0, 1, 2, 3), frag=(4,)),
    "near_names": dict(run=(0, 1, 2, 3), frag=(4,)),
    "near_keys_interleaved": dict(run=(0, 1, 3, 4), frag=(2,)),
    "near_names_interleaved": dict(run=(0, 1, 3, 4), frag=(2,)),
    "separated": dict(run=(0, 1, 2, 3), frag=(4,)),
    "announced": dict(pair=tuple(range(8)) + (9, 10)),
}


def _seed(*what):
    return zlib.crc32(":".join(str(w) for w in what).encode())


def stream(motif: str, L: int, reps: int = REPS):
    """the records of `reps` repetitions of the motif with names of L bytes"""
    p, f = MOTIFS[motif]
    rng = np.random.default_rng(_seed(motif, L))
    nm = _Names(L)
    li = LENGTHS.index(L) if L in LENGTHS else 0
    out = []
    for r in range(reps):
        recs = f(rng, r, nm, li)
        assert len(recs) == p
        out += recs
    return out


class ReadSet:
    """a batch with what the oracle makes of it, computed once and shared (nobody writes to it)"""

    def __init__(self, b: Batch):
        self.b = b
        self._exp = None

    @property
    def expected(self):
        """-> (flags, unclipped positions, scores, permutation as staged, permutation behind mark duplicates, counters).  The oracle is
        run once per split file, as the reference is: flags and counters come split by split, the sort is one over all records."""
        if self._exp is None:
            h, b = header(), self.b
            flags, upos, score = np.zeros(b.n, np.uint16), np.zeros(b.n, np.int32), np.zeros(b.n, np.int32)
            ctr = np.zeros((h.n_lib + 1, orc.NCTR), np.int64)
            for sp in np.unique(b.split):
                idx = np.nonzero(b.split == sp)[0]
                sub = b
                if len(idx) != b.n:
                    sub = b.take(idx)
                    sub.split[:] = 0
                flags[idx], upos[idx], score[idx] = orc.mark_duplicates(sub, h, with_adapted=True)
                ctr += orc.dup_metrics(sub, h, orc.sort_coordinate(sub), 100)[1]
            self._exp = (flags, upos, score, orc.sort_coordinate(b), orc.sort_coordinate(b, flags), ctr)
            for a in self._exp:
                a.setflags(write=False)
        return self._exp


@functools.lru_cache(maxsize=None)
def read_set(motif: str, L: int) -> ReadSet:
    return ReadSet(batch_from_records(stream(motif, L)))


@functools.lru_cache(maxsize=None)
def prefix_set(n: int) -> ReadSet:
    return ReadSet(read_set("plain", PREFIX_L).b.take(np.arange(n)))


@functools.lru_cache(maxsize=None)
def short_set(L: int, s: int) -> ReadSet:
    """Names of one and two bytes: the plain motif over as many repetitions as the alphabet has names for (at most 90), slid through
    the phases by s single-end fragments staged in front.  The pairs' names are all different; a fragment is no mate candidate and
    shares its pair's."""
    names = _SHORT_ALPHABET if L == 1 else [a + b for a in _SHORT_ALPHABET[:14] for b in _SHORT_ALPHABET[:14]]
    reps = min(90, len(names) // 2)
    rng = np.random.default_rng(_seed("short", L))
    out = [_rec(names[k % len(names)], 0x10 * (k & 1), 1, 10 + k) for k in range(s)]
    for r in range(reps):
        a, b = _pair(rng, names[2 * r]), _pair(rng, names[2 * r + 1])
        out += a + [_frag(rng, names[2 * r], on=a[0] if r % 4 == 0 else None)] + b
    return ReadSet(batch_from_records(out))


def phases(n: int) -> np.ndarray:
    return np.arange(n) % WG
