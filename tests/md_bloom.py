"""Read sets that are derived from mark duplicates' key hash (qname_hash and its inline copy in k_md_front, csrc/markdup.hip): names are
searched so that their Bloom-filter bit is one that was announced - or is exactly a given one.

In aligner order a neighbour pair goes through the mate table iff the filter holds its key's bit.  The bit is the low 5 + log2(bw) bits of
the high half of the key hash (word (hi >> 5) & (bw - 1), bit hi & 31; a coarse bit per 16 words), and the hash is plain arithmetic over
the name's bytes, the library and the split id: a numpy replica finds names that hit by search.  With 127 far-apart pairs (254 records that
announce their 127 names) the first mate table gets Tm = 4096 slots; 3969 neighbour pairs whose names hit one of the at most 127 bits make
exactly Tm names on the table path (the set `full`: the table ends full, no retry), one more makes Tm + 1 (the sets `over*`: the first pass
cannot place them all, whatever the interleaving, and the host repeats it with all T slots).  The seam sets hold ONE announcement each, at
a chosen bit index - the first and last bit of a word, of a 64-byte line, of a coarse word, of the filter.

Names are sequential counters; nothing in the search is random.  Positions, strands, CIGARs and qualities come from a seeded generator
over a pool wide enough that between a quarter and three quarters of the pairs are duplicates.

Shared by tests/test_md_bloom_cpu.py (the sets are what they claim: the replica, the plan and the oracle) and tests/test_gpu_md_bloom.py
(device against oracle, and the kernels that ran)."""
import functools

import numpy as np

from elprep_amd.batch import batch_from_records
from tests.md_seams import POOL_CIGAR, POOL_QUAL, ReadSet, _SHORT_ALPHABET, _seed, _toggling, header  # noqa: F401
from tests.kat_cases import _rec

U = np.uint64
N_SEP = 127            # far-apart pairs: n_tab = 254, the most for which the first table has 4096 slots
TM = 4096              # table_size_for(min(n, 4 * 254 + 1024)): 2 * 2040 + 16 = 4096
SETS = ("full", "over", "over_split", "over_big", "over_2048")
SEAM_LENGTHS = (3, 8, 9, 32, 33, 41, 254)  # the mask regimes of the stored hash (four words at hand, then the loop) and BAM's longest name
SEAM_BITS = {1024: (0, 31, 32, 511, 512, 16383, 16384, 32767), 2048: (32768, 65535)}
SEAMS = tuple((bw, t) for bw in SEAM_BITS for t in SEAM_BITS[bw])
SEAM_FILLERS = 20      # neighbour pairs between t2 and (t0, t1) in the small seam sets
BIG_N = 16400          # the least n with 2048 filter words


# ---- the replica of the key hash
def _mix64(x):
    x = x ^ (x >> U(30))
    x = x * U(0xbf58476d1ce4e5b9)
    x = x ^ (x >> U(27))
    x = x * U(0x94d049bb133111eb)
    return x ^ (x >> U(31))


def hash_many(names: np.ndarray, lib, split) -> np.ndarray:
    """key hashes of the names in the rows of a uint8 matrix (all of one length); lib and split: scalars or one per row"""
    n, L = names.shape
    assert 1 <= L <= 254
    W = (L + 7) // 8
    padded = np.zeros((n, 8 * W), np.uint8)  # (the last word masked to the name's bytes)
    padded[:, :L] = names
    w = padded.view("<u8")
    h = np.full(n, 0x9e3779b97f4a7c15 ^ L, U)
    for k in range(W):
        h = (h ^ w[:, k]) * U(0xff51afd7ed558ccd) + (h >> U(29))
    return _mix64(h ^ (np.asarray(lib, U) << U(48)) ^ (np.asarray(split, U) << U(24)))


def bits_many(names, lib, split, bw) -> np.ndarray:
    """the filter's bit index: 32 x word + bit = the low 5 + log2(bw) bits of the hash's high half"""
    return ((hash_many(names, lib, split) >> U(32)) & U(32 * bw - 1)).astype(np.int64)


def _row(name):
    name = name.encode() if isinstance(name, str) else name
    return np.frombuffer(name, np.uint8)[None, :]


def key_hash(name, lib, split) -> int:
    return int(hash_many(_row(name), lib, split)[0])


def filter_bit(name, lib, split, bw) -> int:
    return int(bits_many(_row(name), lib, split, bw)[0])


# ---- what k_md_front makes of a batch, from its columns alone (the CPU tests count with it; nothing of the builders' bookkeeping)
def record_bits(b, bw) -> np.ndarray:
    """every record's filter bit index (library of read group r = header().rg_lib[r])"""
    rg_lib = header().rg_lib
    off = b.qname_off.astype(np.int64)
    lens = off[1:] - off[:-1]
    out = np.zeros(b.n, np.int64)
    for L in np.unique(lens):
        idx = np.nonzero(lens == L)[0]
        names = b.qname[off[idx][:, None] + np.arange(L)[None, :]]
        out[idx] = bits_many(names, rg_lib[b.rgid[idx]], b.split[idx], bw)
    return out


def mate_keys(b):
    """{split, library, QNAME} of every record"""
    rg_lib = header().rg_lib
    return [(int(b.split[i]), int(rg_lib[b.rgid[i]]), b.qname_of(i)) for i in range(b.n)]


def classify(b) -> np.ndarray:
    """0 no mate candidate, 1 table path, 2 leader / 3 follower of a run of exactly two neighbours with one key"""
    f = b.flag.astype(np.int64)
    cand = ((f & (0x4 | 0x100 | 0x800)) == 0) & ((f & (0x1 | 0x8)) == 0x1)
    keys = mate_keys(b)
    join = np.zeros(b.n + 3, bool)  # join[i + 2]: records i and i + 1 are candidates with one key
    for i in range(b.n - 1):
        join[i + 2] = cand[i] and cand[i + 1] and keys[i] == keys[i + 1]
    code = np.zeros(b.n, np.int64)
    for i in range(b.n):
        if cand[i]:
            nx, pv = join[i + 2], join[i + 1]
            code[i] = 2 if nx and not pv and not join[i + 3] else 3 if pv and not nx and not join[i] else 1
    return code


def table_keys(b, bw):
    """-> (keys on the table path: the announced ones and those of the neighbour pairs whose bit was announced, number of table-path
    records of the front pass, the announced bits)"""
    code, bits, keys = classify(b), record_bits(b, bw), mate_keys(b)
    announced = set(bits[code == 1].tolist())
    on_table = {keys[i] for i in range(b.n) if code[i] == 1 or (code[i] == 2 and int(bits[i]) in announced)}
    return on_table, int((code == 1).sum()), announced


# ---- names
def _decimal(prefix: bytes, k0: int, count: int, width: int) -> np.ndarray:
    """prefix + the counters k0 .. k0 + count - 1 in `width` decimal digits, one name per row"""
    k = np.arange(k0, k0 + count, dtype=np.int64)
    out = np.empty((count, len(prefix) + width), np.uint8)
    out[:, :len(prefix)] = np.frombuffer(prefix, np.uint8)
    for d in range(width):
        out[:, len(prefix) + width - 1 - d] = 48 + (k // 10 ** d) % 10
    return out


_ALPHA = np.frombuffer("".join(_SHORT_ALPHABET).encode(), np.uint8)


def _counted(L: int, k0: int, count: int) -> np.ndarray:
    """names of L bytes: 'T', padding, and the counter in the last (at most four) bytes over QNAME's alphabet - for L >= 36 two names
    agree in their first 32 bytes, and names of three bytes are all counter"""
    w, base = min(L, 4), len(_ALPHA)
    k = np.arange(k0, k0 + count, dtype=np.int64)
    out = np.full((count, L), ord("n"), np.uint8)
    if L > w:
        out[:, 0] = ord("T")
    for d in range(w):
        out[:, L - 1 - d] = _ALPHA[(k // base ** d) % base]
    return out


CHUNK = 1 << 17


@functools.lru_cache(maxsize=None)
def _search(prefix: bytes, width: int, lib: int, split: int, bits: tuple, bw: int, want: int, hit: bool):
    """the first `want` names prefix + counter whose bit is (hit) / is not (not hit) one of `bits` -> tuple of names, in counter order"""
    out, k0, bits = [], 0, np.asarray(bits, np.int64)
    while len(out) < want:
        assert k0 + CHUNK <= 10 ** width
        names = _decimal(prefix, k0, CHUNK, width)
        ok = np.isin(bits_many(names, lib, split, bw), bits) == hit
        out += [names[i].tobytes() for i in np.nonzero(ok)[0][:want - len(out)]]
        k0 += CHUNK
    return tuple(out)


@functools.lru_cache(maxsize=None)
def seam_name(bw: int, target: int) -> bytes:
    """the first counted name (library 0, split 0) whose filter bit index is exactly `target`; its length rotates with the case"""
    L = SEAM_LENGTHS[SEAMS.index((bw, target)) % len(SEAM_LENGTHS)]
    total = len(_ALPHA) ** min(L, 4)
    for k0 in range(0, total, CHUNK):
        names = _counted(L, k0, min(CHUNK, total - k0))
        at = np.nonzero(bits_many(names, 0, 0, bw) == target)[0]
        if len(at):
            return names[at[0]].tobytes()
    raise AssertionError((bw, target, L))


# ---- records
def _wide_pair(rng, name, rg=0, split=0, w=11):
    """a true pair -> [first end, second end]; w places per end, two contigs, two orientations"""
    c = int(rng.integers(0, 2))
    p1, p2 = 400 + 10 * int(rng.integers(0, w)), 1000 + 10 * int(rng.integers(0, w))
    rev1 = bool(rng.integers(0, 2))
    f1 = 0x1 | 0x2 | 0x40 | (0x10 if rev1 else 0x20)
    f2 = 0x1 | 0x2 | 0x80 | (0x20 if rev1 else 0x10)
    q1, q2 = int(rng.choice(POOL_QUAL)), int(rng.choice(POOL_QUAL))
    c1, c2 = str(rng.choice(POOL_CIGAR)), str(rng.choice(POOL_CIGAR))
    tlen = p2 + 10 - p1
    return [_rec(name, f1, c, p1, c, p2, tlen, qual=[q1] * 10, cigar=c1, rgid=rg, split=split),
            _rec(name, f2, c, p2, c, p1, -tlen, qual=[q2] * 10, cigar=c2, rgid=rg, split=split)]


def _third(rng, rec):
    """one more record with a pair's name: its first end at a place of its own"""
    return dict(rec, pos=700 + 10 * int(rng.integers(0, 8)), qual=[int(rng.choice(POOL_QUAL))] * 10)


class BloomSet(ReadSet):
    """a read set with what its builder meant: bw, the number of names meant for the table, where the neighbour pairs start"""

    def __init__(self, records, bw, n_names, pair_starts, n_tab):
        super().__init__(batch_from_records(records))
        self.bw, self.n_names, self.n_tab = bw, n_names, n_tab
        self.pair_starts = np.asarray(pair_starts, np.int64)
        self.pair_starts.setflags(write=False)


def _bulk(what, n_names, bw=1024, splits=1, thirds=False, w=11, front_hits=0, fill_to=0):
    """[first ends of the far-apart pairs] [hit pairs] [their second ends]: n_names names for the table.
    splits = 2: the records alternate between two splits, every name searched under its own.
    thirds: four records more (and two far-apart pairs fewer, so that n_tab stays 254) with the name of a hit pair, in front of it and
    behind it, and with that of a far-apart pair, between its ends and behind them.
    front_hits, fill_to: only front_hits hit pairs stand behind the first ends; pairs that do not hit fill up to record fill_to, and the
    other hit pairs follow from there."""
    rng = np.random.default_rng(_seed("bloom", what))
    n_sep = N_SEP - 2 if thirds else N_SEP
    sep_names = [_decimal(b"S", k, 1, 7)[0].tobytes() for k in range(n_sep)]
    sep = [_wide_pair(rng, nm, rg=0, split=k % splits, w=w) for k, nm in enumerate(sep_names)]
    bits = tuple(sorted({filter_bit(nm, 0, k % splits, bw) for k, nm in enumerate(sep_names)}))
    # the hit names: about half under library 1 (names of 11 bytes: two words, the second masked), each searched under its own split
    n_hit = n_names - n_sep
    combos = [(lib, sp) for sp in range(splits) for lib in (0, 1)]
    share = [n_hit // len(combos) + (1 if c < n_hit % len(combos) else 0) for c in range(len(combos))]
    found = [_search(b"h" if lib == 0 else b"g", 7 if lib == 0 else 10, lib, sp, bits, bw, share[c], True) for c, (lib, sp) in enumerate(combos)]
    hits = []
    for k in range(max(share)):
        for c, (lib, sp) in enumerate(combos):
            if k < share[c]:
                hits.append(_wide_pair(rng, found[c][k], rg=lib, split=sp, w=w))
    assert len(hits) == n_hit
    front = [p[0] for p in sep]
    back = [p[1] for p in sep]
    if thirds:
        front.insert(3, _third(rng, hits[40][0]))             # t2 t0 t1: (t2, t0) pair up
        mid = _third(rng, sep[5][0])                          # x0 x2 x1: (x0, x2)
        back += [_third(rng, hits[41][0]), _third(rng, sep[6][0])]  # t0 t1 t2: (t0, t1); x0 x1 x2: (x0, x1)
    out = list(front)
    pair_starts = []

    def put(pairs):
        for p in pairs:
            pair_starts.append(len(out))
            out.extend(p)

    if fill_to:
        put(hits[:front_hits])
        n_fill = (fill_to - len(out)) // 2
        fill = _search(b"f", 7, 0, 0, bits, bw, n_fill, False)
        put(_wide_pair(rng, nm, w=w) for nm in fill)
        put(hits[front_hits:])
    elif thirds:
        put(hits[:2000])
        out.append(mid)
        put(hits[2000:])
    else:
        put(hits)
    out += back
    return BloomSet(out, bw, n_names, pair_starts, 2 * n_sep + (4 if thirds else 0))


BULK = {
    "full": dict(n_names=TM),
    "over": dict(n_names=TM + 1),
    "over_split": dict(n_names=TM + 1, splits=2, w=8),
    "over_big": dict(n_names=TM + 1, thirds=True),
    # 127 first ends and 65 hit pairs: records 0 .. 256; pairs that do not hit up to record 16383; the other hit pairs and the second ends
    # stand in workgroups 63 and up of k_mate_pairs: workgroup 64 appends 256 records to list 0 behind workgroup 0's 256
    "over_2048": dict(n_names=TM + 1, bw=2048, w=18, front_hits=65, fill_to=16383),
}


@functools.lru_cache(maxsize=None)
def read_set(name: str) -> BloomSet:
    return _bulk(name, **BULK[name])


def _seam_records(bw, target, renamed):
    """t2, pair a, pairs that do not hit, then the neighbours t0 t1 with t2's name.  renamed: t2 under a name of its own (what a filter
    false negative makes of the set: (t0, t1) pair up and lose against a)"""
    rng = np.random.default_rng(_seed("seam", bw, target))
    name = seam_name(bw, target)
    n_fill = SEAM_FILLERS if bw == 1024 else (BIG_N - 5 + 1) // 2
    others = _search(b"f", 7, 0, 0, (target,), bw, n_fill + 2, False)
    a, t0, t1, t2 = _toggling(name, others[0], 0)
    if renamed:
        t2 = dict(t2, qname=others[1])
    out = [t2] + a
    for nm in others[2:]:
        out += _wide_pair(rng, nm)
    return out + [t0, t1]


@functools.lru_cache(maxsize=None)
def seam_set(bw: int, target: int, renamed: bool = False) -> BloomSet:
    recs = _seam_records(bw, target, renamed)
    return BloomSet(recs, bw, 1, range(1, len(recs), 2), 1)
