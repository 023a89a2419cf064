"""Optical duplicates' QNAME fields at Go's edges: a restatement of computeTileInfo + strconv.ParseInt(s, 10, 64) and of the
distance rule on Go's wrapping int (filters/mark-optical-duplicates.go:50-71, filters/unpedantic.go:32, filters/utils.go:62), and a
builder of duplicate pile-ups whose QNAMEs the tests choose.  Shared by the CPU and the GPU tests of the optical names."""
import re

import numpy as np

from elprep_amd.batch import Batch, Header

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LIST_CAP = 300000  # countOpticalDuplicatesFromSlice: a strand list over this is not parsed and counts 0 (:328-330)
_INT = re.compile(rb"[+-]?[0-9]+")


def go_parse_int(s: bytes):
    """strconv.ParseInt(s, 10, 64): (value, None) or (None, "syntax" | "range")"""
    if not _INT.fullmatch(s):
        return None, "syntax"
    v = int(s)
    if v < I64_MIN or v > I64_MAX:
        return None, "range"
    return v, None


def go_tile_info(name: bytes):
    """computeTileInfo: (tile, x, y, panics)"""
    cols = name.split(b":")
    if len(cols) == 7:
        fs = cols[4:7]
    elif len(cols) == 5:
        fs = cols[2:5]
    else:
        return -1, -1, -1, False
    vals = [go_parse_int(f) for f in fs]
    if any(err for _, err in vals):
        return -1, -1, -1, True
    return vals[0][0], vals[1][0], vals[2][0], False


def wrap64(v: int) -> int:
    """Go's int arithmetic: the value reduced mod 2^64 into [-2^63, 2^63)"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def go_abs(v: int) -> int:
    """absInt (filters/utils.go:62) on a wrapping int: absInt(MinInt64) == MinInt64"""
    return wrap64(-v) if v < 0 else v


def go_short_close(a, b, dist: int) -> bool:
    """isOpticalDuplicateShort on two (t, x, y) tiles"""
    return go_abs(wrap64(a[1] - b[1])) <= dist and go_abs(wrap64(a[2] - b[2])) <= dist


def go_close(a, b, rg_a, rg_b, dist: int) -> bool:
    """isOpticalDuplicate (:82-93)"""
    return rg_a == rg_b and a[0] != -1 and b[0] != -1 and a[0] == b[0] and go_short_close(a, b, dist)


def go_list_count(tiles, rgs, dist: int):
    """countOpticalDuplicatesFromSlice (:327-368) on a strand list: (optical duplicates, panics)"""
    n = len(tiles)
    if n > LIST_CAP or n < 2:
        return 0, False
    if any(t[3] for t in tiles):
        return 0, True
    if n < 4:
        c = lambda i, j: go_close(tiles[i], tiles[j], rgs[i], rgs[j], dist)
        ctr = int(c(0, 1))
        if n == 2:
            return ctr, False
        ctr += int(c(0, 2))
        if ctr == 2:
            return 2, False
        return ctr + int(c(1, 2)), False
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for i in range(n):
        if tiles[i][0] == -1:
            continue
        for j in range(i + 1, n):
            if tiles[j][0] == tiles[i][0] and rgs[j] == rgs[i] and go_short_close(tiles[i], tiles[j], dist):
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[rj] = ri
    return n - len({find(i) for i in range(n)}), False


class Pile:
    """one duplicate set: the pairs share one pair key; member 0 is the best pair (the origin).  names[k] is the QNAME of pair k,
    fwd[k] whether its listed read (the First of the pair) is on the forward strand, rg[k] its read group."""

    def __init__(self, names, fwd, rg):
        self.names, self.fwd, self.rg = list(names), np.asarray(fwd, bool), np.asarray(rg, np.uint16)
        assert len(self.names) == self.fwd.size == self.rg.size

    def expected(self, dist: int):
        """(optical duplicates, listed reads after the cap, panics) as the reference computes them for this set"""
        opt, listed, panics = 0, 0, False
        for strand in (True, False):
            idx = np.nonzero(self.fwd == strand)[0]
            idx = idx[:LIST_CAP + 1]
            o, p = go_list_count([go_tile_info(self.names[k]) for k in idx], [int(self.rg[k]) for k in idx], dist)
            opt, listed, panics = opt + o, listed + idx.size, panics or p
        return opt, listed, panics


def header(n_rg: int = 2, rg_ids=None) -> Header:
    """one library over all read groups, one contig long enough for a pile-up every 400 positions"""
    return Header(ref_len=np.array([50_000_000], np.int32), rg_lib=np.zeros(n_rg, np.uint16), rg_cov=np.arange(n_rg, dtype=np.uint16),
                  ref_names=["chrO"], rg_ids=list(rg_ids) if rg_ids else ["rg%d" % k for k in range(n_rg)])


def batch(piles, singles=(), L: int = 8) -> Batch:
    """the piles one after the other (pile s at position 1000 + 400 s, mates 200 apart), then `singles`: (name, rg) pairs alone on
    a pair key of their own (records outside any duplicate set).  Mates are adjacent; all names must be distinct."""
    names, first_fwd, rgs, pos = [], [], [], []
    for s, p in enumerate(piles):
        names += p.names
        first_fwd += list(p.fwd)
        rgs += list(p.rg)
        pos += [1000 + 400 * s] * len(p.names)
    for k, (nm, rg) in enumerate(singles):
        names.append(nm)
        first_fwd.append(True)
        rgs.append(rg)
        pos.append(1000 + 400 * (len(piles) + k))
    assert len(set(names)) == len(names), "QNAMEs must be distinct: pairs are matched by name"
    n = len(names)
    first_fwd = np.asarray(first_fwd, bool)
    p0 = np.asarray(pos, np.int32)
    lens = np.fromiter((len(s) for s in names), dtype=np.int64, count=n)
    qname = np.frombuffer(b"".join(s + s for s in names), dtype=np.uint8).copy()
    N = 2 * n
    qoff = np.zeros(N + 1, np.uint64)
    np.cumsum(np.repeat(lens, 2), out=qoff[1:])
    flag = np.empty(N, np.uint16)
    flag[0::2] = np.where(first_fwd, 99, 163)   # forward mate: first (99) or last (163) of the pair
    flag[1::2] = np.where(first_fwd, 147, 83)   # reverse mate
    pos = np.empty(N, np.int32); pos[0::2] = p0; pos[1::2] = p0 + 200
    pnext = np.empty(N, np.int32); pnext[0::2] = p0 + 200; pnext[1::2] = p0
    tlen = np.empty(N, np.int32); tlen[0::2] = 200 + L; tlen[1::2] = -(200 + L)
    qual = np.full((n, 2 * L), 30, np.uint8)
    at = 0
    for p in piles:  # the first pair of every pile is its best pair: the origin
        qual[at] = 40
        at += len(p.names)
    off = np.arange(N + 1, dtype=np.uint64)
    return Batch(refid=np.zeros(N, np.int32), pos=pos, next_refid=np.zeros(N, np.int32), pnext=pnext, tlen=tlen, flag=flag,
                 mapq=np.full(N, 60, np.uint8), rgid=np.asarray(rgs, np.uint16).repeat(2), has_sr=np.zeros(N, np.uint8),
                 l_seq=np.full(N, L, np.uint32), qname_off=qoff, qname=qname, cigar_off=off, cigar=np.full(N, (L << 4) | 0, np.uint32),
                 seq_off=off * np.uint64(L // 2), seq4=np.full(N * L // 2, 0x12, np.uint8), qual_off=off * np.uint64(L), qual=qual.reshape(-1))


def expected_metrics(piles, dist: int, hist_len: int):
    """(optical duplicates, [3][hist_len] histograms of the piles' sets, panics) for one library"""
    opt_all, hist, panics = 0, np.zeros((3, hist_len), np.int64), False
    for p in piles:
        opt, n, pn = p.expected(dist)
        panics = panics or pn
        opt_all += opt
        hist[0, min(n, hist_len - 1)] += 1
        if n - opt > 0:
            hist[1, min(n - opt, hist_len - 1)] += 1
        if opt > 0:
            hist[2, min(opt + 1, hist_len - 1)] += 1
    return opt_all, hist, panics


# ---- field values and names at the edges
EDGE_VALUES = [0, 1, 7, 1101, 99999, 10 ** 17 - 1, 10 ** 17, 10 ** 18 - 1, 10 ** 18, 10 ** 18 + 3, I64_MAX, I64_MAX - 5, I64_MIN, I64_MIN + 5,
               -1, -(10 ** 18), -(10 ** 18) + 1, 4611686018427387904, -4611686018427387904]


def spell(v: int, rng, width_max: int = 26) -> bytes:
    """v written as Go accepts it: sign ('+' optional for v >= 0, '-0' for 0 sometimes), leading zeros up to width_max characters"""
    s = str(abs(v))
    sign = "-" if v < 0 else ("+" if rng.random() < 0.25 else ("-" if v == 0 and rng.random() < 0.3 else ""))
    room = width_max - len(s) - len(sign)
    if room > 0 and rng.random() < 0.4:
        s = "0" * int(rng.integers(1, room + 1)) + s
    return (sign + s).encode()


def tile_name(uid: int, ncol: int, t: bytes, x: bytes, y: bytes, length: int = 0) -> bytes:
    """a QNAME of ncol colon fields with t / x / y in the last three (ncol 5 or 7: the tile fields; other counts: no tile), made
    unique by uid in the first field and padded to `length` bytes (when it is shorter) inside the first field"""
    head = b"u%x" % uid
    if ncol == 7:
        fields = [head, b"1", b"FC", b"1", t, x, y]
    elif ncol == 5:
        fields = [head, b"1", t, x, y]
    else:
        fields = [head] + [b"9"] * max(ncol - 4, 0) + [t, x, y][:ncol - 1]
        fields = fields[:ncol]
    nm = b":".join(fields)
    if len(nm) < length:
        fields[0] = head + b"N" * (length - len(nm))
        nm = b":".join(fields)
    return nm
