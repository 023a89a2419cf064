"""A DEFLATE encoder for tests (RFC 1951, written from the RFC) and a catalogue of the forms a conforming stream may take that zlib's
deflate never writes: other writers' framing (a separate final stored block of LEN 0, one unused distance code, members of 65536 bytes),
non-optimal and deep codes, every header spelling, the matches that strain the resolve phase - and the invalid streams beside them.
zlib's INFLATE is the reference for every form (tests/test_deflate_forms_cpu.py); the device's decoder meets them in
tests/test_gpu_inflate_forms.py.  Plain Python, no GPU; everything is deterministic from the seeds."""
import heapq
import struct
import zlib
from fractions import Fraction

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
MAX_MEMBER = 65536                 # BSIZE is 16 bits: a member is at most this long
MEMBER_OVERHEAD = 26               # 18 bytes of header, CRC-32 and ISIZE
MAX_CDATA = MAX_MEMBER - MEMBER_OVERHEAD
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# length 3..258 -> (length symbol - 257, extra value); 258 is symbol 28 (285)
_LSYM = [None] * 259
for _s in range(28):
    for _x in range(1 << LEN_EXTRA[_s]):
        if LEN_BASE[_s] + _x <= 257:
            _LSYM[LEN_BASE[_s] + _x] = (_s, _x)
_LSYM[258] = (28, 0)
_DSYM = [None] * 32769
for _s in range(30):
    for _x in range(1 << DIST_EXTRA[_s]):
        _DSYM[DIST_BASE[_s] + _x] = (_s, _x)


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lengths):
    """the canonical codes of a list of code lengths (RFC 1951 3.2.2), each as (code with its first bit lowest, length); None for 0"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lengths:
        if n:
            out.append((_rev(nxt[n], n), n))
            nxt[n] += 1
        else:
            out.append(None)
    return out


def kraft(lengths):
    return sum((Fraction(1, 1 << n) for n in lengths if n), Fraction(0))


def huff_lengths(freq, limit):
    """code lengths of at most `limit` bits for the symbols of `freq` (symbol -> count > 0): Huffman's, then the longest shortened to the
    limit and the Kraft sum brought back to 1.  One symbol gets length 1 (the caller completes the code)."""
    syms = sorted(freq)
    if len(syms) == 1:
        return {syms[0]: 1}
    heap = [(freq[s], k, (s,)) for k, s in enumerate(syms)]
    heapq.heapify(heap)
    depth = dict.fromkeys(syms, 0)
    k = len(syms)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], k, a[2] + b[2]))
        k += 1
    if max(depth.values()) > limit:
        for s in syms:
            depth[s] = min(depth[s], limit)
        unit = 1 << limit
        total = sum(unit >> depth[s] for s in syms)
        by_freq = sorted(syms, key=lambda s: (freq[s], s))
        while total > unit:  # lengthen the rarest symbol that is not at the limit yet
            s = max((t for t in by_freq if depth[t] < limit), key=lambda t: (depth[t], -freq[t]))
            total -= unit >> (depth[s] + 1)
            depth[s] += 1
        for s in reversed(by_freq):  # and give what is left over to the most frequent ones
            while depth[s] > 1 and total + (unit >> depth[s]) <= unit:
                total += unit >> depth[s]
                depth[s] -= 1
    return depth


def random_complete_code(symbols, freq, rng, max_depth=15, deep=0.6):
    """a random complete code over `symbols` (two at least): one leaf is split into two until there is a leaf per symbol - the Kraft sum is
    exactly 1 throughout -, preferring (probability `deep`) a deepest leaf that may still be split; the LONG codes go to the frequent
    symbols, what no writer that counts would do.  Returns symbol -> length."""
    symbols = list(symbols)
    assert len(symbols) >= 2 and len(symbols) <= 1 << max_depth
    leaves = [0]
    while len(leaves) < len(symbols):
        can = [k for k, d in enumerate(leaves) if d < max_depth]
        if rng.random() < deep:
            top = max(leaves[k] for k in can)
            can = [k for k in can if leaves[k] == top]
        k = can[int(rng.integers(0, len(can)))]
        leaves[k] += 1
        leaves.append(leaves[k])
    leaves.sort(reverse=True)
    order = sorted(symbols, key=lambda s: (-freq.get(s, 0), s))
    out = dict(zip(order, leaves))
    assert kraft(out.values()) == 1 and max(leaves) <= max_depth
    return out


def chain_lengths(symbols):
    """1, 2, ..., k-1, k-1 over k <= 16 symbols in the order given: the deepest complete code there is over them"""
    k = len(symbols)
    assert 2 <= k <= 16
    return dict(zip(symbols, list(range(1, k)) + [k - 1]))


def greedy_spell(lengths):
    """the code-length list with the run codes 16 / 17 / 18 wherever they fit, as [(code-length symbol, extra value)]"""
    items, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                items.append((18, r - 11))
                run -= r
            if run >= 3:
                items.append((17, run - 3))
                run = 0
        else:
            items.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                items.append((16, r - 3))
                run -= r
        items += [(v, 0)] * run
        i = j
    return items


def expand_spelling(items):
    out = []
    for s, x in items:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


def lz_parse(data, max_dist=32768, max_len=258, literals_only=False, forced=None):
    """a greedy LZ77 parse: tokens, a literal as its byte value, a match as (length, distance).  The last place of every 3-byte prefix is
    kept in a dict.  forced: this token list instead (it must spell `data`)."""
    if forced is not None:
        assert apply_tokens(forced) == bytes(data)
        return list(forced)
    if literals_only:
        return list(data)
    data = bytes(data)
    n, toks, seen, i = len(data), [], {}, 0
    while i < n:
        best = 0
        if i + 3 <= n:
            key = data[i:i + 3]
            c = seen.get(key)
            if c is not None and i - c <= max_dist:
                mx, best = min(max_len, n - i), 3
                while best < mx and data[c + best] == data[i + best]:
                    best += 1
                dist = i - c
            seen[key] = i
        if best >= 3:
            toks.append((best, dist))
            for j in range(i + 1, min(i + best, n - 2)):
                seen[data[j:j + 3]] = j
            i += best
        else:
            toks.append(data[i])
            i += 1
    return toks


def apply_tokens(toks, history=b""):
    out = bytearray(history)
    for t in toks:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t[0], t[1]
            assert 1 <= d <= len(out), (d, len(out))
            for _ in range(n):
                out.append(out[-d])
    return bytes(out[len(history):])


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class Deflater:
    """an LSB-first bit writer with the three block writers on it.  It keeps what it emitted: `out` (the intended bytes), `blocks` (type,
    first header bit, first bit behind it, and for a stored block the byte behind its data), the token counts, the code lengths and the
    (length symbol, length) / distance values in use."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0
        self.out = bytearray()
        self.blocks = []
        self.ntok = self.nmatch = 0
        self.ll_used, self.d_used = set(), set()   # code lengths of emitted symbols
        self.lens, self.dists = set(), set()       # (length symbol, length), distance
        self.pairs = set()                         # (length, distance)
        self.placed = set()                        # (position in the output, length, distance)
        self.headers = []                          # of the dynamic blocks: dict(hlit, hdist, hclen, items, cl)

    # ---- bits
    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.nacc

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.nacc
        self.nacc += n
        if self.nacc >= 64:
            k = self.nacc >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.nacc -= 8 * k

    def align(self):
        if self.nacc & 7:
            self.bits(0, 8 - (self.nacc & 7))
        k = self.nacc >> 3
        self.buf += self.acc.to_bytes(k, "little") if k else b""
        self.acc = self.nacc = 0

    def raw(self, data):
        assert self.nacc % 8 == 0
        self.align()
        self.buf += data

    def getvalue(self):
        """the bytes so far (the last one padded with zero bits)"""
        k = (self.nacc + 7) >> 3
        return bytes(self.buf) + (self.acc.to_bytes(k, "little") if k else b"")

    # ---- blocks
    def stored(self, data, final=False, nlen=None):
        start = self.bitpos
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.align()
        self.bits(len(data), 16)
        self.bits((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
        self.raw(data)
        self.out += data
        self.blocks.append(dict(type=0, start=start, end=self.bitpos, data_end=len(self.buf), len=len(data), final=final))

    def _symbols(self, toks, ll, dl, eob=True):
        llc, dlc = canonical(ll), canonical(dl)
        out, bits = self.out, self.bits
        for t in toks:
            self.ntok += 1
            if isinstance(t, int):
                c, n = llc[t]
                bits(c, n)
                self.ll_used.add(n)
                out.append(t)
                continue
            length, dist = t[0], t[1]
            ls, lx = (t[2], length - LEN_BASE[t[2]]) if len(t) > 2 else _LSYM[length]
            assert 0 <= lx < 1 << LEN_EXTRA[ls]
            ds, dx = _DSYM[dist]
            c, n = llc[257 + ls]
            bits(c, n)
            self.ll_used.add(n)
            bits(lx, LEN_EXTRA[ls])
            c, n = dlc[ds]
            bits(c, n)
            self.d_used.add(n)
            bits(dx, DIST_EXTRA[ds])
            self.nmatch += 1
            self.lens.add((257 + ls, length))
            self.dists.add(dist)
            self.pairs.add((length, dist))
            self.placed.add((len(out), length, dist))
            assert dist <= len(out), "distance reaches in front of the member"
            for _ in range(length):
                out.append(out[-dist])
        if eob:
            c, n = llc[256]
            bits(c, n)
            self.ll_used.add(n)

    def fixed(self, toks, final=False):
        start = self.bitpos
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        self._symbols(toks, FIXED_LL, FIXED_D)
        self.blocks.append(dict(type=1, start=start, end=self.bitpos, final=final))

    def auto_lengths(self, toks):
        """Huffman lengths (limit 15) for the symbols of `toks` and the end-of-block code; a code of one symbol is completed with a
        second one of length 1, and where there is no match the distance code is two codes of length 1"""
        fl, fd = {256: 1}, {}
        for t in toks:
            if isinstance(t, int):
                fl[t] = fl.get(t, 0) + 1
            else:
                s = 257 + (t[2] if len(t) > 2 else _LSYM[t[0]][0])
                fl[s] = fl.get(s, 0) + 1
                d = _DSYM[t[1]][0]
                fd[d] = fd.get(d, 0) + 1
        hl = huff_lengths(fl, 15)
        if len(hl) == 1:
            hl[0] = 1
        hd = huff_lengths(fd, 15) if fd else {0: 1, 1: 1}
        if len(hd) == 1:
            hd[1 if 0 in hd else 0] = 1
        ll, dl = [0] * 286, [0] * 30
        for s, n in hl.items():
            ll[s] = n
        for s, n in hd.items():
            dl[s] = n
        return ll, dl

    def header(self, ll, dl, final=False, hlit=None, hdist=None, hclen=None, spelling="greedy", cl=None, check=True):
        """the header of a dynamic block.  ll / dl: code lengths by symbol (shorter lists are padded with 0).  hlit / hdist / hclen: the
        fields as written (default: the smallest that holds the lengths).  spelling: "greedy", "none" or the list of (code-length symbol,
        extra value) to write.  cl: the 19 lengths of the code-length code (default: Huffman's, at most 7 bits).  check=False writes
        whatever it is given (the invalid forms)."""
        ll, dl = list(ll), list(dl)
        if hlit is None:
            hlit = max(max([k + 1 for k, n in enumerate(ll) if n] or [0]), 257) - 257
        if hdist is None:
            hdist = max(max([k + 1 for k, n in enumerate(dl) if n] or [0]), 1) - 1
        nlen, ndist = hlit + 257, hdist + 1
        ll = (ll + [0] * nlen)[:nlen] if check or len(ll) >= nlen else ll
        dl = (dl + [0] * ndist)[:ndist] if check or len(dl) >= ndist else dl
        lengths = ll + dl
        items = greedy_spell(lengths) if spelling == "greedy" else ([(n, 0) for n in lengths] if spelling == "none" else list(spelling))
        if check:
            assert expand_spelling(items) == lengths, "the spelling does not give the code lengths"
            assert kraft(ll) == 1 or sum(1 for n in ll if n) == 1 and max(ll) == 1
            assert kraft(dl) == 1 or sum(1 for n in dl if n) <= 1 and max(dl) <= 1
        if cl is None:
            f = {}
            for s, _ in items:
                f[s] = f.get(s, 0) + 1
            h = huff_lengths(f, 7)
            if len(h) == 1:
                h[0 if 0 not in h else 1] = 1
            cl = [h.get(s, 0) for s in range(19)]
        need = max([k + 1 for k, s in enumerate(CL_ORDER) if cl[s]] + [4])
        if hclen is None:
            hclen = need - 4
        if check:
            assert hclen + 4 >= need and kraft(cl) == 1 and all(cl[s] for s, _ in items)
        start = self.bitpos
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(hlit, 5)
        self.bits(hdist, 5)
        self.bits(hclen, 4)
        for k in range(hclen + 4):
            self.bits(cl[CL_ORDER[k]], 3)
        clc = canonical(cl)
        for s, x in items:
            if clc[s] is not None:
                self.bits(*clc[s])
            if s >= 16:
                self.bits(x, {16: 2, 17: 3, 18: 7}[s])
        self.headers.append(dict(hlit=hlit, hdist=hdist, hclen=hclen, items=items, cl=cl, start=start))
        return start

    def dynamic(self, toks, final=False, ll=None, dl=None, **hdr):
        if ll is None or dl is None:
            a, b = self.auto_lengths(toks)
            ll, dl = a if ll is None else ll, b if dl is None else dl
        ll, dl = (list(ll) + [0] * 286)[:286], (list(dl) + [0] * 30)[:30]
        start = self.header(ll, dl, final, **hdr)
        self._symbols(toks, ll, dl)
        self.blocks.append(dict(type=2, start=start, end=self.bitpos, final=final))


def frame(cdata, data=None, crc=None, isize=None):
    """a BGZF member around `cdata`: CRC-32 and ISIZE are those of `data`, the intended bytes (or as given: the invalid forms)"""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    assert len(cdata) <= MAX_CDATA and isize <= 65536, (len(cdata), isize)
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata + struct.pack("<II", crc, isize)


def plain_member(data):
    """a member as any writer would make it: one final dynamic block (stored where that is smaller)"""
    d = Deflater()
    d.dynamic(lz_parse(data), final=True)
    c = d.getvalue()
    if len(c) > len(data) + 5 and len(data) <= 65535:
        d = Deflater()
        d.stored(data, final=True)
        c = d.getvalue()
    return frame(c, data)


# =====================================================================================================================================
# The catalogue.  A valid form: name, group, `own` (it generates its content) or not (it encodes the caller's bytes), `size` (the member
# size it is about; None: any), encode(data) -> Enc.  An invalid form: (name, cdata, claimed isize).
# =====================================================================================================================================
class Enc:
    def __init__(self, d, **info):
        self.cdata = d.getvalue()
        self.data = bytes(d.out)
        self.d = d
        self.info = info

    @property
    def member(self):
        return frame(self.cdata, self.data)


class Form:
    def __init__(self, name, group, fn, own=False, size=None, **props):
        self.name, self.group, self.fn, self.own, self.size, self.props = name, group, fn, own, size, props

    def encode(self, data=None):
        return self.fn() if self.own else self.fn(bytes(data))

    def __repr__(self):
        return self.name


def _cut_tokens(toks, per_block):
    return [toks[k:k + per_block] for k in range(0, len(toks), per_block)] or [[]]


def _text(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def _noise(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- padding in front of a member that shifts everything behind it by any number of bits mod 8: empty fixed blocks are 10 bits, and
# an empty dynamic block (end-of-block and one more code of length 1, HCLEN 14) is an odd number
def _empty_dynamic(d, hclen=None, single=False):
    ll = [0] * 257
    ll[256] = 1
    if not single:
        ll[0] = 1
    d.dynamic([], ll=ll, dl=[0] if single else [1, 1], hclen=hclen)


def _shift_recipes():
    out = {}
    for hclen in (None, 14, 15):
        for fixed in range(4):
            for dyn in range(2):
                d = Deflater()
                for _ in range(fixed):
                    d.fixed([])
                if dyn:
                    _empty_dynamic(d, hclen)
                out.setdefault(d.bitpos % 8, (fixed, dyn, hclen))
    assert sorted(out) == list(range(8))
    return out


_SHIFT = _shift_recipes()


def _shift(d, by):
    fixed, dyn, hclen = _SHIFT[by % 8]
    for _ in range(fixed):
        d.fixed([])
    if dyn:
        _empty_dynamic(d, hclen)


def _go_close(kind, phase, per_block):
    """what Go's compress/flate leaves behind Close: non-final blocks cut by token count, then BFINAL=1 stored LEN=0.  `phase`: the bit
    in its byte at which the last end-of-block code ends (what decides the padding in front of LEN)"""
    def body(d, data, parts):
        if kind == "stored":
            for k in range(0, max(len(data), 1), 20000):
                d.stored(data[k:k + 20000])
            return
        for part in parts:
            (d.fixed if kind == "fixed" else d.dynamic)(part)

    def fn(data):
        parts = _cut_tokens(lz_parse(data), per_block) if kind != "stored" else None
        d = Deflater()
        body(d, data, parts)
        if kind != "stored":  # (a second time behind the blocks that shift its end to the phase asked for)
            end = d.bitpos % 8
            d = Deflater()
            _shift(d, phase - end)
            body(d, data, parts)
            assert d.bitpos % 8 == phase
        eob_end = d.bitpos
        d.stored(b"", final=True)
        return Enc(d, eob_end=eob_end, phase=eob_end % 8)
    return fn


def _go_literals_only(dist_len):
    def fn(data):
        d = Deflater()
        toks = lz_parse(data, literals_only=True)
        ll, _ = d.auto_lengths(toks)
        d.dynamic(toks, ll=ll, dl=[dist_len], hdist=0)
        d.stored(b"", final=True)
        return Enc(d)
    return fn


def _flush_blocks(data):
    # (one parse of the member, cut into four parts: a later part's matches reach back into the earlier ones)
    q = len(data) // 4
    at, cuts, parts, cur = 0, [q, 2 * q, 3 * q, len(data)], [], []
    d = Deflater()
    for t in lz_parse(data):
        cur.append(t)
        at += 1 if isinstance(t, int) else t[0]
        if at >= cuts[len(parts)] and len(parts) < 3:
            parts.append(cur)
            cur = []
    parts.append(cur)
    d.dynamic(parts[0])
    d.stored(b"")                # an empty stored block in mid-member (Z_FULL_FLUSH)
    d.fixed(parts[1])
    d.fixed([])                  # an empty fixed block (Z_PARTIAL_FLUSH)
    d.dynamic(parts[2])
    for _ in range(200):
        d.fixed([])
    _empty_dynamic(d)            # end-of-block only
    _empty_dynamic(d, single=True)
    d.stored(b"")
    d.stored(b"")
    d.dynamic(parts[3], final=True)
    return Enc(d)


def _many_blocks(data):
    d = Deflater()
    parts = _cut_tokens(lz_parse(data), 4)
    for k, part in enumerate(parts):
        d.dynamic(part, final=k == len(parts) - 1)
    return Enc(d, n_dynamic=len(parts))


def _stored_then_dynamic(end_at):
    """a stored block whose data ends at byte `end_at` of CDATA (its header is 5 bytes), then a dynamic block"""
    def fn(data):
        d = Deflater()
        d.stored(data[:end_at - 5])
        assert len(d.buf) == end_at
        d.dynamic(lz_parse(data[end_at - 5:]), final=True)
        return Enc(d, stored_end=end_at)
    return fn


def _stored_after_compressed(phase):
    def fn(data):
        h = len(data) // 2
        d = Deflater()
        toks = lz_parse(data[:h])
        d.dynamic(toks)
        end = d.bitpos % 8
        d = Deflater()
        _shift(d, phase - end)
        d.dynamic(toks)
        assert d.bitpos % 8 == phase
        eob_end = d.bitpos
        d.stored(data[h:], final=True)
        return Enc(d, phase=eob_end % 8)
    return fn


def _two_stored(data):
    d = Deflater()
    h = len(data) // 3
    d.stored(data[:h])
    d.stored(data[h:2 * h])
    d.dynamic(lz_parse(data[2 * h:]), final=True)
    return Enc(d)


def _largest_stored(data):
    d = Deflater()
    d.stored(data, final=True)
    return Enc(d)


def _isize_parsed(literals_only):
    def fn(data):
        d = Deflater()
        d.dynamic(lz_parse(data, literals_only=literals_only), final=True)
        return Enc(d)
    return fn


def _deep_codes(seed):
    def fn(data):
        rng = np.random.default_rng(seed)
        toks = lz_parse(data)
        d = Deflater()
        for part in _cut_tokens(toks, 3000):
            fl, fd = {256: 1}, {}
            for t in part:
                if isinstance(t, int):
                    fl[t] = fl.get(t, 0) + 1
                else:
                    fl[257 + _LSYM[t[0]][0]] = fl.get(257 + _LSYM[t[0]][0], 0) + 1
                    fd[_DSYM[t[1]][0]] = fd.get(_DSYM[t[1]][0], 0) + 1
            # (the code covers more symbols than the block uses - a writer with a fixed alphabet -, at least 40 / 12 of them)
            ls = sorted(set(fl) | set(int(s) for s in rng.choice(286, 40, replace=False)))
            ds = sorted(set(fd) | set(int(s) for s in rng.choice(30, 12, replace=False)))
            hl, hd = random_complete_code(ls, fl, rng), random_complete_code(ds, fd, rng)
            ll, dl = [0] * 286, [0] * 30
            for s, n in hl.items():
                ll[s] = n
            for s, n in hd.items():
                dl[s] = n
            d.dynamic(part, ll=ll, dl=dl)
        d.stored(b"", final=True)
        return Enc(d)
    return fn


# ---- forms with content of their own
def _one_dist_code(sym):
    def fn():
        rng = np.random.default_rng(40 + sym)
        d = Deflater()
        dl = [0] * 30
        dl[sym] = 1
        if sym == 0:
            toks = []
            for k in range(300):
                toks += [int(rng.integers(0, 256)), (int(rng.integers(3, 259)), 1)]
        else:
            toks = list(_text(rng, 33000))
            for k in range(320):
                toks.append((int(rng.integers(3, 150)), int(rng.integers(24577, 32769))))
                toks.append(int(rng.integers(65, 91)))
        ll, _ = d.auto_lengths(toks)
        d.dynamic(toks, final=True, ll=ll, dl=dl, hdist=sym)
        return Enc(d)
    return fn


def _isize_own(which):
    def fn():
        rng = np.random.default_rng(50)
        d = Deflater()
        if which == "most_tokens":          # 1 literal + 21845 matches of length 3 at distance 1
            d.dynamic([7] + [(3, 1)] * 21845, final=True)
        elif which == "runs_258":
            d.dynamic([9] + [(258, 1)] * 254 + [(3, 1)], final=True)
        elif which == "match_ends_at_65535":
            d.dynamic(list(_text(rng, 65536 - 258)) + [(258, 8232)], final=True)
        elif which == "match_starts_at_65533":
            d.dynamic(list(_text(rng, 65533)) + [(3, 32765)], final=True)
        elif which == "dist_32768":
            toks = list(_text(rng, 32768)) + [(258, 32768)]
            toks += list(_text(rng, 65536 - 32768 - 258 - 20)) + [(17, 32768), (3, 32768)]
            d.dynamic(toks, final=True)
        elif which == "stored_noise_then_compressed":
            d.stored(_noise(rng, 30000))
            d.dynamic(lz_parse((_text(rng, 1777) * 21)[:35536]), final=True)
        assert len(d.out) == 65536
        return Enc(d)
    return fn


def _header_phase(bit):
    """a dynamic block whose header starts at bit `bit` of CDATA, behind a fixed block of literals (8 bits below 144, 9 bits from there)"""
    def fn():
        nine = next(b for b in range(8) if (bit - 10 - 9 * b) % 8 == 0)
        eight = (bit - 10 - 9 * nine) // 8
        d = Deflater()
        d.fixed([65 + k % 26 for k in range(eight)] + [200 + k for k in range(nine)])
        assert d.bitpos == bit
        rng = np.random.default_rng(bit)
        d.dynamic(lz_parse(_text(rng, 12) + _text(rng, 9) * 4), final=True)
        return Enc(d, header_bit=d.blocks[1]["start"])
    return fn


_CHAIN_LITS = [65] + list(range(97, 110))  # 14 literals


def _chain_codes():
    ll, dl = [0] * 286, [0] * 30
    for s, n in chain_lengths(_CHAIN_LITS + [256, 284]).items():  # 65: 1 bit ... 256 and 284: 15 bits
        ll[s] = n
    for s, n in chain_lengths(list(range(14)) + [15, 29]).items():  # distance symbol 0: 1 bit ... 15 and 29: 15 bits
        dl[s] = n
    return ll, dl


def _longest_match_symbol():
    """length code 284 of 15 bits + 5 extra, distance code 29 of 15 bits + 13 extra: 48 bits in one symbol, behind 0 .. 63 literals of one
    bit each so that it starts at every offset of a 64-bit window.  Every code length 1..15 of both alphabets is in use."""
    ll, dl = _chain_codes()
    rng = np.random.default_rng(60)
    toks = [65] * 33000 + list(_CHAIN_LITS)
    for k in range(14):  # every distance symbol of the chain once
        toks.append((227 + k, DIST_BASE[k], 27))
    toks.append((250, DIST_BASE[15], 27))
    for k in range(64):
        toks += [65] * k + [(227 + int(rng.integers(0, 32)), int(rng.integers(24577, 32769)), 27)]
    toks += [(258, 32768, 27), (257, 24577, 27)]
    d = Deflater()
    d.dynamic(toks, final=True, ll=ll, dl=dl)
    return Enc(d)


def _all_lengths_all_dists():
    rng = np.random.default_rng(61)
    toks = list(_text(rng, 4000, b"ACGTN.-"))
    for n in range(3, 259):  # (4000 + 33408 + 256 bytes: the distances behind them may be 32768)
        toks.append((n, int(rng.integers(1, 4001))))
        toks.append(int(rng.integers(65, 91)))
    toks.append((258, 5, 27))  # 258 as code 284 with extra 31
    toks.append((258, 32768, 27))
    for s in range(30):
        toks += [(3, DIST_BASE[s]), 66, (4, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1), 67]
    d = Deflater()
    d.dynamic(toks[:2000])
    d.fixed(toks[2000:4300])
    d.dynamic(toks[4300:], final=True)
    return Enc(d)


def _matches(which):
    def fn():
        rng = np.random.default_rng(70)
        d = Deflater()
        if which == "self_overlap":
            toks = []
            for dist in (1, 2, 3, 7, 257):
                toks += list(_noise(rng, dist)) + [(258, dist)]
            d.dynamic(toks, final=True)
        elif which == "dist_near_length":
            toks = list(_noise(rng, 40))
            for n in (3, 4, 10, 64, 200, 258):
                for dist in (n - 1, n, n + 1):
                    toks += [(n, dist), int(rng.integers(0, 256))]
                toks += list(_noise(rng, 259))
            d.fixed(toks, final=True)
        elif which == "dist_is_position":
            toks = [1, 2, 3, 4, 5, (5, 5), (258, 10), (100, 268)]
            toks += list(_text(rng, 32768 - 368)) + [(258, 32768)]
            d.dynamic(toks, final=True)
        elif which == "deep_chain":  # every match copies the bytes of the match in front of it: 21000 deep
            d.dynamic([1, 2, 3] + [(3, 3)] * 21000, final=True)
        elif which == "deep_chain_far":  # the same through matches of 5 at distance 7, two interleaved chains
            d.dynamic(list(range(10, 17)) + [(5, 7)] * 13000, final=True)
        elif which == "into_stored_block":
            d.stored(_noise(rng, 700))
            d.dynamic([(258, 700), (3, 1), (50, 958), 5, (258, 300)])
            d.stored(_noise(rng, 1))
            d.fixed([(4, 1), (200, 1215)], final=True)
        elif which == "into_previous_blocks_match":
            d.dynamic(list(_noise(rng, 30)) + [(100, 30)])
            d.dynamic([(100, 100), (258, 65)])
            d.fixed([(258, 258), (3, 746)])
            d.dynamic([(258, 1)] * 20 + [(258, 258 * 20)], final=True)
        return Enc(d)
    return fn


def _header_spelling(which):
    def fn():
        rng = np.random.default_rng(80)
        d = Deflater()
        text = _text(rng, 300, b"abcdefgh") + _text(rng, 40, b"ab") * 5
        toks = lz_parse(text)
        if which == "hlit_0":
            toks = list(text)
            ll, _ = d.auto_lengths(toks)
            d.dynamic(toks, final=True, ll=ll, dl=[0], hlit=0, hdist=0)
        elif which == "hlit_29":
            d.dynamic(toks, final=True, hlit=29)
        elif which == "hdist_29":
            d.dynamic(toks, final=True, hdist=29)
        elif which == "hclen_15":
            d.dynamic(toks, final=True, hclen=15)
        elif which == "hclen_smallest":  # 16, 17, 18, 0 and 8: every code is 8 bits - 255 literals and the end-of-block code -, no distance code
            data = bytes(rng.integers(0, 255, 500, dtype=np.uint8))
            cl = [0] * 19
            cl[0] = cl[8] = 1
            d.dynamic(list(data), final=True, ll=[8] * 255 + [0, 8], dl=[0], hclen=1, cl=cl, spelling="none")
        elif which == "cl_7_bits":
            ll, dl = d.auto_lengths(toks)
            items = greedy_spell(ll[:257 + max(k for k in range(29) if ll[257 + k]) + 1] + dl[:max(k for k in range(30) if dl[k]) + 1])
            f = {}
            for s, _ in items:
                f[s] = f.get(s, 0) + 1
            used = sorted(f, key=lambda s: (-f[s], s))
            assert len(used) <= 8
            used += [s for s in range(19) if s not in f][:8 - len(used)]
            cl = [0] * 19
            for s, n in chain_lengths(used).items():
                cl[s] = n
            assert max(cl) == 7 and all(cl[s] for s in f)
            d.dynamic(toks, final=True, ll=ll, dl=dl, cl=cl)
        elif which in ("16_across_boundary", "16_after_18", "16_after_17", "17_ends_at_the_end", "18_of_138", "no_run_codes"):
            # literals 138 (1 bit), 139 (2 bits); the end-of-block code and length 3 (257) at 3 bits; 3 distance codes: 1, 2, 2 bits or 2 x 4
            ll = [0] * 258
            ll[138], ll[139], ll[256], ll[257] = 1, 2, 3, 3
            toks = [138, 139, 138, 138, (3, 1), 139, (3, 2), (3, 3), 138]
            if which == "16_across_boundary":   # HLIT 0: the end-of-block code's 3 is the last literal length; the 16 behind it repeats it
                ll = ll[:257]                   # into the first six of eight distance codes of 3 bits
                ll[140] = 3
                items = greedy_spell(ll[:256]) + [(3, 0), (16, 3), (3, 0), (3, 0)]
                d.dynamic([138, 139, 140, 138, 138], final=True, ll=ll, dl=[3] * 8, hlit=0, spelling=items)
            elif which == "16_after_18":
                items = [(18, 127), (1, 0), (2, 0), (18, 102), (16, 0)] + greedy_spell(ll[256:] + [1, 2, 2])  # 116 zeros: 113 + 3
                assert expand_spelling(items) == ll + [1, 2, 2]
                d.dynamic(toks, final=True, ll=ll, dl=[1, 2, 2], spelling=items)
            elif which == "16_after_17":
                items = [(18, 127), (1, 0), (2, 0), (18, 83), (17, 7), (16, 3), (16, 3)] + greedy_spell(ll[256:] + [1, 2, 2])  # 94 + 10 + 6 + 6
                assert expand_spelling(items) == ll + [1, 2, 2]
                d.dynamic(toks, final=True, ll=ll, dl=[1, 2, 2], spelling=items)
            elif which == "17_ends_at_the_end":
                dl = [1, 2, 2, 0, 0, 0, 0]
                items = greedy_spell(ll + dl)
                assert items[-1] == (17, 1)
                d.dynamic(toks, final=True, ll=ll, dl=dl, hdist=6, spelling=items)
            elif which == "18_of_138":
                items = greedy_spell(ll + [1, 2, 2])
                assert items[0] == (18, 127)
                d.dynamic(toks, final=True, ll=ll, dl=[1, 2, 2], spelling=items)
            else:
                d.dynamic(toks, final=True, ll=ll, dl=[1, 2, 2], spelling="none")
        return Enc(d, header=d.headers[-1])
    return fn


SEAMS = [511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 30000]


def valid_forms():
    """the valid forms, in a fixed order"""
    f = []
    # ---- framing of other writers (the caller's bytes)
    for kind, per_block in (("dynamic", 1 << 30), ("dynamic", 1500), ("fixed", 4000)):
        for phase in range(8):
            f.append(Form("go_close_%s_%s_phase%d" % (kind, "one" if per_block > 1 << 20 else "cut", phase), "go_close", _go_close(kind, phase, per_block),
                          size=(65536, 30011, 4099, 300)[phase % 4] if kind == "dynamic" else 9001, phase=phase, go_close=True))
    f.append(Form("go_close_stored", "go_close", _go_close("stored", 0, 0), size=45001, phase=0, go_close=True))
    f.append(Form("go_literals_only", "go_close", _go_literals_only(1), size=20011, go_close=True))
    f.append(Form("no_dist_codes", "go_close", _go_literals_only(0), size=777, go_close=True))
    f.append(Form("flush_blocks", "blocks", _flush_blocks, size=40000))
    f.append(Form("many_blocks", "blocks", _many_blocks, size=7001))
    f.append(Form("isize_65536_records", "blocks", _isize_parsed(False), size=65536, isize=65536))
    f.append(Form("isize_65536_literals_only", "blocks", _isize_parsed(True), size=65536, isize=65536))
    for at in SEAMS:
        f.append(Form("stored_ends_at_%d" % at, "stored_seams", _stored_then_dynamic(at), size=at + (3000 if at < 30000 else 35536), stored_end=at))
    for phase in range(8):
        f.append(Form("stored_after_compressed_phase%d" % phase, "stored_seams", _stored_after_compressed(phase), size=1500 + 211 * phase, phase=phase))
    f.append(Form("two_stored_blocks", "stored_seams", _two_stored, size=5000))
    f.append(Form("largest_stored_block", "stored_seams", _largest_stored, size=MAX_CDATA - 5, isize=MAX_CDATA - 5))
    for seed in range(4):
        f.append(Form("deep_codes_%d" % seed, "deep_codes", _deep_codes(seed), size=(20000, 6000, 65536, 900)[seed], **({"isize": 65536} if seed == 2 else {})))
    # ---- content of their own
    f.append(Form("one_dist_code_symbol_0", "one_dist_code", _one_dist_code(0), own=True))
    f.append(Form("one_dist_code_symbol_29", "one_dist_code", _one_dist_code(29), own=True))
    for which in ("most_tokens", "runs_258", "match_ends_at_65535", "match_starts_at_65533", "dist_32768", "stored_noise_then_compressed"):
        f.append(Form("isize_65536_" + which, "isize_65536", _isize_own(which), own=True, isize=65536, **({"ntok": 21846} if which == "most_tokens" else {})))
    for bit in range(505 * 8, 520 * 8):
        f.append(Form("header_at_bit_%d" % bit, "header_phase", _header_phase(bit), own=True, header_bit=bit))
    f.append(Form("longest_match_symbol", "codes", _longest_match_symbol, own=True))
    f.append(Form("all_lengths_all_dists", "codes", _all_lengths_all_dists, own=True))
    for which in ("hlit_0", "hlit_29", "hdist_29", "hclen_15", "hclen_smallest", "cl_7_bits", "16_across_boundary", "16_after_18", "16_after_17",
                  "17_ends_at_the_end", "18_of_138", "no_run_codes"):
        f.append(Form("header_" + which, "header_spellings", _header_spelling(which), own=True))
    for which in ("self_overlap", "dist_near_length", "dist_is_position", "deep_chain", "deep_chain_far", "into_stored_block", "into_previous_blocks_match"):
        f.append(Form("matches_" + which, "matches", _matches(which), own=True))
    return f


DATA_GROUPS = ["go_close", "blocks", "stored_seams", "deep_codes"]


_INVALID_TEXT = b"the quick brown fox jumps over the lazy dog " * 6


def lax_output(name, isize, previous):
    """for the invalid forms whose bit stream is well-formed: the `isize` bytes a decoder that lacked the one check the form is about
    would leave behind (`previous`: the inflated bytes in front of the member; what lies behind a too short output is taken as zeros).
    A member framed with the CRC-32 of these bytes can be refused by the decoder's own check only.  None: there are no such bytes."""
    if name in ("output_longer_than_isize", "output_much_longer_than_isize", "stored_longer_than_isize", "output_shorter_than_isize",
                "output_much_shorter_than_isize"):
        return (_INVALID_TEXT + bytes(isize))[:isize]
    if name == "distance_into_the_previous_member":
        return previous[-1:] * 6
    if name == "distance_one_more_than_the_position":
        return b"a" + previous[-1:] + b"a" + previous[-1:]
    return None


# ---- the invalid forms: (name, cdata, claimed isize).  Each is a member no inflater may accept.
def invalid_forms():
    out = []

    def add(name, d, isize=None, cut=None, pad=b""):
        c = d.getvalue() + pad
        out.append((name, c if cut is None else c[:cut], len(d.out) if isize is None else isize))

    text = _INVALID_TEXT
    toks = lz_parse(text)
    d = Deflater()
    d.bits(1, 1); d.bits(3, 2); d.bits(0, 29); add("btype_3", d, 10, pad=bytes(8))
    d = Deflater()
    d.stored(text, final=True, nlen=(~len(text) & 0xFFFF) ^ 0x0100); add("stored_len_not_nlen", d)
    d = Deflater()
    d.stored(text, final=True); add("stored_past_cdata", d, cut=5 + len(text) - 30)
    ll, dl = Deflater().auto_lengths(toks)
    for name, kw in (("hlit_30", dict(hlit=30)), ("hlit_31", dict(hlit=31)), ("hdist_30", dict(hdist=30)), ("hdist_31", dict(hdist=31))):
        d = Deflater()
        d.header(ll + [0] * 8, dl + [0] * 8, final=True, check=False, **kw)
        d._symbols(toks, ll, dl)
        add(name, d)
    base_items = greedy_spell(ll[:257 + 29] + dl)

    def with_cl(name, cl, items=None, hclen=15):
        d = Deflater()
        d.header(ll, dl, final=True, hlit=29, hdist=29, check=False, cl=cl, hclen=hclen, spelling=base_items if items is None else items)
        d.bits(0, 64)
        add(name, d, len(text))
    d = Deflater()
    d.header(ll, dl, final=True, hlit=29, hdist=29)
    over = list(d.headers[-1]["cl"])  # a complete code-length code, and one more code of one bit
    over[over.index(0)] = 1
    assert kraft(over) > 1
    with_cl("cl_code_oversubscribed", over)
    with_cl("cl_code_incomplete", [2 if s in (0, 18) else 0 for s in range(19)], items=[(18, 127), (0, 0)])
    cl16 = [0] * 19
    cl16[16] = cl16[0] = 1
    with_cl("first_length_is_16", cl16, items=[(16, 0), (0, 0)])
    # a run past nlen + ndist: 29 distance lengths are left and the last 18 brings 138 zeros
    items = greedy_spell(ll[:257 + 29] + dl[:1]) + [(18, 127)]
    h = huff_lengths({s: 1 for s, _ in items}, 7)
    d = Deflater()
    d.header(ll, dl, final=True, hlit=29, hdist=29, check=False, cl=[h.get(s, 0) for s in range(19)], spelling=items)
    d.bits(0, 64)
    add("run_past_the_lengths", d, len(text))

    def with_lengths(name, ll2, dl2, body=None, isize=None):
        d = Deflater()
        d.header(ll2, dl2, final=True, check=False)
        if body:
            body(d)
        else:
            d.bits(0, 64)
        add(name, d, len(text) if isize is None else isize)
    no_eob = list(ll)
    no_eob[256] = 0
    with_lengths("no_end_of_block_code", no_eob, dl)
    over = list(ll)
    over[over.index(0)] = 1
    with_lengths("literal_code_oversubscribed", over, dl)
    inc = [0] * 257
    inc[97] = inc[98] = inc[256] = 2
    with_lengths("literal_code_incomplete", inc, [1, 1])
    with_lengths("distance_code_oversubscribed", ll, [1, 1, 1])
    with_lengths("distance_code_incomplete", ll, [2, 2, 2])

    def unused_pattern(d):  # 'a' 'a' 'a', then length 3 and the bit 1 where the only distance code is 0
        c = canonical(ll3)
        for s in (97, 97, 97, 257):
            d.bits(*c[s])
        d.bits(1, 1)
        d.bits(*c[256])
        d.bits(0, 32)
    ll3 = [0] * 258
    ll3[97], ll3[256], ll3[257] = 1, 2, 2
    with_lengths("unused_pattern_of_the_single_distance_code", ll3, [1], unused_pattern, 6)
    with_lengths("match_without_distance_codes", ll3, [0], unused_pattern, 6)
    for sym in (286, 287):
        d = Deflater()
        d.bits(1, 1); d.bits(1, 2)
        c = canonical(FIXED_LL)
        d.bits(*c[97]); d.bits(*c[sym]); d.bits(0, 5); d.bits(*c[256]); d.bits(0, 32)
        add("fixed_symbol_%d" % sym, d, 4)
    for sym in (30, 31):
        d = Deflater()
        d.bits(1, 1); d.bits(1, 2)
        c = canonical(FIXED_LL)
        d.bits(*c[97]); d.bits(*c[257]); d.bits(*canonical(FIXED_D)[sym]); d.bits(*c[256]); d.bits(0, 32)
        add("fixed_distance_%d" % sym, d, 4)
    d = Deflater()
    d.bits(1, 1); d.bits(1, 2)
    c = canonical(FIXED_LL)
    d.bits(*c[97]); d.bits(*c[257]); d.bits(*canonical(FIXED_D)[1]); d.bits(*c[256]); d.bits(0, 32)
    add("distance_one_more_than_the_position", d, 4)
    d = Deflater()
    d.bits(1, 1); d.bits(1, 2)
    d.bits(*c[260]); d.bits(*canonical(FIXED_D)[0]); d.bits(*c[256]); d.bits(0, 32)
    add("distance_into_the_previous_member", d, 6)
    for name, delta in (("output_longer_than_isize", -1), ("output_much_longer_than_isize", -200), ("output_shorter_than_isize", 1),
                        ("output_much_shorter_than_isize", 40000)):
        d = Deflater()
        d.dynamic(toks, final=True)
        add(name, d, len(text) + delta)
    d = Deflater()
    d.stored(text, final=True)
    add("stored_longer_than_isize", d, len(text) - 1)
    d = Deflater()
    d.dynamic(toks, final=True)
    add("ends_mid_symbol", d, cut=len(d.getvalue()) - 3)
    add("ends_in_the_header", d, cut=9)
    d = Deflater()
    d.dynamic(toks)
    add("no_final_block", d)
    d = Deflater()
    d.stored(text)
    add("no_final_block_stored", d)
    return out


def rejected(cdata, isize):
    """zlib's verdict on an invalid form: it raises, does not reach the end of the stream within CDATA, or gives another length"""
    o = zlib.decompressobj(-15)
    try:
        got = o.decompress(cdata)
    except zlib.error:
        return True
    return not o.eof or len(got) != isize
