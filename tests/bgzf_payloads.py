"""Payloads for the device's BGZF compressor (k_bgzf_deflate, elprep_amd/csrc/bgzf_out.hip; the algorithm: deflate_core.hpp) at the seams
of its match finder, its window, its parts and its blocks - and the way onto the device: records_for() packs payloads into BAM records
whose optional field lands on whole 65280-byte blocks of the record stream.  BAM records of sequencing reads never hold a match that
ends on the payload's last byte, a source exactly 32768 or 32769 bytes back, a block without any match, or a block a few bytes on
either side of the stored fallback; the payloads here do, and every one comes with the facts a test can hold the writer to
(tests/test_bgzf_payloads_cpu.py on the host emulation tests/deflate_host.cpp, tests/test_gpu_deflate_seams.py on the device;
tests/deflate_tokens.py reads the tokens).  Everything is generated from fixed seeds.

payloads() yields (name, bytes, facts); facts["group"] says what the payload is for:
  a  planted copies in zero filler: distance x length x phase.  The block is zeros (all zero words share bucket 0 of hash4: they evict
     nothing else).  An island of `length` random bytes in 1..200 lies at s = p - dist, byte 201 in front of it and 203 behind it; its
     copy lies at p, 202 in front and 204 behind.  Every landing of the parse inside the copy finds its source inserted by an EARLIER
     strip, and all 4-byte words that touch a non-zero byte lie in buckets of their own, none in bucket 0 (_Block.check): neither the
     order of the threads nor a lost racing insert can take the source away.  So the tokens over [p, p + length) follow a plain rule,
     expected_tokens().  facts["plants"] = [(p, length, dist)].  The sweep: A_DISTS x A_LENGTHS x A_PHASES (p mod 256), as many plants
     to a block as find room and buckets; "short" is the closest source, length + 2 back (203 and 202 side by side) - or p mod 256 + 1
     where that is more, so that the source still lies in the strip in front; 300 bytes from 300 back do not exist (the copy would
     begin inside its island).
  b  the same with the source beyond the 32 KB window: no match may touch the copy (facts["no_match"] = [(lo, hi)]), and no block
     anywhere may hold a distance above 32768.
  c  the payload's end: copies that end at n, n - 1, n - 2, n - 3; copies cut off by the payload's end after 1, 2, 3 bytes (fewer than
     MINM are left: no match); zero runs up to the last byte - in a full block and in a short last one, where what lies behind the
     payload in LDS is zero padding that looks like more of the run.
  d  no match at all: a de Bruijn sequence B(16, 4) (every 4-byte window differs), the same with every byte moved to 144..159 (9-bit
     fixed codes), prefixes.  facts["match_free"]: the tokens cannot depend on the schedule, so the bytes of all orders are the same.
  e  few distance codes: a one-byte run that only the first strip sees (the table is empty during its look-ups, only the byte in front
     is a candidate: distance 1 and nothing else - facts["one_distance_code"]) in front of match-free bytes or alone; a one-byte run of
     65280 (which is NOT one distance code: from the second strip on the hash table's candidate wins the tie against the byte in front,
     with the distance the schedule left there).  b"xxxy" (no distance code at all) and two-value noise are among g's.
  f  the stored fallback: noise, and noise with the last t bytes zero - facts["kind"] / facts["kind_fixed"] = the form the emulation
     must choose with dynamic codes allowed / with fixed codes only (0 fixed, 1 stored, 2 dynamic).
  g  the payloads of tests/test_deflate_cpu.py (imported).

Sizes over the catalogue on the host emulation, measured by tests/test_bgzf_payloads_cpu.py (which fails if they move): the largest
difference in DEFLATE size between the thread orders 0 and 1 is DELTA = 267 bytes (with fixed codes only, orders 16 and 17:
DELTA_FIXED = 2233 bytes).  Both come from one payload, "g two values": noise of two byte values, where every look-up finds some
match and which one depends on who wrote the bucket last.  By group the difference is GROUP_DELTA: 12, 12 and 11 bytes for the
planted blocks of a, b and c, 9 for e, 0 for d and f.
The device may run a legal schedule that neither order reproduces, so the device test compares a block's type with the emulation's
only where both orders choose the same form and the form wins against the next one (fixed codes, dynamic codes, stored) by more than
a band, exempt().  The band is 4 * the payload's GROUP's difference, and one byte's rounding at the least - not 4 * DELTA: a block of
zeros with plants takes 250 bytes with dynamic codes and 500 with fixed ones, and a band of 4 * 267 bytes around every choice would
exempt 19 payloads in 20 and leave the comparison empty.  Within a group the payloads are of one make, and the group's largest
difference says what a schedule can move there."""
import ctypes as C
import struct

import numpy as np

PAYLOAD, PART, STRIP, MINM, MAXL, WINDOW, HBITS = 65280, 255, 256, 4, 255, 32768, 12
DELTA, DELTA_FIXED = 267, 2233
GROUP_DELTA = {"a": 12, "b": 12, "c": 11, "d": 0, "e": 9, "f": 0, "g": 267}
N_SHORT = 40001  # the short last block of group c

A_DISTS = ["short", 300, 511, 512, 513, 4096, 4097, 16384, 16385, 24576, 24577, 32767, 32768]
A_LENGTHS = [4, 5, 6, 7, 8, 9, 12, 13, 100] + list(range(250, 260)) + [300]
A_PHASES = [0, 1, 2, 3, 250, 251, 252, 253, 254, 255]
B_DISTS = [32769, 32770, 33000, 50000, 65000]


def hash4(w):
    """deflate_core.hpp hash4 on an array of 4-byte words"""
    return ((np.asarray(w, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HBITS)


def expected_tokens(p, length, dist):
    """the matches over the copy [p, p + length) of a plant: the parse lands on p; wherever it lands, the finder's note is the rest of
    the copy (MAXL at the most) at `dist`, and the parse cuts it at the end of its 255-byte part; fewer than MINM bytes are literals"""
    out, q, end = [], p, p + length
    while q < end:
        l = min(end - q, PART - q % PART, MAXL)
        if l >= MINM:
            out.append((q, l, dist))
            q += l
        else:
            q += 1
    return out


def _landings_see_their_source(p, length, dist):
    """every landing of expected_tokens() that is a match has its source position in an earlier strip than itself"""
    return all((q - dist) // STRIP < q // STRIP for q, _, _ in expected_tokens(p, length, dist))


class _Block:
    """a payload of zeros that takes plants; keeps which bytes are taken and which word owns which bucket"""
    BUDGET = 2600  # buckets in use at the most: a new word finds a free one at the first tries

    def __init__(self, n, rng):
        self.n, self.rng = n, rng
        self.b = bytearray(n)
        self.taken = np.zeros(n + 16, bool)
        self.used = {0: 0}  # bucket -> the word in it
        self.plants, self.no_match = [], []

    def _free(self, lo, hi):
        return lo >= 0 and not self.taken[max(lo, 0):hi].any()

    def _island(self, length, cut, tail, gap):
        """`length` bytes in 1..200, drawn one by one so that every word they complete in the plant's surroundings - 0 0 0 201 | island |
        203 | `gap` zeros | 202 | the island's first `cut` bytes | 204 0 0 0 (zeros where the payload ends: `tail` = False) - gets a
        bucket of its own; a byte that finds none sends the one in front of it back.  None if that does not help."""
        stream = [0, 0, 0, 201] + [-1 - j for j in range(length)] + [203] + [0] * min(gap, 3) + [202] + [-1 - j for j in range(cut)] + \
            ([204, 0, 0, 0] if tail else [0, 0, 0])
        by_last = [[] for _ in range(length + 1)]  # the windows that byte j completes ([length]: those without a byte of the island)
        for k in range(len(stream) - 3):
            win = tuple(stream[k:k + 4])
            last = max([-1 - x for x in win if x < 0], default=length)
            if any(win) and win not in by_last[last]:
                by_last[last].append(win)
        used = self.used
        new, claims, isl = {}, [], []

        def claim(words, shared=False):
            """the words' buckets if they are free (shared: or hold the same word - the words around the marks alone, which all plants
            have; a word with a byte of an island must not occur in another plant: it would be a match there)"""
            mine = {}
            for w in words:
                h = ((w * 2654435761) & 0xFFFFFFFF) >> (32 - HBITS)
                have = used.get(h)
                if have is None:
                    have = new.get(h, mine.get(h))
                if have is None:
                    mine[h] = w
                elif not shared or have != w:
                    return None
            return mine

        fixed = claim([w[0] | w[1] << 8 | w[2] << 16 | w[3] << 24 for w in by_last[length]], shared=True)
        if fixed is None:
            return None
        new.update(fixed)
        backtracks = 0
        while len(isl) < length:
            j = len(isl)
            parts = []  # of every window that byte j completes: the bytes there are, and where byte j goes
            for win in by_last[j]:
                parts.append((sum((x if x >= 0 else isl[-1 - x]) << (8 * k) for k, x in enumerate(win) if x != -1 - j),
                              sum(1 << (8 * k) for k, x in enumerate(win) if x == -1 - j)))
            for c in self.rng.permutation(200) + 1:
                c = int(c)
                mine = claim([base + c * at for base, at in parts])
                if mine is not None:
                    new.update(mine)
                    claims.append(mine)
                    isl.append(c)
                    break
            else:
                backtracks += 1
                if not isl or backtracks > 300:
                    return None
                isl.pop()
                for h in claims.pop():
                    del new[h]
        self.used.update(new)
        return bytes(isl)

    def plant(self, length, dist, phase=None, p=None, cut=None, from_p=0):
        """an island of `length` bytes and the copy of its first `cut` (default: all) at p (given, or the first free place at or
        behind from_p with p % 256 = phase); False if the block has no room"""
        cut, p_given = length if cut is None else cut, p
        if len(self.used) + 2 * length + 16 > self.BUDGET:
            return False
        if p is None:
            p = max(from_p, dist + 8)
            p += (phase - p) % STRIP
        while True:
            s = p - dist
            if p + cut + (8 if p_given is None else 0) > self.n:  # (only a copy at a given p may lie at the payload's end)
                return False
            if s >= 8 and dist >= length + 2 and self._free(s - 8, s + length + 8) and self._free(p - 8, p + cut + 8) and \
                    (cut < MINM or _landings_see_their_source(p, cut, dist)):
                break
            if phase is None:
                return False
            p += STRIP
        tail = p + cut < self.n
        for _ in range(5):
            isl = self._island(length, cut, tail, dist - length - 2)
            if isl is not None:
                break
        else:
            return False
        b = self.b
        b[s - 1], b[s + length] = 201, 203
        b[s:s + length] = isl
        b[p - 1] = 202
        b[p:p + cut] = isl[:cut]
        if tail:
            b[p + cut] = 204
        self.taken[s - 8:s + length + 8] = True
        self.taken[p - 8:p + cut + 8] = True
        if cut >= MINM and dist <= WINDOW:
            self.plants.append((p, cut, dist))
        else:
            self.no_match.append((p, p + cut))
        self.last_p = p
        return True

    def check(self):
        """all 4-byte words with a non-zero byte: different words in different buckets, none in the zero word's (hash4 in numpy)"""
        a = np.frombuffer(bytes(self.b) + bytes(3), dtype=np.uint8).astype(np.uint64)
        w = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
        u, count = np.unique(w[w != 0], return_counts=True)
        h = hash4(u)
        assert np.unique(h).size == u.size and not (h == 0).any()
        marks = [201 << 24, 202 << 24, 203, 204]  # (a word with a byte of an island: in the island and in its copy, nowhere else)
        assert (count[~np.isin(u, marks)] <= 2).all()
        return bytes(self.b)


def _sweep(rng, dists, lengths, phases, group, label=None):
    """every (dist, length, phase) as a plant, as many to a block as find room and buckets"""
    out, blk, at = [], None, 0
    for dist in dists:
        for phase in phases:
            for length in lengths:
                d = max(length + 2, phase + 1) if dist == "short" else dist
                if d < length + 2:  # (300 bytes from 300 back: the copy would begin inside its island)
                    continue
                if blk is None or not blk.plant(length, d, phase, from_p=at):
                    if blk is not None:
                        out.append(blk)
                    blk = _Block(PAYLOAD, rng)
                    assert blk.plant(length, d, phase), (dist, length, phase)
                at = blk.last_p + length + 16
    out.append(blk)
    for k, blk in enumerate(out):
        yield "%s plants %d" % (label or group, k), blk.check(), {"group": group, "plants": blk.plants, "no_match": blk.no_match}


def de_bruijn(k=16, n=4):
    """B(k, n) by the Lyndon words' concatenation: k^n symbols in which, read cyclically, every n-window occurs once"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


_CACHE = {}


def payloads():
    """[(name, bytes, facts)], built once"""
    if "all" not in _CACHE:
        _CACHE["all"] = list(_payloads())
        names = [name for name, _, _ in _CACHE["all"]]
        assert len(set(names)) == len(names)
        assert all(0 < len(data) <= PAYLOAD for _, data, _ in _CACHE["all"])
    return _CACHE["all"]


def _payloads():
    from tests.test_deflate_cpu import _cases, _edge_cases
    # a, b
    yield from _sweep(np.random.default_rng(101), A_DISTS, A_LENGTHS, A_PHASES, "a")
    rng = np.random.default_rng(102)
    yield from _sweep(rng, B_DISTS[:3], A_LENGTHS, [0, 255], "b")
    yield from _sweep(rng, [50000], A_LENGTHS, [3], "b", "b far")
    for length in (4, 9, 100, 250):  # (65000 back: one plant fills the block's ends)
        blk = _Block(PAYLOAD, rng)
        assert blk.plant(length, 65000, p=65000 + 11)
        yield "b 65000 back, %d bytes" % length, blk.check(), {"group": "b", "plants": [], "no_match": blk.no_match}
    # c
    rng = np.random.default_rng(103)
    for n, far in ((PAYLOAD, 32768), (N_SHORT, 32768)):
        size = "full" if n == PAYLOAD else "short"
        for e in range(4):
            for length in (4, 5, 6, 7, 8, 9, 13):
                blk = _Block(n, rng)
                assert blk.plant(length, far if (e + length) % 2 else 300, p=n - e - length)
                assert blk.plants == [(n - e - length, length, far if (e + length) % 2 else 300)]
                yield "c %s: %d bytes end at n - %d" % (size, length, e), blk.check(), {"group": "c", "plants": blk.plants, "no_match": []}
        for cut in (1, 2, 3):
            blk = _Block(n, rng)
            assert blk.plant(8, 300 if cut % 2 else far, p=n - cut, cut=cut) and blk.no_match == [(n - cut, n)]
            yield "c %s: a copy cut off after %d" % (size, cut), blk.check(), {"group": "c", "plants": [], "no_match": blk.no_match}
        noise = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
        yield "c %s: noise, then zeros to the end" % size, noise + bytes(n - 700), {"group": "c"}
    for n in (4, 5, 259, N_SHORT):
        yield "c %d zeros" % n, bytes(n), {"group": "c"}
    # d
    db = de_bruijn()[:PAYLOAD]
    w = np.frombuffer(db, dtype=np.uint8).astype(np.uint32)
    assert np.unique(w[:-3] | w[1:-2] << 8 | w[2:-1] << 16 | w[3:] << 24).size == PAYLOAD - 3
    yield "d de Bruijn", db, {"group": "d", "match_free": True, "kind": 2, "size": 33160}
    yield "d de Bruijn in 144..159", bytes(c + 144 for c in db), {"group": "d", "match_free": True, "kind": 2}
    for n in (1, 2, 3, 4, 255, 256, 257):
        yield "d de Bruijn, %d bytes" % n, db[:n], {"group": "d", "match_free": True}
    # e
    yield "e one value", b"\xc8" * PAYLOAD, {"group": "e", "kind": 2}
    yield "e one strip of one value, then de Bruijn", b"\xc8" * 256 + db[:PAYLOAD - 256], {"group": "e", "one_distance_code": True, "kind": 2}
    yield "e 255 of one value", b"\xc8" * 255, {"group": "e", "one_distance_code": True}
    yield "e 256 of one value", b"\xc8" * 256, {"group": "e", "one_distance_code": True}
    # f
    rng = np.random.default_rng(104)
    noise = rng.integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes()
    yield "f noise", noise, {"group": "f", "kind": 1, "kind_fixed": 1}
    for t in (8, 16, 32, 48, 64, 128, 256):
        yield "f noise, %d zeros" % t, noise[:PAYLOAD - t] + bytes(t), {"group": "f", "kind": 1 if t <= 48 else 2, "kind_fixed": 1}
    # g ("empty" is no block of a stream: left out)
    for name, data in list(_cases()) + list(_edge_cases().items()):
        if data:
            facts = {"group": "g"}
            if name == "one symbol many times":  # b"xxxy": literals only
                facts["match_free"] = True
            yield "g " + name, data, facts


def full_blocks():
    return [(name, data, facts) for name, data, facts in payloads() if len(data) == PAYLOAD]


def short_blocks():
    return [(name, data, facts) for name, data, facts in payloads() if len(data) < PAYLOAD]


# ---- what holds for the tokens of a payload's block, wherever it was compressed
def check_tokens(block, data, facts, name):
    """block: deflate_tokens.Block of the payload `data` - the claims of the payload's facts, and those that hold everywhere"""
    from tests import deflate_tokens as dt
    assert block.data == data, name
    for pos, length, dist in block.matches:
        assert 3 <= length <= 258 and 1 <= dist <= min(pos, WINDOW), (name, pos, length, dist)
    for p, length, dist in facts.get("plants", ()):
        got = [m for m in block.matches if m[0] < p + length and m[0] + m[1] > p]
        assert got == expected_tokens(p, length, dist), (name, (p, length, dist), got)
    for lo, hi in facts.get("no_match", ()):
        got = [m for m in block.matches if m[0] < hi and m[0] + m[1] > lo]
        assert not got, (name, (lo, hi), got)
    if facts.get("match_free"):
        assert not block.matches and block.n_literals == len(data), name
    if facts.get("one_distance_code"):
        assert dt.used_distance_symbols(block) == {0}, name
        if block.btype == 2:
            assert [l for l in block.d_lens if l] in ([1], [1, 1]), (name, block.d_lens)


# ---- the host emulation
def emulation():
    if "lib" not in _CACHE:
        from tests.test_deflate_cpu import _build_lib
        L = _build_lib()
        L.dfl_last_sizes.restype = None
        L.dfl_last_sizes.argtypes = [C.c_void_p]
        _CACHE["lib"] = L
    return _CACHE["lib"]


def emulate(data, order):
    """-> (DEFLATE data, kind, tokens, (bytes with fixed codes, with dynamic codes, stored)) of tests/deflate_host.cpp; order: 0 / 1 the
    threads in index order / reversed, + 16 fixed codes only"""
    from tests.test_deflate_cpu import _deflate
    key = ("emu", data, order)
    if key not in _CACHE:
        cdata, kind, ntok = _deflate(emulation(), data, order)
        sizes = np.zeros(3, np.uint32)
        emulation().dfl_last_sizes(sizes.ctypes.data)
        _CACHE[key] = (cdata, kind, ntok, tuple(int(x) for x in sizes))
    return _CACHE[key]


def margin(data, fixed_only):
    """(kind, bytes by which the chosen form beats the next one) if both thread orders choose the same form, else (None, 0)"""
    kinds, margins = set(), []
    for order in (16, 17) if fixed_only else (0, 1):
        _, kind, _, (fixed, dyn, stored) = emulate(data, order)
        sizes = sorted([fixed, stored] if fixed_only else [fixed, dyn, stored])
        kinds.add(kind)
        margins.append(sizes[1] - sizes[0])
    return (kinds.pop(), min(margins)) if len(kinds) == 1 else (None, 0)


def exempt(data, facts, fixed_only):
    """the payload's block type on the device is not compared with the emulation's: the orders disagree, or the chosen form wins by no
    more than the band (the module's docstring)"""
    kind, by = margin(data, fixed_only)
    return kind is None or by <= 4 * max(GROUP_DELTA[facts["group"]], 1)


# ---- onto the device
PER_RECORD = 15  # payload blocks behind a record's first block
RG_ID = "seams"


def header():
    from elprep_amd.batch import Header
    return Header.from_read_groups(["chrS"], [1 << 20], [{"ID": RG_ID, "LB": "lib"}])


def records_for(blocks):
    """the payloads `blocks` (each 65280 bytes; the last may be shorter) as BAM records: unmapped reads of one read group with the data in
    one XB:B:C field, PER_RECORD payloads to a record.  A record's first 65280 bytes hold its fixed fields, name, read group and the
    field's first bytes (zeros); each payload lies on a block of its own behind that, so every record is a whole number of blocks long
    (but for a short last payload) and a record's head always opens a block.  No payload: one record of one block.  Records keep their
    order in a coordinate sort: unmapped, ascending POS.
    -> (the record stream, the records' offsets, [index in the stream of each payload's block])"""
    assert all(len(b) == PAYLOAD for b in blocks[:-1]) and (not blocks or 0 < len(blocks[-1]) <= PAYLOAD)
    out, offs, where, total = [], [0], [], 0
    for r, k in enumerate(range(0, max(len(blocks), 1), PER_RECORD)):
        mine = blocks[k:k + PER_RECORD]
        name = b"blocks%06d\0" % r
        rg = b"RGZ" + RG_ID.encode() + b"\0"
        head = 36 + len(name) + 2 + 4 + len(rg) + 8  # (four bases: two bytes of SEQ, four of QUAL)
        filler = bytes(PAYLOAD - head)
        n_tag = len(filler) + sum(len(b) for b in mine)
        size = head + n_tag - 4
        # refID -1, POS r, l_read_name, MAPQ 0, bin 4680, no CIGAR, FLAG 4, l_seq 4, mate -1 / -1, TLEN 0
        rec = struct.pack("<IiiBBHHHIiii", size, -1, r, len(name), 0, 4680, 0, 4, 4, -1, -1, 0) + name + b"\x12\x48" + b"\x1e" * 4 + rg + \
            b"XBBC" + struct.pack("<I", n_tag) + filler
        assert len(rec) == PAYLOAD
        first = total // PAYLOAD
        where += [first + 1 + j for j in range(len(mine))]
        out += [rec] + list(mine)
        total += PAYLOAD + sum(len(b) for b in mine)
        offs.append(total)
    return np.frombuffer(b"".join(out), dtype=np.uint8), np.asarray(offs, dtype=np.uint64), where


def record_names(stream):
    """the read names of a stream of BAM records, in its order"""
    names, p = [], 0
    while p < len(stream):
        size, l_name = struct.unpack_from("<I", stream, p)[0], stream[p + 12]
        names.append(bytes(stream[p + 36:p + 36 + l_name - 1]))
        p += 4 + size
    assert p == len(stream)
    return names
