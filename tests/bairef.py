"""The BAM index (SAM specification 5.2) restated for the tests of elp_index_sorted_bgzf / elp_index_merged_bgzf, in two pieces that share
nothing but the specification and this file's small readers of BGZF members and BAM records:

  build(bgzf, base_coffset, n_ref)   the canonical index of a stream of BGZF members that hold BAM records in coordinate order - what the
                                     device call must return, byte for byte (include/elprep_hip.h states the form)
  query(bai, bgzf, base_coffset, refid, beg, end)   a reader that USES an index: reg2bins, the linear index's cut, a seek to every chunk,
                                     -> the virtual offsets of the records that overlap [beg, end).  It knows nothing of build().

and the test side's writers: bam_record() and bgzf_write() (zlib, members of 65280 bytes, as the emitters frame them)."""
import functools
import struct
import zlib

PAYLOAD = 65280
PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X consume the reference


# ---- writers
def bam_record(refid, pos, flag=0, cigar=(), name=b"r", l_seq=1, pad=None, mapq=30, tags=b""):
    """one BAM alignment record, block_size field included.  pos: the BAM field (0-based; -1 for POS 0); cigar: (length, op code) pairs;
    pad: the length of the value of a ZP:Z field (None: no such field) - a record grows by 4 + pad bytes; tags: further fields, encoded"""
    rec = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, 0, len(cigar), flag, l_seq, -1, -1, 0)
    rec += name + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
    rec += bytes([0x11] * ((l_seq + 1) // 2)) + bytes([30] * l_seq) + tags
    if pad is not None:
        rec += b"ZPZ" + b"p" * pad + b"\0"
    return struct.pack("<I", len(rec)) + rec


def bgzf_write(stream, level=1, payload=PAYLOAD):
    """the stream as BGZF members of `payload` bytes (the last: what is left), DEFLATE by zlib"""
    out = []
    for at in range(0, len(stream), payload):
        part = stream[at:at + payload]
        if level == 0:  # one final stored block, written here: 5 bytes around the payload, whatever zlib's buffering would make of it
            cdata = b"\x01" + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
        else:
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            cdata = co.compress(part) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(cdata) + 8 - 1) + cdata
                   + struct.pack("<II", zlib.crc32(part), len(part)))
    return b"".join(out)


# ---- readers
@functools.lru_cache(maxsize=4)
def members(bgzf):
    """[(offset in bgzf, inflated payload)] and the offset behind the last member (kept for the last few streams: the tests ask again
    and again)"""
    out, p = [], 0
    while p < len(bgzf):
        assert bgzf[p:p + 4] == b"\x1f\x8b\x08\x04" and bgzf[p + 12:p + 16] == b"BC\x02\0", p
        bsize = struct.unpack_from("<H", bgzf, p + 16)[0] + 1
        data = zlib.decompress(bgzf[p + 18:p + bsize - 8], -15)
        assert len(data) == struct.unpack_from("<I", bgzf, p + bsize - 4)[0]
        out.append((p, data))
        p += bsize
    assert p == len(bgzf)
    return out, p


def record_fields(stream, at):
    """-> (size with the block_size field, refid, beg, end, flag) of the record at `at`: beg = max(pos, 0) - the BAM field is POS - 1 -,
    end = beg + the reference-consuming CIGAR operations, + 1 if those are 0 or the read is unmapped"""
    bs, refid, pos, l_name, _, _, n_cig, flag = struct.unpack_from("<IiiBBHHH", stream, at)
    span = 0
    for k in range(n_cig):
        c = struct.unpack_from("<I", stream, at + 36 + l_name + 4 * k)[0]
        if c & 15 in REF_OPS:
            span += c >> 4
    if span == 0 or flag & 4:
        span = 1
    beg = max(pos, 0)
    return 4 + bs, refid, beg, beg + span, flag


def reg2bin(beg, end):
    """the specification's function; end is exclusive"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


# ---- (a) the canonical index
def build(bgzf, base_coffset, n_ref):
    mem, total = members(bgzf)
    coff = [p for p, _ in mem] + [total]
    stream = b"".join(d for _, d in mem)
    assert all(len(d) == PAYLOAD for _, d in mem[:-1])

    def voff(p):
        return (base_coffset + coff[p // PAYLOAD]) << 16 | p % PAYLOAD

    contigs = [None] * n_ref  # per contig: bins {bin: [[beg, end], ...]}, windows {w: S}, first S, last E, mapped, unmapped
    n_no_coor, at = 0, 0
    while at < len(stream):
        size, refid, beg, end, flag = record_fields(stream, at)
        s, e = voff(at), voff(at + size)
        at += size
        if refid < 0:
            n_no_coor += 1
            continue
        if end > 1 << 29:
            raise ValueError("a record ends beyond 2^29")
        c = contigs[refid]
        if c is None:
            c = contigs[refid] = dict(bins={}, win={}, first=s, last=e, n=[0, 0])
        c["last"] = e
        c["n"][1 if flag & 4 else 0] += 1
        chunks = c["bins"].setdefault(reg2bin(beg, end), [])
        if chunks and s >> 16 == chunks[-1][1] >> 16:
            chunks[-1][1] = e
        else:
            chunks.append([s, e])
        for w in range(beg >> 14, (end - 1 >> 14) + 1):
            c["win"][w] = min(c["win"].get(w, s), s)
    assert at == len(stream)
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for c in contigs:
        if c is None:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(c["bins"]) + 1))
        for b in sorted(c["bins"]):
            out.append(struct.pack("<Ii", b, len(c["bins"][b])) + b"".join(struct.pack("<QQ", *ch) for ch in c["bins"][b]))
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, c["first"], c["last"], c["n"][0], c["n"][1]))
        n_intv = max(c["win"]) + 1
        io, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            nxt = c["win"].get(w, nxt)
            io[w] = nxt
        out.append(struct.pack("<i%dQ" % n_intv, n_intv, *io))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


# ---- (b) a reader that uses an index
@functools.lru_cache(maxsize=4)
def parse(bai):
    """-> ([(bins {bin: [(beg, end)]}, ioffset list)] per contig, n_no_coor)"""
    assert bai[:4] == b"BAI\1"
    n_ref, at = struct.unpack_from("<i", bai, 4)[0], 8
    contigs = []
    for _ in range(n_ref):
        n_bin, at = struct.unpack_from("<i", bai, at)[0], at + 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            bins[b] = [struct.unpack_from("<QQ", bai, at + 8 + 16 * k) for k in range(n_chunk)]
            at += 8 + 16 * n_chunk
        n_intv = struct.unpack_from("<i", bai, at)[0]
        contigs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, bai, at + 4))))
        at += 4 + 8 * n_intv
    n_no_coor = struct.unpack_from("<Q", bai, at)[0]
    assert at + 8 == len(bai)
    return contigs, n_no_coor


class _Reader:
    """reads the inflated stream from a virtual offset on, member by member"""

    def __init__(self, bgzf, base_coffset, voff):
        self.bgzf, self.base = bgzf, base_coffset
        self.coff, self.uoff = (voff >> 16) - base_coffset, voff & 0xFFFF
        self._load()

    def _load(self):
        self.data, self.bsize = b"", 0
        if self.coff < len(self.bgzf):
            self.bsize = struct.unpack_from("<H", self.bgzf, self.coff + 16)[0] + 1
            self.data = zlib.decompress(self.bgzf[self.coff + 18:self.coff + self.bsize - 8], -15)

    def _settle(self):  # a position at the end of a full member is the next member's first
        if self.uoff == PAYLOAD and self.uoff == len(self.data):
            self.coff, self.uoff = self.coff + self.bsize, 0
            self._load()

    def tell(self):
        self._settle()
        return (self.base + self.coff) << 16 | self.uoff

    def read(self, n):
        out = b""
        while len(out) < n:
            self._settle()
            take = self.data[self.uoff:self.uoff + n - len(out)]
            assert take, "read past the end of the stream"
            out += take
            self.uoff += len(take)
        return out


def query(bai, bgzf, base_coffset, refid, beg, end):
    """the sorted virtual offsets of the records of contig refid that overlap [beg, end), found through the index alone"""
    contigs, _ = parse(bai)
    bins, ioffset = contigs[refid]
    if beg >> 14 >= len(ioffset):
        return []
    min_off = ioffset[beg >> 14]
    chunks = sorted(ch for b in reg2bins(beg, end) if b != PSEUDO_BIN for ch in bins.get(b, ()) if ch[1] > min_off)
    found = set()
    for c_beg, c_end in chunks:
        r = _Reader(bgzf, base_coffset, c_beg)
        while r.tell() < c_end:
            s = r.tell()
            head = r.read(4)
            rec = head + r.read(struct.unpack("<I", head)[0])
            _, rid, rbeg, rend, _ = record_fields(rec, 0)
            if rid == refid and rbeg < end and rend > beg:
                found.add(s)
    return sorted(found)


def brute_force(bgzf, base_coffset, refid, beg, end):
    """the same by a scan over every record of the stream"""
    mem, total = members(bgzf)
    coff = [p for p, _ in mem] + [total]
    stream = b"".join(d for _, d in mem)
    out, at = [], 0
    while at < len(stream):
        size, rid, rbeg, rend, _ = record_fields(stream, at)
        if rid == refid and rbeg < end and rend > beg:
            out.append((base_coffset + coff[at // PAYLOAD]) << 16 | at % PAYLOAD)
        at += size
    return out
