"""BQSR known sites at every seam of the device's index arithmetic: a second restatement of the reference's rule and the read sets that
walk the seams.

The rule: a base inside a known-site interval is left out of the recalibration tables - calculateSkipSlice (filters/bqsr.go:389-414) over
intervals.Intersect (intervals/intervals.go:166-173) and getReadCoordinateForReferenceCoordinate (filters/utils.go:267-349), on the copy of
the read that hardClipSoftClippedBases (utils.go:506-534) left.  The restatement below is written from that Go source, quirks included:
  !ok or fs < 0 -> 0;  !ok or fe > n - 1 -> n - 1;  a site that ends on the first base of a D gives the read coordinate of the base in
  front of it, one inside the D too;  a goal reached at the end of the LAST element fails;  a read coordinate of -1 (a leading D) fails;
  read coordinate 0 of a read that starts with an insertion is the first base behind it (the `left` rule).
It covers unpaired reads and paired reads that need no adaptor clip (needs_adaptor_clip says which), and returns the skip mask of the
clipped copy together with the index of its first base in the read.

On the device the rule is five pieces of index arithmetic (bqsr.hip, bqsr_prologue.hip, count3.hip):
  k_ref_mark_sites   bit 2 of the nibble of every site base of the packed reference, one word of WORD = 8 bases at a time
  k_site_index       per BUCKET = 64 bases the first site whose End is >= 64 b
  set / clear_skip_bits   words of SKIPW = 32 bits that neighbouring reads share, bit origin QUAL offset (+ clip)
  rec_simple         which reads take their bits from the reference window: POS-1-aoff >= REC_LO, POS-1-aoff+l_seq <= LN + REC_HI,
                     len <= REC_MAXLEN
  three prologues (fast, plain, general) x two forms (descriptors, records)

Every read matches the reference except for a few planted mismatches, has qualities >= 6 and no N, and is forward unless it is a
reverse twin.  A family of reads has its own read group (covariate), and the one quality of a read is 6 + (its probe index mod nq): a
table cell that differs decodes to (family, probe class, base index) - Case.decode.

Shared by tests/test_bq_sites_cpu.py (restatement against the oracle, coverage: no GPU) and tests/test_gpu_bq_sites.py (device against
the oracle)."""
import bisect
import functools

import numpy as np

import oracle as orc
from elprep_amd.batch import Batch, Header

WORD, BUCKET, SKIPW = 8, 64, 32                  # read back from the kernels by tests/test_bq_sites_cpu.py
REC_LO, REC_HI, REC_MAXLEN = 16, 32, 1022
REF_LDS = 256

READ_OPS, REF_OPS = "MIS=X", "MDN=X"
LISTS = ("A", "B", "C", "0")                     # site lists of a case: its own, sites elsewhere, A one base further, none


# ------------------------------------------------------------------------------------------------------------ the restatement
def parse_cigar(s):
    out, num = [], ""
    for ch in s:
        if ch.isdigit():
            num += ch
        else:
            out.append((ch, int(num)))
            num = ""
    return out


def read_length(cig):
    return sum(ln for op, ln in cig if op in READ_OPS)


def reference_length(cig):
    return sum(ln for op, ln in cig if op in REF_OPS)


def _hard_soft_offset(cig):
    """calculateHardSoftOffset, utils.go:351-371"""
    size, i = 0, 0
    while i < len(cig) and cig[i][0] == "H":
        size += cig[i][1]
        i += 1
    while i < len(cig) and cig[i][0] == "S":
        size += cig[i][1]
        i += 1
    return size


def _alignment_shift(op, ln, n):
    """calculateHardClippingAlignmentShift, utils.go:377-386: (operation, ITS length, the length asked about)"""
    if op == "I":
        return -n
    if op in "DN":
        return ln
    return 0


def _clean_hard_clipped(cig):
    """cleanHardClippedCigar, utils.go:473-504"""
    total, i = 0, 0
    while i < len(cig) and cig[i][0] in "HDN":
        total += cig[i][1]
        i += 1
    if i > 0:
        cig = [("H", total)] + cig[i:]
    total, i = 0, len(cig) - 1
    while i >= 0 and cig[i][0] in "HDN":
        total += cig[i][1]
        i -= 1
    if i < len(cig) - 1:
        cig = cig[:i + 1] + [("H", total)]
    return cig


def _hard_clip_cigar(cig, start, stop):
    """hardClipCigar, utils.go:407-471"""
    index, total, shift_sum, new = 0, stop - start + 1, 0, []
    if start == 0:
        k = 0
        for k, (op, ln) in enumerate(cig):  # (Go's range leaves the index on the last element when nothing breaks)
            if op != "H":
                break
            total += ln
        while index <= stop and k < len(cig):
            op, ln = cig[k]
            shift = ln if op in READ_OPS else 0
            if index + shift == stop + 1:
                shift_sum += _alignment_shift(op, ln, ln)
                new.append(("H", total + shift_sum))
            elif index + shift > stop + 1:
                shift_sum += _alignment_shift(op, ln, stop - index + 1)
                new += [("H", total + shift_sum), (op, ln - (stop - index + 1))]
            index += shift
            shift_sum += _alignment_shift(op, ln, shift)
            k += 1
        new += cig[k:]
    else:
        k = 0
        while index < start and k < len(cig):
            op, ln = cig[k]
            shift = ln if op in READ_OPS else 0
            if index + shift < start:
                new.append((op, ln))
            else:
                after = start - index
                shift_sum += _alignment_shift(op, ln, ln - (start - index))
                if op == "H":
                    total += after
                else:
                    new.append((op, after))
            index += shift
            k += 1
        while k < len(cig):
            op, ln = cig[k]
            shift_sum += _alignment_shift(op, ln, ln)
            if op == "H":
                total += ln
            k += 1
        new.append(("H", total + shift_sum))
    return _clean_hard_clipped(new)


def _hard_clip(pos, cig, n, lo, start, stop):
    """hardClip, utils.go:388-405 -> (POS, CIGAR, bases left, index of the first base left in the read as staged)"""
    new = _hard_clip_cigar(cig, start, stop)
    if start == 0:
        pos += _hard_soft_offset(new) - _hard_soft_offset(cig)
        lo += stop + 1
    return pos, new, n - (stop - start + 1), lo


def hard_clip_soft_clipped(pos, cig):
    """hardClipSoftClippedBases, utils.go:506-534 -> (POS, CIGAR, bases left, index of the first base left)"""
    n = read_length(cig)
    read_index, cut_left, cut_right, right_tail = 0, -1, -1, False
    for op, ln in cig:
        if op == "S":
            if right_tail:
                cut_right = read_index
            else:
                cut_left = read_index + ln - 1
        elif op != "H":
            right_tail = True
        read_index += ln if op in READ_OPS else 0
    lo = 0
    if cut_right >= 0:
        pos, cig, n, lo = _hard_clip(pos, cig, n, lo, cut_right, n - 1)
    if cut_left >= 0:
        pos, cig, n, lo = _hard_clip(pos, cig, n, lo, 0, cut_left)
    return pos, cig, n, lo


def soft_start(pos, cig):
    """utils.go:224-234"""
    for op, ln in cig:
        if op == "S":
            pos -= ln
        elif op != "H":
            break
    return pos


def soft_end(pos, cig):
    """utils.go:236-248; aln.End() = POS + reference length - 1"""
    end = pos + reference_length(cig) - 1
    soft = end
    for op, ln in reversed(cig):
        if op == "S":
            soft += ln
        elif op != "H":
            return soft
    return end


def intersect(sites, start, end):
    """intervals.Intersect: sites (sorted, flattened) with End >= start and Start <= end"""
    lo = bisect.bisect_left([e for _, e in sites], start)
    hi = bisect.bisect_right([s for s, _ in sites], end)
    return sites[lo:hi]


def _compute_read_coord(cig, sstart, ref_index):
    """computeReadCoordinateForReferenceCoordinate, utils.go:267-326"""
    goal = ref_index - sstart
    if goal < 0:
        return -1, False
    read_bases = ref_bases = index = 0
    inside = before = either = False
    while ref_bases != goal and index < len(cig):
        op, ln = cig[index]
        index += 1
        shift = 0
        if op in REF_OPS or op == "S":
            shift = ln if ref_bases + ln < goal else goal - ref_bases
            ref_bases += shift
        consumes = 1 if op in READ_OPS else 0
        if ref_bases != goal:
            read_bases += consumes * ln
        else:
            if shift >= ln and index == len(cig):
                return -1, False
            if shift < ln:
                inside = op in "DN"
            else:
                nxt = cig[index]
                index += 1
                if nxt[0] == "I":
                    read_bases += nxt[1]
                    if index == len(cig):
                        return -1, False
                    nxt = cig[index]
                    index += 1
                before = nxt[0] in "DN"
            either = before or inside
            if not either:
                read_bases += consumes * shift
            elif before:
                read_bases += consumes * (shift - 1)
            else:
                read_bases -= 1
    if ref_bases != goal:
        return -1, False
    return read_bases, either


def read_coordinate(cig, sstart, ref_index, right=False):
    """getReadCoordinateForReferenceCoordinate, utils.go:335-349 -> (read coordinate, ok)"""
    rb, either = _compute_read_coord(cig, sstart, ref_index)
    if rb == -1:
        return -1, False
    if right and either:
        rb += 1
    if not right and rb == 0:
        for op, ln in cig:  # readStartsWithInsertion, bqsr.go:287-299
            if op == "I":
                rb = min(ln, read_length(cig) - 1)
                break
            if op not in "HS":
                break
    return rb, True


def needs_adaptor_clip(flag, pos, cig, next_refid, pnext, tlen):
    """hardClipAdaptorSequence would clip (utils.go:148-180, 214-222): such a read is outside this restatement"""
    rev, nrev = bool(flag & 0x10), bool(flag & 0x20)
    if not (tlen != 0 and (flag & 0x1) and not (flag & 0x8) and next_refid >= 0 and pnext != 0 and rev != nrev):
        return False
    end = pos + reference_length(cig) - 1
    if rev:
        if not end > pnext:
            return False
        boundary = pnext - 1
    else:
        if not pos <= pnext + tlen:
            return False
        boundary = pos + abs(tlen)
    return pos <= boundary <= end


def skip_mask(pos, cig, sites):
    """calculateSkipSlice on the read as BaseRecalibrator.Recalibrate hands it over -> (mask of the clipped copy, index of its first base in
    the read).  cig: [(operation, length)], sites: [(Start, End)] sorted and flattened."""
    pos, cig, n, lo = hard_clip_soft_clipped(pos, cig)
    mask = np.zeros(n, bool)
    ss, se = soft_start(pos, cig), soft_end(pos, cig)
    for s, e in intersect(sites, ss, se):
        fs, ok = read_coordinate(cig, ss, s)
        if not ok or fs < 0:
            fs = 0
        fe, ok = read_coordinate(cig, ss, e)
        if not ok or fe > n - 1:
            fe = n - 1
        mask[fs:fe + 1] = True
    return mask, lo


# ------------------------------------------------------------------------------------------------------------ read sets
_NIB = np.array([1, 2, 4, 8], np.uint8)          # A C G T in BAM's nibbles
_CODE = np.zeros(256, np.uint8)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k
_OPS = "MIDNSHP=X"


def _reference(seed, n):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), n)


class Case:
    """One staged read set: header, batch, reference, the site lists A / B / C / 0, per read its family (= read group = covariate), probe
    index and parsed CIGAR.  What the oracle makes of it is computed once per list and shared (nobody writes to it)."""

    def __init__(self, name, ref_len, refs, sites, families, reads, max_cycle, nq):
        self.name, self.refs, self.sites, self.families, self.max_cycle, self.nq = name, refs, sites, list(families), max_cycle, nq
        self.h = Header.from_read_groups(["c%d" % k for k in range(len(ref_len))], list(ref_len),
                                         [{"ID": f, "LB": "lib", "PU": f} for f in families])
        n = len(reads)
        self.cig = [parse_cigar(r["cigar"]) for r in reads]
        self.fam = np.array([r["fam"] for r in reads], np.int64)
        self.probe = np.array([r["probe"] for r in reads], np.int64)
        lens = np.array([read_length(c) for c in self.cig], np.int64)
        qv = (6 + self.probe % nq).astype(np.uint8)
        qual_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        seq_off = np.concatenate([[0], np.cumsum((lens + 1) // 2)]).astype(np.uint64)
        seq4 = np.zeros(int(seq_off[-1]), np.uint8)
        cigs = []
        for i, (r, cig) in enumerate(zip(reads, self.cig)):
            codes = self._bases(refs[r["refid"]], r["pos"], cig, r["probe"])
            nib = _NIB[codes]
            if nib.size & 1:
                nib = np.append(nib, np.uint8(0))
            seq4[int(seq_off[i]):int(seq_off[i + 1])] = (nib[0::2] << 4) | nib[1::2]
            cigs.append(np.array([(ln << 4) | _OPS.index(op) for op, ln in cig], np.uint32))
        cigar_off = np.concatenate([[0], np.cumsum([c.size for c in cigs])]).astype(np.uint64)
        col = lambda k, d, dt: np.array([r.get(k, d) for r in reads], dt)
        self.b = Batch(refid=col("refid", 0, np.int32), pos=col("pos", 0, np.int32), next_refid=col("next_refid", -1, np.int32),
                       pnext=col("pnext", 0, np.int32), tlen=col("tlen", 0, np.int32), flag=col("flag", 0, np.uint16), mapq=np.full(n, 60, np.uint8),
                       rgid=self.fam.astype(np.uint16), has_sr=np.zeros(n, np.uint8), l_seq=lens.astype(np.uint32),
                       qname_off=np.arange(n + 1, dtype=np.uint64), qname=np.full(n, ord("r"), np.uint8), cigar_off=cigar_off,
                       cigar=np.concatenate(cigs), seq_off=seq_off, seq4=seq4, qual_off=qual_off, qual=np.repeat(qv, lens))
        self._exp = {}

    @staticmethod
    def _bases(ref, pos, cig, probe):
        """the read's bases as codes 0..3: the reference along M / = / X (A behind the contig's end), anything in I and S, and - every fifth
        probe - one planted mismatch"""
        out, j = [], pos - 1
        for op, ln in cig:
            if op in "M=X":
                idx = np.arange(j, j + ln)
                out.append(np.where(idx < ref.size, _CODE[ref[np.minimum(idx, ref.size - 1)]], 0).astype(np.uint8))
                j += ln
            elif op in "IS":
                out.append(((np.arange(ln) + probe) % 4).astype(np.uint8))
            elif op in "DN":
                j += ln
        codes = np.concatenate(out)
        if probe % 5 == 0:
            m = (probe * 7) % codes.size
            codes[m] = (codes[m] + 1 + probe % 3) % 4
        return codes

    @property
    def uniform(self):
        return len(set(self.b.l_seq.tolist())) == 1

    def sites_of(self, which):
        return [np.asarray(s, np.int32).reshape(-1, 2) for s in self.sites[which]]

    def expected(self, which="A"):
        """-> the oracle's (quality, cycle, context) tables under the site list `which`"""
        if which not in self._exp:
            t = orc.bqsr_gather(self.b, self.h, orc.BqsrRef(self.refs, self.sites_of(which)), None, self.max_cycle)
            for a in t:
                a.setflags(write=False)
            self._exp[which] = t
        return self._exp[which]

    def decode(self, cov, q, cyc):
        """a cell (covariate, quality, index into the cycle axis) -> whose it is"""
        c = int(cyc) - self.max_cycle
        return "case %s, family %s, probes = %d mod %d, cycle %d (base %d of a forward read, base len - %d of a reverse twin)" % (
            self.name, self.families[int(cov)], int(q) - 6, self.nq, c, c - 1, c)

    def simple(self, i):
        """-> (aoff, len) if read i's CIGAR is [H] [S] <match> [S] [H] (the fast prologue's reads), else None"""
        ops = [x for x in self.cig[i] if x[0] != "H"]
        if any(op == "H" for op, _ in self.cig[i][1:-1]):
            return None
        aoff = ops[0][1] if ops and ops[0][0] == "S" else 0
        core = ops[1:] if aoff else ops
        if core and core[-1][0] == "S":
            core = core[:-1]
        if len(core) != 1 or core[0][0] not in "M=X":
            return None
        return aoff, core[0][1]

    def rec_simple(self, i):
        """pf_record's rec_simple (bqsr_prologue.hip): the read's known-site bits come with its reference window, not the skip column"""
        s = self.simple(i)
        if s is None:
            return False
        e0 = int(self.b.pos[i]) - 1 - s[0]
        return s[1] <= REC_MAXLEN and e0 >= REC_LO and e0 + int(self.b.l_seq[i]) <= int(self.h.ref_len[self.b.refid[i]]) + REC_HI


def _shifted(sites, ref_len):
    """list C: every site one base further (the last one stays where it would leave the contig)"""
    return [[(s + 1, e + 1) if e + 1 <= ln else (s, e) for s, e in per] for per, ln in zip(sites, ref_len)]


def _lists(a, b, ref_len):
    return {"A": a, "B": b, "C": _shifted(a, ref_len), "0": [[] for _ in a]}


# ---- ruler
@functools.lru_cache(maxsize=None)
def ruler_layout():
    """-> (contig lengths, list A, list B, (start, end) of the long site).  Contig 0 carries a site for every start phase a and end phase b
    of the 8-base word over 1, 2 and 3 words, sites that end / start / lie at 64 b - 1, 64 b, 64 b + 1 for three buckets each, a
    300-base site over five bucket seams, [1, 1] and [LN, LN]; its length is 64 k - 1.  Contig 1 has no sites, contig 2 (64 k) one that
    ends past LN, contig 3 is 64 k + 1 long.  Neighbouring sites are at least 2 bases apart (Flatten merges at Start <= End)."""
    a0 = [(1, 1)]
    combos = [(nw, a, b) for nw in (1, 2, 3) for a in range(WORD) for b in range(WORD) if nw > 1 or b >= a]
    w = 3
    for k, (nw, a, b) in enumerate(combos):
        a0.append((WORD * w + a + 1, WORD * (w + nw - 1) + b + 1))
        nxt = combos[k + 1][1] if k + 1 < len(combos) else 0
        w += nw if WORD - b + nxt >= 2 else nw + 1
    bk = WORD * w // BUCKET + 2
    for form in ("end", "start", "single"):
        for _ in range(3):
            for d in (-1, 0, 1):
                x = BUCKET * bk + d
                a0.append({"end": (x - 4, x), "start": (x, x + 4), "single": (x, x)}[form])
                bk += 1
    long_site = (BUCKET * (bk + 1) + 20, BUCKET * (bk + 1) + 319)
    a0.append(long_site)
    pad = BUCKET * (long_site[1] // BUCKET + 2)
    ln0 = pad + 5 * BUCKET - 1
    a0.append((ln0, ln0))
    ref_len = (ln0, 150, 5 * BUCKET, 5 * BUCKET + 1)
    a = [a0, [], [(1, 1), (60, 70), (ref_len[2] - 2, ref_len[2] + 40)], [(3, 5), (BUCKET, BUCKET), (ref_len[3], ref_len[3])]]
    # B: nothing near the start of contig 0, sites in its empty tail, a list where there was none and none where there was one
    b0 = [s for s in a0 if s[0] > 160] [:-1] + [(pad + 10, pad + 12), (pad + 70, pad + 70), (pad + 130, pad + 140), (ln0, ln0)]
    b = [b0, [(10, 12), (100, 149)], [], [(200, 210), (ref_len[3], ref_len[3])]]
    return ref_len, a, b, long_site


def _ruler_refs(ref_len):
    return [_reference(100 + k, ln) for k, ln in enumerate(ref_len)]


def _variants(p, ln, L):
    """which positions also get the 3S... / ...4S reads: a third each, and everything near the contig's ends"""
    edge = p <= 48 or p > ln - (L + 40)
    return edge or p % 3 == 0, edge or p % 3 == 1


@functools.lru_cache(maxsize=None)
def ruler(L):
    """one read of L bases at every position 1..LN of every contig (those near the end hang over it), some also as 3S<L-3>M (aoff moves
    POS-1-aoff across 15, 16, 17 and below 0) and <L-4>M4S.  L = 0: the same reads with ragged lengths 1..70 (the descriptor form)."""
    ref_len, a, b, _ = ruler_layout()
    reads = []
    for r, ln in enumerate(ref_len):
        for p in range(1, ln + 1):
            l = L if L else 1 + (p * 37 + r * 11) % 70
            reads.append(dict(refid=r, pos=p, cigar="%dM" % l, fam=0, probe=p))
            v3, v4 = _variants(p, ln, l)
            if v3 and l >= 8:
                reads.append(dict(refid=r, pos=p, cigar="3S%dM" % (l - 3), fam=1, probe=p))
            if v4 and l >= 8:
                reads.append(dict(refid=r, pos=p, cigar="%dM4S" % (l - 4), fam=2, probe=p))
    return Case("ruler%d" % L if L else "ruler_ragged", ref_len, _ruler_refs(ref_len), _lists(a, b, ref_len), ("plain", "3S", "4S"), reads, 128, 16)


@functools.lru_cache(maxsize=None)
def ruler_long(L):
    """a few dozen reads of 1022 (the longest the records describe) / 1023 bases over the long site, at the start of the contig and at the
    three overhangs around its end + REC_HI"""
    ref_len, a, b, long_site = ruler_layout()
    ps = [1, REC_LO, REC_LO + 1, REC_LO + 2] + [long_site[0] - 1000 + 25 * k for k in range(40)] + [ref_len[0] + REC_HI - L + d for d in (0, 1, 2)]
    reads = [dict(refid=0, pos=p, cigar="%dM" % L, fam=0, probe=k) for k, p in enumerate(ps)]
    return Case("ruler_long%d" % L, ref_len, _ruler_refs(ref_len), _lists(a, b, ref_len), ("long",), reads, 1100, 4)


@functools.lru_cache(maxsize=None)
def many_contigs():
    """257 contigs (REF_LDS = 256: the per-contig facts come from memory, not LDS), the last one with sites"""
    n = REF_LDS + 1
    ref_len = tuple(90 + k % 7 for k in range(n))
    a = [[(5, 6), (30, 40)] if k % 50 == 0 else [] for k in range(n)]
    a[n - 1] = [(1, 1), (20, 22), (ref_len[n - 1], ref_len[n - 1])]
    b = [[(50, 52)] if k % 50 == 1 else [] for k in range(n)]
    reads = [dict(refid=k, pos=p, cigar="37M", fam=0, probe=5 * k + j) for k in range(n)
             for j, p in enumerate((1, 20, 40, ref_len[k] - 10, ref_len[k] - 2))]
    return Case("many_contigs", ref_len, [_reference(300 + k, ln) for k, ln in enumerate(ref_len)], _lists(a, b, ref_len), ("many",), reads, 128, 16)


# ---- indels: one read and one site per probe
SHAPES = ("20M3D20M", "20M3I17M", "5S15M2D15M5S", "3I37M", "37M3I", "3D40M", "8M1I8M2D8M1I8M1D6M", "15M2I3D20M", "2H36M2H", "60M2P40M", "98M1D3M")
WIDTHS = (1, 2, 3, 6)
WORDS_SHAPE = "98M1D3M"                          # the skip column's word seams: runs of these lengths from these bit phases
WORDS_WIDTHS, WORDS_PHASES = (1, 2, 3, 4, 30, 31, 32, 64), (0, 1, 30, 31)
INDEL_LENGTHS = (40, 37, 36, 100, 101)


def _slot(L):
    return 128 if L <= 47 else 256


@functools.lru_cache(maxsize=None)
def _indel_layout():
    """-> (contig lengths, list A, list B, per read length the reads).  One contig per read length; probe k of a contig lives in slot k (128
    bases, 256 for the long shapes): the read starts at base 13 of the slot, the site is [s, s + w - 1] for w in 1, 2, 3, 6 and s from
    POS - 8 to End + 8, so no read sees another probe's site and nothing flattens together.  Every second probe has a reverse twin."""
    ref_len, a, b, reads = [], [], [], {}
    for c, L in enumerate(INDEL_LENGTHS):
        sa, sb, rs, k = [], [], [], 0
        for fam, shape in enumerate(SHAPES):
            cig = parse_cigar(shape)
            if read_length(cig) != L:
                continue
            span, j = reference_length(cig), 0
            if shape == WORDS_SHAPE:
                probes = [(w, ph) for w in WORDS_WIDTHS for ph in WORDS_PHASES]
            else:
                probes = [(w, d) for w in WIDTHS for d in range(-8, span + 8)]
            for w, d in probes:
                pos = _slot(L) * k + 13
                if shape == WORDS_SHAPE:  # (no twins in this family: read k's QUAL starts at 101 k)
                    d = (d - len(rs) * L) % SKIPW
                sa.append((pos + d, pos + d + w - 1))
                if k % 3 == 0:
                    sb.append((_slot(L) * k + (100 if L <= 47 else 200), _slot(L) * k + (101 if L <= 47 else 203)))
                rs.append(dict(refid=c, pos=pos, cigar=shape, fam=fam, probe=j))
                if j % 2 and shape != WORDS_SHAPE:
                    rs.append(dict(refid=c, pos=pos, cigar=shape, fam=fam, probe=j, flag=0x10))
                k += 1
                j += 1
        ref_len.append(_slot(L) * k + BUCKET)
        a.append(sa)
        b.append(sb)
        reads[L] = rs
    return tuple(ref_len), a, b, reads


@functools.lru_cache(maxsize=None)
def indels(L):
    """the probes of the shapes with reads of L bases: a one-length set"""
    ref_len, a, b, reads = _indel_layout()
    return Case("indels%d" % L, ref_len, [_reference(500 + k, ln) for k, ln in enumerate(ref_len)], _lists(a, b, ref_len), SHAPES, reads[L], 128, 8)


# ---- adaptor: FR pairs with a short insert (oracle only: the restatement does not clip)
ADAPTOR_SHAPES = ("50M", "4S46M", "25M2D25M")


@functools.lru_cache(maxsize=None)
def adaptor():
    """48 reads of pairs whose insert is shorter than the read: forward reads lose their right tail from POS + |TLEN| on, reverse reads their
    left tail up to PNEXT - 1 (a.off != 0), and a site of 1..4 bases straddles the clip point or lies next to it"""
    n, L = 48, 50
    ref_len = (256 * n + BUCKET,)
    a, b, reads = [], [], []
    for k in range(n):
        shape = ADAPTOR_SHAPES[k % 3]
        pos, ins = 256 * k + 60, 30 + (k * 7) % 16
        if k % 2 == 0:  # forward, mate reverse: boundary = POS + TLEN
            rec = dict(flag=0x1 | 0x40 | 0x20, pnext=pos + ins - L, tlen=ins, fam=0)
            clip = pos + ins
        else:           # reverse, mate forward: boundary = PNEXT - 1
            rec = dict(flag=0x1 | 0x40 | 0x10, pnext=pos + L - ins, tlen=-ins, fam=1)
            clip = rec["pnext"] - 1
        s = clip + (k % 5) - 2
        a.append((s, s + k % 4))
        b.append((256 * k + 200, 256 * k + 201))
        reads.append(dict(refid=0, pos=pos, cigar=shape, next_refid=0, probe=k, **rec))
    return Case("adaptor", ref_len, [_reference(700, ref_len[0])], _lists([a], [b], ref_len), ("forward", "reverse"), reads, 128, 8)


CASES = {
    "ruler37": functools.partial(ruler, 37), "ruler101": functools.partial(ruler, 101), "ruler_ragged": functools.partial(ruler, 0),
    "ruler_long1022": functools.partial(ruler_long, 1022), "ruler_long1023": functools.partial(ruler_long, 1023), "many_contigs": many_contigs,
    "indels40": functools.partial(indels, 40), "indels37": functools.partial(indels, 37), "indels36": functools.partial(indels, 36),
    "indels100": functools.partial(indels, 100), "indels101": functools.partial(indels, 101), "adaptor": adaptor,
}
RECORD_CASES = tuple(k for k in CASES if k not in ("ruler_ragged", "ruler_long1023"))  # one length, at most REC_MAXLEN bases: count3.hip takes them
