"""GPU parity tests (-m gpu) on every CIGAR operation: =, X, P, N (introns up to 200 kb), zero-length M / I / D / P, leading and trailing
I or D, I next to D - next to the M / I / D / S / H of the other generators.  The device branches on these letters in the BQSR prologue
routing (fast: [H][S](M|=|X)[S][H]; plain: two to five ops of M / = / X / I / D; general: the rest, bqsr_prologue.hip), the reference pieces,
the read coordinate of a known site next to a D, the unclipped 5' position of a reverse read (an N counts), the filter predicates,
CleanSam and the BAM emitter's bin.  Every output is compared bit for bit with the CPU oracle."""
import functools

import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Header, batch_from_records
from elprep_amd.engine import ElpError, Engine
from tests.test_gpu_ragged import _check_gather_apply
from tests.test_gpu_round3 import _oracle_path, _same, _whole_path
from tests.test_oracle_kat import _READ, _REF, _ClipPanic, _c_clip, _draw_all_ops

pytestmark = pytest.mark.gpu

# hand shapes, written for 150-base reads (_fit moves the last aligned run to other lengths), each with what it is there for
HAND = [
    ("150=", "fast prologue, = only"),
    ("75=1X74=", "adjacent = / X runs with one offset: plain prologue, ONE merged reference piece"),
    ("2H4S140X6S1H", "fast prologue with an X run between clips"),
    ("60M2P90M", "P inside a match: general prologue, still one piece"),
    ("60=0I90=", "zero-length I: plain prologue, no piece opened for it"),
    ("75M0D75M", "zero-length D: plain prologue, one piece"),
    ("0M150M", "zero-length leading M: plain prologue"),
    ("3I147M", "leading insertion (the 'left' rule's first-insertion case)"),
    ("147M3I", "trailing insertion"),
    ("3D150M", "leading deletion"),
    ("70M2I3D78M", "I next to D: read coordinate of a site that ends before the D"),
    ("70M3D2I78M", "D next to I"),
    ("50M100000N100M", "100 kb intron: gather drops it, apply rewrites it, the unclipped end of a reverse read moves by 100 kb"),
    ("30M500N40M200N80M", "two introns"),
    ("30S20M300N100M", "soft clip and intron"),
    ("25=1X25=1X25=1X25=1X25=1X20=", "eleven = / X ops: general prologue with an = / X CIGAR"),
    ("40M1P0I30=2X78M", "P, zero-length I and = / X runs in one general CIGAR"),
]
# reads whose N spans cross 2^14 / 2^17 boundaries (reg2bin level 4 / 3 instead of 5): (contig, pos, CIGAR)
BIN_SHAPES = [(0, (1 << 14) - 60, "50M20000N100M"), (0, 3 * (1 << 14) - 20, "120M900N30M"), (0, (1 << 17) - 70, "50M150000N100M"),
              (0, 5 * (1 << 17) - 40, "60M3000N90M")]
QUALS = [2, 5, 6, 12, 23, 37, 41]
REF_LEN = (2_500_000, 400_000)


def _ops(s):
    out, num = [], ""
    for ch in s:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    return out


def _cig(ops):
    return "".join("%d%s" % x for x in ops)


def _fit(ops, L):
    """ops with read length L: the last non-empty M / = / X run takes the difference; None if it cannot"""
    d = L - sum(l for l, o in ops if o in _READ)
    for k in range(len(ops) - 1, -1, -1):
        l, o = ops[k]
        if o in "M=X" and l > 0:
            if l + d < 1:
                return None
            return ops[:k] + [(l + d, o)] + ops[k + 1:]
    return None


def route(ops):
    """the prologue a read of this (staged) CIGAR takes, by the rule of k_bqsr_prologue_fast (bqsr_prologue.hip): 'fast', 'plain' or 'general'"""
    nop = len(ops)
    simple, k, mlen = 1 <= nop <= 5, 0, 0
    if simple and ops[0][1] == "H":
        k = 1
    if simple and k < nop and ops[k][1] == "S":
        k += 1
    if simple and k < nop and ops[k][1] in "M=X":
        mlen = ops[k][0]; k += 1
    else:
        simple = False
    if simple and k < nop and ops[k][1] == "S":
        k += 1
    if simple and k < nop and ops[k][1] == "H":
        k += 1
    if simple and k == nop and mlen != 0:
        return "fast"
    if 2 <= nop <= 5 and all(o in "M=XID" for _, o in ops):
        return "plain"
    return "general"


def _unclipped_5p(pos, flag, ops, count_n=True):
    """filters/mark-duplicates.go:90-108"""
    if flag & 0x10:
        end = pos - 1 + sum(l for l, o in ops if o in "MD=X" or (count_n and o == "N"))
        k = len(ops) - 1
        while k >= 0 and ops[k][1] in "SH":
            end += ops[k][0]; k -= 1
        return end
    k = 0
    while k < len(ops) and ops[k][1] in "SH":
        pos -= ops[k][0]; k += 1
    return pos


@functools.lru_cache(maxsize=4)
def _case(seed, length=0, n_random=2200, copies=10):
    """reads of `length` bases (0: ragged, 20..300) on two contigs of 2.5 Mb and 400 kb: _draw_all_ops CIGARs, the HAND and BIN_SHAPES
    shapes, pairs that are duplicates only through an N span; FR pairs with short inserts (adaptor clipping), reverse reads, low-quality
    tails, N bases, reads over the contig end.  Bases under = / X follow the reference or not, whatever the letter says.
    -> (batch, header, refs, sites, meta) with meta = {'dupN': [(A read 1, B read 1)], 'bin': [record indices]}"""
    rng = np.random.default_rng(seed)
    refs = []
    for L in REF_LEN:
        r = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)
        for _ in range(20):
            s = int(rng.integers(0, L - 40)); r[s:s + int(rng.integers(1, 30))] = ord("N")
            s = int(rng.integers(0, L - 40)); r[s:s + 25] = np.where(r[s:s + 25] != ord("N"), r[s:s + 25] | 0x20, r[s:s + 25])
        refs.append(r)
    sites = []
    for L in REF_LEN:
        st = rng.integers(1, L, L // 150)
        sites.append(orc.flatten(orc.sort_by_start(np.stack([st, st + rng.integers(0, 12, st.size)], axis=1).astype(np.int32))))
    rgs = [{"ID": "rg%d" % k, "LB": "lib%d" % (k % 2), "PU": "pu%d" % (k % 2)} for k in range(3)]
    h = Header.from_read_groups(["c0", "c1"], list(REF_LEN), rgs)
    recs = []

    def read_len():
        return length if length else int(rng.integers(20, 301))

    def seq_for(ops, r, pos):
        seq, j, ref = [], pos - 1, refs[r]
        for l, o in ops:
            if o in "M=X":
                for _ in range(l):
                    c = chr(ref[j]).upper() if 0 <= j < ref.size else "A"
                    if c not in "ACGT" or rng.random() < 0.12:
                        c = "ACGT"[int(rng.integers(0, 4))]
                    seq.append("N" if rng.random() < 0.01 else c)
                    j += 1
            elif o in "IS":
                seq += ["ACGT"[int(x)] for x in rng.integers(0, 4, l)]
            elif o in "DN":
                j += l
        return "".join(seq)

    def quals(L):
        q = rng.choice(QUALS, size=L).astype(np.uint8)
        if rng.random() < 0.3:
            q[:int(rng.integers(0, min(4, L) + 1))] = 2
        if rng.random() < 0.3:
            t = int(rng.integers(0, min(4, L) + 1))
            if t:
                q[-t:] = 2
        return q

    def add(ops, r=None, pos=None, pair=None, qname=None):
        span = sum(l for l, o in ops if o in _REF)
        RL = REF_LEN[r] if r is not None else 0
        if r is None:
            r = int(rng.integers(0, 2)) if span < REF_LEN[1] - 10 else 0
            RL = REF_LEN[r]
            if span >= RL - 2:
                return None
            pos = int(rng.integers(max(1, RL - span // 2), RL + 1)) if rng.random() < 0.03 else int(rng.integers(1, RL - span))
        L = sum(l for l, o in ops if o in _READ)
        rev = rng.random() < 0.5
        flag, pnext, tlen, nref = 0, 0, 0, -1
        if pair is not None:
            flag, pnext, tlen, nref = pair
        elif rng.random() < 0.7:
            flag, nref = 0x1 | (0x40 if rng.random() < 0.5 else 0x80), r
            if rng.random() < 0.45:  # FR with a short insert: adaptor clipping (filters/utils.go:149-180)
                ins = int(rng.integers(max(12, L // 2), L + 40))
                flag |= 0x10 if rev else 0x20
                pnext, tlen = (max(1, pos + span - ins), -ins) if rev else (pos + max(0, ins - 20), ins)
            else:
                flag |= (0x10 if rev else 0) | (0x20 if rng.random() < 0.5 else 0)
                pnext = int(rng.integers(1, RL))
        else:
            flag = 0x10 if rev else 0
        if pair is None and not any(o == "N" for _, o in ops):
            try:
                _c_clip(dict(ops=ops, L=L, pos=pos, flag=flag, pnext=pnext, tlen=tlen, next_refid=nref))
            except _ClipPanic:  # the reference panics on this geometry (test_clipping_panics_surface_as_errors): a single-end read instead
                flag, pnext, tlen, nref = flag & 0x10, 0, 0, -1
        if pair is None and rng.random() < 0.02:
            flag |= 0x800
        recs.append(dict(qname=qname or "r%06d" % len(recs), flag=flag, refid=r, pos=pos, mapq=int(rng.choice([60, 60, 60, 29, 0, 255])) if pair is None else 60,
                         cigar=_cig(ops), next_refid=nref, pnext=pnext, tlen=tlen, seq=seq_for(ops, r, pos), qual=quals(L), rgid=int(rng.integers(0, 3))))
        return len(recs) - 1

    while len(recs) < n_random:
        L = read_len()
        ops = _fit(_draw_all_ops(rng, m_hi=max(2, L // 3)), L)
        if ops is not None:
            add(ops)
    for s, _ in HAND:
        for _ in range(copies):
            ops = _fit(_ops(s), read_len())
            if ops is not None:
                add(ops)
    meta = {"dupN": [], "bin": []}
    for r, pos, s in BIN_SHAPES:
        ops = _fit(_ops(s), read_len())
        if ops is not None:
            meta["bin"].append(add(ops, r, pos))
    # pairs that are duplicates only through an N span: A = (fwd, rev with an intron), B = (fwd at the same place, rev without one)
    for k in range(6):
        L1, L2 = read_len(), read_len()
        a1, b1 = _fit([(150, "M")], L1), _fit([(150, "M")], L1)
        a2 = _fit([(40, "M"), (int(rng.integers(1000, 150_000)), "N"), (110, "M")], L2)
        b2 = _fit([(150, "M")], L2)
        if a2 is None:
            continue
        p1 = int(rng.integers(1, 800_000))
        p2 = p1 + int(rng.integers(0, 300))
        sa = sum(l for l, o in a2 if o in _REF)
        q2 = p2 + sa - sum(l for l, o in b2 if o in _REF)
        rg = int(rng.integers(0, 3))
        ia = add(a1, 0, p1, (0x1 | 0x2 | 0x20 | 0x40, p2, p2 + sa - p1, 0), "dA%d" % k)
        add(a2, 0, p2, (0x1 | 0x2 | 0x10 | 0x80, p1, -(p2 + sa - p1), 0), "dA%d" % k)
        ib = add(b1, 0, p1, (0x1 | 0x2 | 0x20 | 0x40, q2, p2 + sa - p1, 0), "dB%d" % k)
        add(b2, 0, q2, (0x1 | 0x2 | 0x10 | 0x80, p1, -(p2 + sa - p1), 0), "dB%d" % k)
        for i in (ia, ia + 1, ib, ib + 1):
            recs[i]["rgid"] = rg
        meta["dupN"].append((ia, ib))
    if not length:
        recs.append(dict(qname="un", flag=4, refid=-1, pos=0, mapq=0, cigar="*", seq="ACGTN", qual=[30, 2, 40, 7, 9], rgid=0))
    return batch_from_records(recs), h, refs, sites, meta


def _cigars(b):
    return [[(int(c) >> 4, "MIDNSHP=X"[int(c) & 15]) for c in b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])]] for i in range(b.n)]


def _check_coverage(b, h, refs, sites, meta):
    """the case reaches what it is written for: each prologue with = / X / P / zero-length ops among the reads the gather takes, an N read
    whose QUAL apply changes, a duplicate pair that exists only through an N span"""
    oflags = orc.mark_duplicates(b, h)
    cig = _cigars(b)
    cnt = {}
    for i in range(b.n):
        f, mq, r, p = int(oflags[i]), int(b.mapq[i]), int(b.refid[i]), int(b.pos[i])
        ops, L = cig[i], int(b.l_seq[i])
        if not (0 < mq < 255) or f & 0x704 or r < 0 or p <= 0 or p > REF_LEN[r] or L == 0 or any(o == "N" for _, o in ops):
            continue
        rt = route(ops)
        cnt[rt] = cnt.get(rt, 0) + 1
        for key, hit in (("=", any(o == "=" for _, o in ops)), ("X", any(o == "X" for _, o in ops)), ("P", any(o == "P" for _, o in ops)),
                         ("0", any(l == 0 for l, _ in ops))):
            if hit:
                cnt[rt + key] = cnt.get(rt + key, 0) + 1
    want = ["fast", "plain", "general", "fast=", "fastX", "plain=", "plainX", "plain0", "general=", "generalX", "generalP", "general0"]
    assert all(cnt.get(k, 0) > 0 for k in want), cnt
    oq, oc, ox = orc.bqsr_gather(b, h, orc.BqsrRef(refs, sites), oflags, 500)
    oqual = orc.BqsrFinal(oq, oc, ox, 500).apply(b, h, 0)
    n_reads = [i for i in range(b.n) if any(o == "N" for _, o in cig[i])]
    assert any((oqual[int(b.qual_off[i]):int(b.qual_off[i + 1])] != b.qual_of(i)).any() for i in n_reads), "no N read rewritten by apply"
    n_dup = 0
    for ia, ib in meta["dupN"]:
        ea, eb = _unclipped_5p(int(b.pos[ia + 1]), int(b.flag[ia + 1]), cig[ia + 1]), _unclipped_5p(int(b.pos[ib + 1]), int(b.flag[ib + 1]), cig[ib + 1])
        assert ea == eb and _unclipped_5p(int(b.pos[ia + 1]), int(b.flag[ia + 1]), cig[ia + 1], count_n=False) != eb
        n_dup += bool((oflags[ia] | oflags[ib]) & 0x400)
    assert n_dup > 0, "no pair is a duplicate through its N span"


# kernel choices: every value of every key at least once with the ragged set and with a one-length set (four settings x two sets)
TUNINGS = [dict(count_kernel=0, apply_kernel=0, score_kernel=0, mate_path=0),
           dict(count_kernel=1, apply_kernel=1, score_kernel=1, mate_path=2),
           dict(count_kernel=2, apply_kernel=3, score_kernel=0, mate_path=2),
           dict(count_kernel=3, apply_kernel=0, score_kernel=1, mate_path=2)]


@pytest.mark.parametrize("tune,length", [(t, 0) for t in range(len(TUNINGS))] + [(t, 150 if t % 2 == 0 else 151) for t in range(len(TUNINGS))])
def test_whole_path_on_every_cigar_op(monkeypatch, tune, length):
    """adapted unclipped positions and scores, flags, permutation, metrics counters and histograms, the three tables, every QUAL byte;
    one-length sets (150 or 151 bases) take count3 / apply3 and the apply_rec record"""
    b, h, refs, sites, meta = _case(1 if not length else length, length)
    if length:
        assert len(set(np.diff(b.qual_off).tolist())) == 1
    if tune == 0:
        _check_coverage(b, h, refs, sites, meta)
    monkeypatch.setenv("ELP_TUNE", ",".join("%s=%d" % kv for kv in TUNINGS[tune].items()))
    _check_gather_apply(b, h, refs, sites, chunks=2)
    e = Engine(h)
    e.stage(b)
    got = _whole_path(e, b, h, refs, sites)
    want = _oracle_path(b, h, refs, sites)
    _same(got, want)
    ctr, hist = e.dup_metrics(100, 8)
    _, octr, ohist = orc.dup_metrics(b, h, want[1], 100, 8)
    assert np.array_equal(ctr, octr) and np.array_equal(hist, ohist)
    e.close()


def _regions(rng):
    out = []
    for L in REF_LEN:
        s = np.sort(rng.integers(0, L - 3000, 300))
        out.append(orc.flatten(orc.sort_by_start(np.stack([s, s + rng.integers(1, 2000, s.size)], axis=1).astype(np.int32))))
    return out


@pytest.mark.parametrize("sel", [dict(remove_non_exact=True), dict(use_regions=True), dict(remove_non_exact=True, use_regions=True, min_mapq=1)])
def test_filter_predicates_on_every_cigar_op(sel):
    """remove_non_exact (anything but M and S) and the regions' alignment end (N, = and X consume the reference, P does not)"""
    from oracle import simple_filters as sf
    b, h, refs, sites, meta = _case(1, 0)
    sel = dict(sel)
    regions = _regions(np.random.default_rng(3)) if sel.pop("use_regions", False) else None
    keep = sf.keep_mask(b, regions=regions, **sel)
    assert 0 < keep.sum() < b.n
    e = Engine(h)
    e.stage(b)
    assert e.filter_records(regions=regions, **sel) == int((~keep).sum())
    assert e.n_sorted == int(keep.sum())
    kept = np.nonzero(keep)[0]
    kb = b.take(kept)
    oflags = orc.mark_duplicates(kb, h)
    flags = e.mark_duplicates(True)
    assert np.array_equal(flags[kept], oflags)
    operm = orc.sort_coordinate(kb, oflags)
    assert np.array_equal(e.sort_coordinate()[:e.n_sorted], kept[operm])
    for r in range(h.n_ref):
        e.set_reference(r, refs[r])
        e.set_known_sites(r, sites[r])
    oq, oc, ox = orc.bqsr_gather(kb, h, orc.BqsrRef(refs, sites), oflags, 500)
    qt, ct, xt = e.recalibrate(500)
    assert np.array_equal(qt, oq) and np.array_equal(ct, oc) and np.array_equal(xt, ox)
    e.close()


def test_clean_sam_on_every_cigar_op():
    """contigs cut so that reads end behind them through N / = / X / P: rewritten CIGARs (read back through the BAM encoder) and the flags
    and order downstream against the oracle's CleanSam restatement; a record where the reference panics ('Unexpected non-0 relative
    clipping position') is an error"""
    from oracle import simple_filters as sf
    b, h, refs, sites, meta = _case(1, 0)
    cut = np.array([1_600_000, 250_000], np.int32)
    cig = _cigars(b)
    take, panics = [], []
    for i in range(b.n):
        r, p = int(b.refid[i]), int(b.pos[i])
        if r < 0 or b.flag[i] & 0x4:
            take.append(i)
            continue
        if p > cut[r] - 20:
            continue
        end = p + sum(l for l, o in cig[i] if o in _REF) - 1
        if end > cut[r]:
            try:
                sf.clean_sam(b.take([i]), cut)
            except ValueError:
                panics.append(i)
                continue
        take.append(i)
    bb = b.take(np.asarray(take))
    h2 = Header(ref_len=cut, rg_lib=h.rg_lib, rg_cov=h.rg_cov, ref_names=h.ref_names, rg_ids=h.rg_ids, lib_names=h.lib_names, cov_names=h.cov_names)
    want, n_changed = sf.clean_sam(bb, cut)
    over = [cig[i] for i in take if b.refid[i] >= 0 and int(b.pos[i]) + sum(l for l, o in cig[i] if o in _REF) - 1 > cut[b.refid[i]]]
    assert n_changed == len(over) and all(any(any(o == x for _, o in c) for c in over) for x in "N=XP"), n_changed
    e = Engine(h2)
    e.set_read_group_ids(h2.rg_ids)
    e.stage_bam(orc.bam_encode(bb, h2.rg_ids))
    assert e.clean_sam() == n_changed
    flags = e.mark_duplicates(True)
    oflags = orc.mark_duplicates(want, h2)
    assert np.array_equal(flags, oflags)
    perm = e.sort_coordinate()
    operm = orc.sort_coordinate(want, oflags)
    assert np.array_equal(perm, operm)
    got = e.emit_sorted_bam().tobytes()
    assert got == orc.bam_encode(want, h2.rg_ids, order=operm[:orc.num_sorted(want)], flags=oflags, normalize_tags=True).tobytes()
    e.close()
    # softClipEndOfRead adds endPos to pos (utils.go:118): after 3M and 2= pos is 8, the D at clip position 6 is where the reference panics
    bad = batch_from_records([dict(qname="c", flag=0, refid=0, pos=int(cut[0]) - 6, mapq=60, cigar="3M2=1D50M", seq="A" * 55, qual=[30] * 55,
                                   rgid=0)] + [dict(qname="c%d" % k, flag=0, refid=0, pos=int(cut[0]) - 6, mapq=60, cigar="3M2=1X50M",
                                                    seq="A" * 56, qual=[30] * 56, rgid=0) for k in range(2)])
    with pytest.raises(ValueError):
        sf.clean_sam(bad, cut)
    for recs in (bad, b.take(np.asarray(panics[:1] + take[:50]))) if panics else (bad,):
        e = Engine(h2)
        e.stage(recs)
        with pytest.raises(ElpError, match="Unexpected non-0"):
            e.clean_sam()
        e.close()


def _bin_level(bin_):
    for lvl, first in ((5, 4681), (4, 585), (3, 73), (2, 9), (1, 1), (0, 0)):
        if bin_ >= first:
            return lvl


def test_emit_sorted_bam_and_stage_bam_on_every_cigar_op():
    """emit_sorted_bam byte-equal to the oracle's encoder on the sorted, marked, recalibrated records (reg2bin over N spans that cross
    2^14 and 2^17 boundaries), and the same records staged from BAM bytes give every output the column route gives"""
    b, h, refs, sites, meta = _case(1, 0)
    raw = orc.bam_encode(b, h.rg_ids)
    e, e2 = Engine(h), Engine(h)
    e.set_read_group_ids(h.rg_ids)
    e.stage_bam(raw)
    e2.stage(b)
    assert e.n == b.n and e.n_sorted == e2.n_sorted == orc.num_sorted(b)
    for x, y in zip(e.adapted(), e2.adapted()):
        assert np.array_equal(x, y)
    got, got2 = _whole_path(e, b, h, refs, sites), _whole_path(e2, b, h, refs, sites)
    want = _oracle_path(b, h, refs, sites)
    _same(got, want)
    _same(got2, want)
    oflags, operm, _, _, oqual = want
    out = e.emit_sorted_bam()
    exp = orc.bam_encode(b, h.rg_ids, order=operm[:orc.num_sorted(b)], flags=oflags, qual=oqual, normalize_tags=True)
    assert out.size == exp.size and np.array_equal(out, exp)
    # the bins of the records whose N spans cross 2^14 / 2^17 boundaries, read from the stream
    where, p = {}, 0
    order = operm[:orc.num_sorted(b)].tolist()
    for k in range(len(order)):
        where[order[k]] = p
        p += 4 + int(out[p:p + 4].view(np.uint32)[0])
    levels = {_bin_level(int(out[where[i] + 14:where[i] + 16].view(np.uint16)[0])) for i in meta["bin"]}
    assert {3, 4} <= levels, levels
    e.close()
    e2.close()


def test_clipping_panics_surface_as_errors():
    """single records where the clipping restatement (tests/test_oracle_kat.py) says the reference panics - a leading D or an insertion
    at the adaptor boundary: the gather raises ElpError like the oracle, and the context runs the next read set as a new one would"""
    b0, h, refs, sites, meta = _case(1, 0)
    rng = np.random.default_rng(17)
    found = []
    while len(found) < 4:
        ops = _draw_all_ops(rng, n_hi=50)
        if any(o == "N" for _, o in ops):
            continue
        L = sum(l for l, o in ops if o in _READ)
        span = sum(l for l, o in ops if o in _REF)
        pos = int(rng.integers(1000, 2000))
        revd = rng.random() < 0.5
        flag = 0x1 | 0x40 | (0x10 if revd else 0x20)
        edges, r = [pos], pos
        for l, o in ops:
            if o in _REF:
                r += l
                edges.append(r)
        t = edges[int(rng.integers(0, len(edges)))] + int(rng.integers(-1, 2))
        pnext, tlen = (t + 1, -(span + 10)) if revd else (pos, t - pos)
        try:
            _c_clip(dict(ops=ops, L=L, pos=pos, flag=flag, pnext=pnext, tlen=tlen, next_refid=0))
            continue
        except _ClipPanic:
            pass
        found.append(dict(qname="p", flag=flag, refid=0, pos=pos, mapq=60, cigar=_cig(ops), next_refid=0, pnext=pnext, tlen=tlen,
                          seq="".join("ACGT"[int(x)] for x in rng.integers(0, 4, L)), qual=[30] * L, rgid=0))
    good = b0.take(np.arange(300))
    for rec in found:
        pb = batch_from_records([rec])
        with pytest.raises(RuntimeError):
            orc.bqsr_gather(pb, h, orc.BqsrRef(refs, sites), orc.mark_duplicates(pb, h), 500)
        e = Engine(h)
        e.stage(pb)
        e.mark_duplicates(True)
        for r in range(h.n_ref):
            e.set_reference(r, refs[r])
            e.set_known_sites(r, sites[r])
        with pytest.raises(ElpError, match="non-existing base"):
            e.recalibrate(500)
        e.reset()
        e.stage(good)
        _same(_whole_path(e, good, h, refs, sites), _oracle_path(good, h, refs, sites))
        e.close()


@pytest.mark.parametrize("count_kernel", [0, 1, 3])
def test_known_site_next_to_a_deletion_in_one_run_of_matches(monkeypatch, count_kernel):
    """found by 18M0I8X47=0D47=12=19= (151 bases): count3 took the reference window's known-site flags of a read that is ONE run of matches
    on top of its skip-column bits - but a D in such a read (zero-length, or trailing and never clipped) moves the reference's read
    coordinate of a site that ends just before it one base to the left (filters/utils.go:306-316), so the base the site covers was skipped
    as well.  A site on exactly that base for every read; count_kernel 1 is the general kernel, the others count3."""
    b0, h, refs, sites0, meta = _case(151, 151)
    rng = np.random.default_rng(23)
    # (CIGAR, reference offset from POS of the base behind a zero-length D / of the last base before a trailing D)
    shapes = [("74=0D77=", 74), ("18M0I8X47=0D47=12=19=", 73), ("60M0D0I91M", 60), ("151M3D", 150), ("2S146X3S2D", 145), ("100M0P0D51M", 100)]
    recs, ivs = [], []
    for k in range(600):
        cig, at = shapes[k % len(shapes)]
        pos = 1000 + 1000 * k
        recs.append(dict(qname="s%d" % k, flag=0x10 if rng.random() < 0.5 else 0, refid=0, pos=pos, mapq=60, cigar=cig,
                         seq="".join("ACGT"[int(x)] for x in rng.integers(0, 4, 151)), qual=rng.choice([20, 30, 40], 151), rgid=int(rng.integers(0, 3))))
        ivs.append((pos + at, pos + at + int(rng.integers(0, 2))))
    b = batch_from_records(recs)
    sites = [orc.flatten(orc.sort_by_start(np.asarray(ivs, np.int32))), sites0[1]]
    monkeypatch.setenv("ELP_TUNE", "count_kernel=%d" % count_kernel)
    _check_gather_apply(b, h, refs, sites, chunks=1)
