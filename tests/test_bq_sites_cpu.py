"""The known-site read sets (tests/bq_sites.py) are what they claim to be, and the restatement there agrees with the oracle on them: for every
probe of the indel families and thousands of the ruler's reads the oracle's tables of the read ALONE hold exactly the bases the
restatement's mask leaves, at exactly their cycles.  The coverage the device test relies on - every word phase of k_ref_mark_sites, every
bit phase of the skip column's words in both forms, the thresholds of rec_simple, the bucket index - is computed from the masks and the
staged offsets, and the constants behind it are read out of the kernels.  Oracle only, no GPU."""
import os
import re

import numpy as np
import pytest

import oracle as orc
from tests import bq_sites as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csrc(name):
    with open(os.path.join(ROOT, "elprep_amd", "csrc", name)) as f:
        return f.read()


def test_seam_constants_are_the_kernels():
    host, pro, common, plan = _csrc("bqsr.hip"), _csrc("bqsr_prologue.hip"), _csrc("bqsr_common.hpp"), _csrc("bqsr_plan.hpp")
    # k_ref_mark_sites: words of 8 bases, a mask cut on both sides
    assert 1 << int(re.search(r"const int64_t w = j >> (\d+);", host).group(1)) == bs.WORD
    assert "(0x44444444u >> (4 * (7 - b))) & (0x44444444u << (4 * a))" in host
    # k_site_index and the prologues' entries into it: buckets of 64 bases
    assert 1 << int(re.search(r"const int64_t x = b << (\d+);", host).group(1)) == bs.BUCKET
    assert re.search(r"nbuck = \(\(int64_t\)c->h_ref_len\[refid\] >> (\d+)\) \+ 1;", host).group(1) == "6"
    assert re.findall(r"\(p < rl \? p : rl\) >> (\d+);", pro) == ["6"] and re.findall(r"\(ss < 0 \? 0 : ss\) >> (\d+);", pro) == ["6"]
    # the skip column: words of 32 bits, in both helpers
    assert re.findall(r"(?:int|uint32_t) cnt = (\d+) - in_word;", pro) == [str(bs.SKIPW)] * 2
    assert len(re.findall(r"\(cnt == (\d+) \? 0xFFFFFFFFu", pro)) == 2 and pro.count("b & 31") == 2 and pro.count("b >> 5") == 2
    # rec_simple and make_rec's tests that it restates; the plan's longest one-length read
    m = re.search(r"rec_simple = recs && !plain && len <= (\d+) && \(int64_t\)p - 1 - \(int64_t\)aoff >= (\d+) && .*? <= rec_rlen \+ (\d+);", pro)
    assert [int(x) for x in m.groups()] == [bs.REC_MAXLEN, bs.REC_LO, bs.REC_HI]
    m = re.search(r"general \|= E0 < (\d+) \|\| E0 \+ lorig > rlen \+ (\d+);", common)
    assert [int(x) for x in m.groups()] == [bs.REC_LO, bs.REC_HI]
    assert re.search(r"P\.np < 1 \|\| len > (\d+);", common).group(1) == str(bs.REC_MAXLEN)
    assert re.search(r"g\.lmax > g\.max_cycle \|\| g\.lmax > (\d+)\)", plan).group(1) == str(bs.REC_MAXLEN)
    assert re.search(r"constexpr int REF_LDS = (\d+);", common).group(1) == str(bs.REF_LDS)


def test_restatement_quirks_by_hand():
    """the Go quirks, worked out on paper from utils.go:267-349"""
    c = bs.parse_cigar("20M3D20M")
    rc = lambda g: bs.read_coordinate(c, 100, 100 + g)
    assert rc(19) == (19, True) and rc(20) == (19, True)      # the first deleted base: one short
    assert rc(21) == (19, True) and rc(22) == (19, True)      # inside the D
    assert rc(23) == (20, True)                                # the base behind the D
    assert rc(42) == (39, True) and rc(43) == (-1, False)     # the goal reached at the end of the last element fails
    assert bs.read_coordinate(c, 100, 99) == (-1, False)
    assert bs.read_coordinate(bs.parse_cigar("3D40M"), 100, 101) == (-1, False)  # readBases -1 reads as "not found"
    assert bs.read_coordinate(bs.parse_cigar("3I37M"), 100, 100) == (3, True)    # the `left` rule
    assert bs.read_coordinate(bs.parse_cigar("20M3I17M"), 100, 120) == (23, True)
    assert bs.hard_clip_soft_clipped(100, bs.parse_cigar("5S15M2D15M5S")) == (100, bs.parse_cigar("5H15M2D15M5H"), 30, 5)
    assert bs.hard_clip_soft_clipped(100, bs.parse_cigar("2H36M2H")) == (100, bs.parse_cigar("2H36M2H"), 36, 0)
    # 3D40M with a site that ends inside the leading D: fe is "not found", the whole read is masked
    mask, lo = bs.skip_mask(100, bs.parse_cigar("3D40M"), [(99, 101)])
    assert mask.all() and lo == 0
    mask, lo = bs.skip_mask(100, bs.parse_cigar("3S34M"), [(90, 100), (110, 111)])
    assert lo == 3 and np.nonzero(mask)[0].tolist() == [0, 10, 11]
    assert not bs.needs_adaptor_clip(0x1 | 0x40 | 0x20, 100, c, 0, 300, 250)
    assert bs.needs_adaptor_clip(0x1 | 0x40 | 0x20, 100, c, 0, 90, 30)


def test_site_lists_are_flat_and_sizes_small():
    for name, make in bs.CASES.items():
        case = make()
        assert case.b.n <= 20000 and int(case.h.ref_len.max()) <= 300_000, name
        assert (case.b.qual >= 6).all() and ((case.b.seq4 >> 4) != 15).all() and ((case.b.seq4 & 15) != 15).all()  # no N
        assert not (case.b.flag & 0x80).any() and (name == "adaptor" or not (case.b.flag & ~np.uint16(0x10)).any())
        for which in bs.LISTS:
            for r, s in enumerate(case.sites_of(which)):
                assert np.array_equal(orc.flatten(s), s), (name, which, r)
                assert (s[1:, 0] - s[:-1, 1] >= 2).all() and (s[:, 0] <= s[:, 1]).all() and (s[:, 0] >= 1).all(), (name, which, r)
        # B takes the sites away from the reads that had them: the indel probes, the ruler's reads near the start of contig 0
        if name.startswith("indels"):
            for i in range(case.b.n):
                assert not bs.skip_mask(int(case.b.pos[i]), case.cig[i], case.sites["B"][case.b.refid[i]])[0].any(), (name, i)
    ref_len, a, b, long_site = bs.ruler_layout()
    assert [ln % bs.BUCKET for ln in ref_len[:1] + ref_len[2:]] == [bs.BUCKET - 1, 0, 1]
    assert a[1] == [] and a[0] and a[2] and b[1] and b[2] == []                          # an empty list between two, both ways round
    assert a[0][0] == (1, 1) and a[0][-1] == (ref_len[0], ref_len[0]) and a[2][-1][1] > ref_len[2]
    assert long_site[1] - long_site[0] + 1 == 300 and long_site[1] // bs.BUCKET - long_site[0] // bs.BUCKET >= 4
    assert not any(s <= 160 for s, _ in b[0]) and bs.many_contigs().h.n_ref == bs.REF_LDS + 1 and bs.many_contigs().sites["A"][-1]
    for name in bs.RECORD_CASES:
        assert bs.CASES[name]().uniform, name
    assert not bs.ruler(0).uniform and set(bs.ruler(0).b.l_seq.tolist()) >= set(range(1, 71))
    assert int(bs.ruler_long(1022).b.l_seq[0]) == bs.REC_MAXLEN and int(bs.ruler_long(1023).b.l_seq[0]) == bs.REC_MAXLEN + 1


def _check_alone(case, idx):
    """the oracle on each read of idx alone against the restatement's mask -> reads checked"""
    ref = orc.BqsrRef(case.refs, case.sites_of("A"))
    b = case.b
    for i in idx:
        i = int(i)
        assert not bs.needs_adaptor_clip(int(b.flag[i]), int(b.pos[i]), case.cig[i], int(b.next_refid[i]), int(b.pnext[i]), int(b.tlen[i]))
        mask, lo = bs.skip_mask(int(b.pos[i]), case.cig[i], case.sites["A"][b.refid[i]])
        n = mask.size
        qt, ct, _ = orc.bqsr_gather(b.take([i]), case.h, ref, None, case.max_cycle)
        where = (case.name, i, b.cigar_of(i), int(b.pos[i]), int(b.flag[i]))
        assert int(qt[..., 0].sum()) == n - int(mask.sum()), where
        kept = np.nonzero(~mask)[0]
        cycles = (n - kept) if b.flag[i] & 0x10 else (kept + 1)  # prepareCycleCovariates, bqsr.go:376-383, unpaired
        got = np.nonzero(ct[case.fam[i], 6 + case.probe[i] % case.nq, :, 0])[0] - case.max_cycle
        assert sorted(got.tolist()) == sorted(cycles.tolist()), where
        assert int(ct[..., 0].sum()) == kept.size, where
    return len(idx)


@pytest.mark.parametrize("L", bs.INDEL_LENGTHS)
def test_restatement_against_the_oracle_every_indel_probe(L):
    case = bs.indels(L)
    assert _check_alone(case, np.arange(case.b.n)) == case.b.n
    masks = [bs.skip_mask(int(case.b.pos[i]), case.cig[i], case.sites["A"][case.b.refid[i]])[0] for i in range(case.b.n)]
    for fam in set(case.fam.tolist()):  # every family sees reads without a masked base, with one, and (w = 6) with several
        counts = {int(m.sum()) for m, f in zip(masks, case.fam) if f == fam}
        assert (0 in counts or bs.SHAPES[fam] == bs.WORDS_SHAPE) and 1 in counts and max(counts) >= 4, (L, bs.SHAPES[fam], counts)


def test_every_shape_and_a_reverse_twin_for_half_of_the_probes():
    seen = set()
    for L in bs.INDEL_LENGTHS:
        case = bs.indels(L)
        seen |= {bs.SHAPES[f] for f in case.fam}
        if L != 101:  # (the word-phase family has no twins: its reads' QUAL offsets are the probe index times 101)
            twins = int(((case.b.flag & 0x10) != 0).sum())
            assert abs(2 * twins - (case.b.n - twins)) <= len(set(case.fam.tolist())), L
    assert seen == set(bs.SHAPES)
    assert [s.count("I") + s.count("D") for s in bs.SHAPES].count(4) == 1  # the shape with four indels: more than three pieces


def test_adaptor_reads_are_clipped_and_sites_straddle_the_clip_point():
    case = bs.adaptor()
    b = case.b
    straddle = {0: 0, 1: 0}
    for i in range(b.n):
        assert bs.needs_adaptor_clip(int(b.flag[i]), int(b.pos[i]), case.cig[i], int(b.next_refid[i]), int(b.pnext[i]), int(b.tlen[i])), i
        a, e, pos, _ = orc.clip_for_bqsr(b, i)  # the bases left: [a, e) of the read, the first of them at `pos`
        s0, s1 = case.sites["A"][0][i]
        if b.flag[i] & 0x10:
            assert a >= 5 and e == 50 and pos == b.pnext[i], i
            straddle[1] += s0 < pos <= s1
        else:
            assert a in (0, 4) and e < 50, i
            straddle[0] += s0 <= b.pos[i] + b.tlen[i] - 1 < s1  # the last base in front of the boundary POS + |TLEN|
    assert straddle[0] >= 5 and straddle[1] >= 5
    assert int(case.expected("0")[0][..., 0].sum()) - int(case.expected("A")[0][..., 0].sum()) >= 30


def _ruler_sample(case):
    b = case.b
    ln = case.h.ref_len[b.refid]
    edge = (b.pos <= 130) | (b.pos > ln - 150)
    return np.nonzero(edge | (np.arange(b.n) % 7 == 0))[0]


@pytest.mark.parametrize("name", ["ruler37", "ruler101", "ruler_ragged", "ruler_long1022", "ruler_long1023", "many_contigs"])
def test_restatement_against_the_oracle_ruler_reads(name):
    case = bs.CASES[name]()
    idx = _ruler_sample(case) if name.startswith("ruler") and "long" not in name else np.arange(case.b.n)
    assert _check_alone(case, idx) >= (2000 if name in ("ruler37", "ruler101", "ruler_ragged") else 40)


# ------------------------------------------------------------------------------------------------------------------------ coverage
def _masks(case, idx=None):
    b = case.b
    for i in (range(b.n) if idx is None else idx):
        mask, lo = bs.skip_mask(int(b.pos[i]), case.cig[i], case.sites["A"][b.refid[i]])
        yield int(i), mask, lo


def _runs(mask):
    """-> [(first, last)] of the runs of set entries"""
    d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


def test_every_word_phase_of_the_reference_flags():
    """every (start phase, end phase) of the 8-base word over 1, 2 and 3 words, as k_ref_mark_sites cuts a site into words; the clamps at
    base 0 and behind the contig's end"""
    ref_len, a, _, _ = bs.ruler_layout()
    seen = set()
    for s, e in a[0]:
        lo, hi = s - 1, e - 1
        nw = hi // bs.WORD - lo // bs.WORD + 1
        if nw <= 3:
            seen.add((nw, lo % bs.WORD, hi % bs.WORD))
    want = {(nw, x, y) for nw in (1, 2, 3) for x in range(bs.WORD) for y in range(bs.WORD) if nw > 1 or y >= x}
    assert want <= seen
    assert any(s == 1 for s, _ in a[0]) and any(e > ln for per, ln in zip(a, ref_len) for _, e in per)


def test_every_bit_phase_of_the_skip_column_in_both_forms():
    """runs of masked bases by the bit phases of their first and last base in the column's 32-bit words: every pair out of {0, 1, 30, 31},
    a run over one whole word and one over two - among the reads that use the column when descriptors are written (every read with a
    site) and among those that use it when records are (not rec_simple)"""
    pairs = {"descriptors": set(), "records": set()}
    whole = {"descriptors": 0, "records": 0}
    for name in ("indels101", "indels37", "ruler37"):
        case = bs.CASES[name]()
        idx = None if name != "ruler37" else np.nonzero(case.b.pos <= 60)[0]
        for i, mask, lo in _masks(case, idx):
            forms = ["descriptors"] + ([] if case.rec_simple(i) else ["records"])
            for f, l in _runs(mask):
                bit0, bit1 = int(case.b.qual_off[i]) + lo + f, int(case.b.qual_off[i]) + lo + l
                words = (bit1 + 1) // bs.SKIPW - -(-bit0 // bs.SKIPW)  # whole words inside [bit0, bit1]
                for form in forms:
                    pairs[form].add((bit0 % bs.SKIPW, bit1 % bs.SKIPW))
                    whole[form] = max(whole[form], words)
    want = {(x, y) for x in (0, 1, 30, 31) for y in (0, 1, 30, 31)}
    for form in pairs:
        assert want <= pairs[form], (form, sorted(want - pairs[form]))
        assert whole[form] >= 2, form


def test_the_thresholds_of_rec_simple_and_the_bucket_index():
    e0s, over, multi, own_bucket = set(), set(), 0, 0
    for name in ("ruler37", "ruler101", "ruler_long1022"):
        case = bs.CASES[name]()
        b = case.b
        for i in range(b.n):
            s = case.simple(i)
            assert s is not None
            e0 = int(b.pos[i]) - 1 - s[0]
            e0s.add(e0 if e0 >= 0 else -1)
            over.add((name, e0 + int(b.l_seq[i]) - int(case.h.ref_len[b.refid[i]])))
            assert case.rec_simple(i) == (e0 >= 16 and e0 + int(b.l_seq[i]) <= int(case.h.ref_len[b.refid[i]]) + 32 and s[1] <= 1022)
    assert {-1, bs.REC_LO - 1, bs.REC_LO, bs.REC_LO + 1} <= e0s
    for name in ("ruler37", "ruler101", "ruler_long1022"):
        assert {(name, bs.REC_HI + d) for d in (-1, 0, 1)} <= over
    case = bs.ruler(101)
    b = case.b
    sites = case.sites["A"][0]
    ends = np.array([e for _, e in sites])
    for i in np.nonzero((b.refid == 0) & (case.fam == 0))[0]:
        p = int(b.pos[i])
        multi += len(bs.intersect(sites, p, p + 100)) >= 3
        first = int(np.searchsorted(ends, bs.BUCKET * (min(p, int(case.h.ref_len[0])) // bs.BUCKET)))  # k_site_index
        own_bucket += first < len(sites) and sites[first][1] < p and sites[first][1] // bs.BUCKET == p // bs.BUCKET
    assert multi >= 100 and own_bucket >= 100
