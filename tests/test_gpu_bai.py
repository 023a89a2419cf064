"""GPU tests (-m gpu) of elp_index_sorted_bgzf / elp_index_merged_bgzf: the device's BAM index must equal tests/bairef.py's canonical
index of the bytes the emitter returned, bit for bit, on a fresh and on a reused context, and the independent reader bairef.query must
find through it what a scan over all records finds, on regions that end at, on and one past every window seam and record end present.
Record sizes are steered with a padding ZP:Z field (bairef.bam_record): a mapped record with one CIGAR operation is 44 bytes + 4 + pad."""
import ctypes as C
import struct

import numpy as np
import pytest

from elprep_amd import sfm
from elprep_amd.batch import Header
from elprep_amd.engine import ElpError, Engine, _vp
from tests import bairef
from tests.bairef import PAYLOAD, bam_record

pytestmark = pytest.mark.gpu

ELP_ERR_ARG, ELP_ERR_DATA, ELP_ERR_UNSUPPORTED = -1, -4, -5
M, S = 0, 4
BIG_BASE = (1 << 33) + 12345  # a file offset above 2^32


def _header(n_ref=3, ref_len=600_000_000):
    return Header(ref_len=np.full(n_ref, ref_len, np.int32), rg_lib=np.array([0], np.uint16), rg_cov=np.array([0], np.uint16),
                  ref_names=["c%d" % r for r in range(n_ref)], rg_ids=["rg0"])


def rec(refid, pos, span=10, size=None, flag=0, **kw):
    """a mapped record <span>M at BAM position pos, of `size` bytes in all if given (>= 48)"""
    pad = None if size is None else size - 48
    assert pad is None or pad >= 0
    r = bam_record(refid, pos, flag=flag, cigar=[(span, M)], pad=pad, **kw)
    assert size is None or len(r) == size
    return r


def _stage(e, recs):
    if recs:
        e.stage_bam(np.frombuffer(b"".join(recs), np.uint8))


def _engine(h, recs, replace_rg=None):
    e = Engine(h)
    if replace_rg is None:
        e.set_read_group_ids(h.rg_ids)
    else:
        e.set_replace_read_group(replace_rg)
    _stage(e, recs)
    return e


def _regions(bz, n_ref):
    """per contig, regions that end one before, on and one past every window seam and record end present (and begin a little in front),
    and the single positions there; at most 24 seams per contig, the first and last always"""
    stream = b"".join(d for _, d in bairef.members(bz)[0])
    seams = [set() for _ in range(n_ref)]
    at = 0
    while at < len(stream):
        size, refid, beg, end, _ = bairef.record_fields(stream, at)
        at += size
        if refid >= 0:
            seams[refid] |= {end, beg, (beg >> 14) << 14, ((end - 1 >> 14) + 1) << 14}
    out = []
    used = {r for r in range(n_ref) if seams[r]}
    for refid in sorted(r for r in used | {q + d for q in used for d in (-1, 1)} | {0, n_ref - 1} if 0 <= r < n_ref):  # and the empty contigs beside
        s = sorted(x for x in seams[refid] if x > 0)
        if len(s) > 24:
            s = sorted(set(s[:: len(s) // 22] + [s[0], s[-1]]))
        for x in s:
            out += [(refid, max(0, e_ - 70), e_) for e_ in (x - 1, x, x + 1) if e_ > 0] + [(refid, x, x + 1), (refid, max(0, x - 1), x + 16384)]
        out.append((refid, 0, 1 << 29))
    return out


def _check_index(bai, bz, base, n_ref):
    """the index against the reference's, then used by the independent reader"""
    bai, bz = bai.tobytes(), bz.tobytes()
    want = bairef.build(bz, base, n_ref)
    if bai != want:  # say where
        first = next((k for k, (a, b) in enumerate(zip(bai, want)) if a != b), min(len(bai), len(want)))
        raise AssertionError(("index differs", len(bai), len(want), "first difference at byte", first, bai[first & ~7:(first & ~7) + 16].hex(), want[first & ~7:(first & ~7) + 16].hex()))
    for refid, beg, end in _regions(bz, n_ref):
        assert bairef.query(bai, bz, base, refid, beg, end) == bairef.brute_force(bz, base, refid, beg, end), (refid, beg, end)
    return bai


def _index_of(e, n_ref, base=0):
    bz = e.emit_sorted_bgzf()
    return _check_index(e.index_sorted_bgzf(bz, base), bz, base, n_ref), bz


WARM = [rec(0, 50 + 3 * k, span=1 + 200 * (k % 90), size=48 + 37 * (k % 50)) for k in range(1500)]  # a larger set, for the reused context


def _fresh_and_reused(h, recs, base=0, before_sort=None, tuning=()):
    """the case on a fresh context, and on one that has indexed a larger read set before (scratch slots longer than the case needs, filled
    with that set's values); -> the index"""
    out = []
    for reuse in (False, True):
        e = _engine(h, WARM if reuse else recs)
        try:
            if reuse:
                e.sort_coordinate(fetch=False)
                e.index_sorted_bgzf(e.emit_sorted_bgzf(), 77)
                e.reset()
                _stage(e, recs)
            for key, value in tuning:
                e.set_tuning(key, value)
            if before_sort:
                before_sort(e)
            e.sort_coordinate(fetch=False)
            bai, bz = _index_of(e, h.n_ref, base)
            out.append(bai)
            # the call left the context as it was: the same stream (a compressed member's DEFLATE data depends on the launch that made it:
            # what it inflates to is compared), the same index of the same bytes
            assert [d for _, d in bairef.members(e.emit_sorted_bgzf().tobytes())[0]] == [d for _, d in bairef.members(bz.tobytes())[0]]
            assert e.index_sorted_bgzf(bz, base).tobytes() == bai
        finally:
            e.close()
    if dict(tuning).get("bgzf_stored"):  # (stored members are the same bytes every time, so the two indices are)
        assert out[0] == out[1]
    return out[0]


# ---- the cases.  Positions ascend and differ, so the output order is the order written here
def _phases():
    """starts: a 0; b 65279 (phase 65279); c 65328; d 130560 (phase 0); e 195841 (phase 1); f 195889.  ends: a 65279 (phase 65279); c
    130560 (phase 0); d 195841 (phase 1); f 261120 = 4 x 65280: the last record ends exactly on the last member's end.  Bins alternate."""
    recs = [rec(0, 100, size=65279), rec(0, 16380, size=49), rec(0, 16390, size=65232), rec(0, 32760, size=65281), rec(0, 32770, size=48), rec(0, 32780, size=65231)]
    assert sum(len(r) for r in recs) == 4 * PAYLOAD
    return recs


def _long_record():
    """the second record is longer than two members: it covers member 1 whole, no record starts there"""
    return [rec(0, 100, size=100), rec(0, 200, span=20000, size=140000), rec(0, 300, size=60), rec(1, 5, size=60)]


def _levels():
    """contig 0: records that straddle 2^14, 2^17, 2^20, 2^23 and 2^26 - every bin level and bin 0 -, ends at 16383, 16384 and 16385, an
    end at 2^29 exactly.  Contig 1: the first record far in (a run of untouched windows at the start), the next far behind it (a run in
    the middle).  Contig 2: POS 0 (the BAM field -1: beg clamped to 0), an unmapped placed read, a mapped read without CIGAR, a read
    whose CIGAR consumes no reference.  Then unplaced reads."""
    c0 = [rec(0, 100), rec(0, 16000, span=383), rec(0, 16001, span=383), rec(0, 16002, span=383), rec(0, 16380, span=10), rec(0, 130000, span=2000),
          rec(0, 1048000, span=1000), rec(0, 8388000, span=1000), rec(0, 67108000, span=1000), rec(0, (1 << 29) - 10, span=10)]
    c1 = [rec(1, 5_000_000, span=40000), rec(1, 5_000_100), rec(1, 9_000_000, span=16384), rec(1, 9_016_384)]
    c2 = [rec(2, -1, span=5), bam_record(2, 500, flag=4), bam_record(2, 600), bam_record(2, 700, cigar=[(5, S)], l_seq=5), rec(2, 20000)]
    return c0 + c1 + c2 + [bam_record(-1, -1, flag=4, name=b"u%d" % k) for k in range(3)]


def _revisits():
    """bin 4681 (X) and bin 585 (Y, records that cross 2^14): X Y X in member 0 - the second X extends X's chunk across the foreign record:
    one chunk -; then a Y of 70000 bytes that runs into member 1 and an X there: X's second chunk; Y's records follow each other: one"""
    return [rec(0, 100, size=100), rec(0, 200, span=17000, size=100), rec(0, 300, size=100), rec(0, 400, span=17000, size=70000), rec(0, 500, size=100)]


CASES = {
    "phases": (_phases, 3),
    "long_record": (_long_record, 3),
    "short_stream": (lambda: [rec(0, 10 + k, size=48 + k) for k in range(5)], 3),
    "empty": (lambda: [], 3),
    "only_unplaced": (lambda: [bam_record(-1, -1, flag=4, name=b"u%d" % k, pad=k) for k in range(5)], 3),
    "levels": (_levels, 3),
    "revisits": (_revisits, 3),
    "many_contigs": (lambda: [rec(0, 10), rec(0, 20000), rec(35000, 7), rec(35000, 40000, span=70000), rec(69999, 1 << 20), bam_record(-1, -1, flag=4)], 70000),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_index_equals_the_reference(name):
    make, n_ref = CASES[name]
    bai = _fresh_and_reused(_header(n_ref), make())
    contigs, n_no_coor = bairef.parse(bai)
    if name == "revisits":
        assert len(contigs[0][0][4681]) == 2 and len(contigs[0][0][585]) == 1
    if name == "levels":
        assert set(contigs[0][0]) >= {0, 1, 9, 73, 585, 4681} and len(contigs[0][1]) == 1 << 15 and n_no_coor == 3
        assert contigs[1][1][0] == contigs[1][1][5_000_000 >> 14] and contigs[2][1][0] < contigs[2][1][1]
    if name == "empty":
        assert bai == b"BAI\1" + struct.pack("<iiiiiii", 3, 0, 0, 0, 0, 0, 0) + bytes(8)
    if name == "only_unplaced":
        assert n_no_coor == 5 and all(not b and not io for b, io in contigs)
    if name == "many_contigs":
        assert [r for r, (b, _) in enumerate(contigs) if b] == [0, 35000, 69999]


def _random_set(n, seed=3):
    rng = np.random.default_rng(seed)
    recs, pos = [], 0
    for k in range(n):
        pos += int(rng.integers(1, 700))
        unm = k % 37 == 5
        recs.append(bam_record(k * 3 // n, pos, flag=4 if unm else 0, cigar=[] if unm else [(int(rng.choice([1, 40, 150, 20000])), M)], name=b"q%d" % k,
                               pad=int(rng.integers(20000, 66000)) if k % 29 == 0 else int(rng.integers(0, 300)), mapq=k % 50))
    return recs + [bam_record(-1, -1, flag=4, name=b"u")] * 2


@pytest.mark.parametrize("stored", [0, 1])
@pytest.mark.parametrize("base", [0, BIG_BASE])
def test_index_does_not_depend_on_the_passes(stored, base):
    """400 records in some 15 members; with 7 and with 97 records per pass members and records straddle passes and bytes are carried"""
    h, recs = _header(), _random_set(400)
    want = _fresh_and_reused(h, recs, base, tuning=(("bgzf_stored", stored),))
    for per_pass in (7, 97):
        got = _fresh_and_reused(h, recs, base, tuning=(("bgzf_stored", stored), ("emit_pass", per_pass)))
        # (each was compared with the reference's index of its own bytes; stored members are the same bytes wherever the passes fall)
        assert got == want or not stored, per_pass
    assert len(bairef.parse(want)[0][0][0]) > 3


def test_settings_that_change_sizes_and_spans():
    """a tag filter that drops the padding, a replacing read group that adds a field, CleanSam that clips a read at its contig's end (the
    span shrinks), records rejected by a filter and sr-tagged records (neither is output)"""
    h = _header(2, 100000)
    recs = [bam_record(0, 10 + 5 * k, cigar=[(30, M)], l_seq=30, name=b"q%d" % k, pad=(k * 53) % 400, mapq=k % 3 * 20, tags=b"srC\1" if k % 11 == 3 else b"")
            for k in range(900)]
    recs += [bam_record(1, 99990, cigar=[(50, M)], l_seq=50, pad=70000, mapq=40), bam_record(1, 99995, cigar=[(50, M)], l_seq=50, mapq=40)]
    plain = _fresh_and_reused(h, recs)
    def settings(e):
        assert e.clean_sam() == 2
        assert e.filter_records(min_mapq=20) > 100
        e.set_tag_filter(remove=["ZP"])
    e = _engine(h, recs, replace_rg="another")
    try:
        settings(e)
        e.sort_coordinate(fetch=False)
        assert 0 < e.n_sorted < 800
        bai, bz = _index_of(e, 2, 5)
        stream = b"".join(d for _, d in bairef.members(bz.tobytes())[0])
        assert b"ZPZ" not in stream and stream.count(b"RGZanother\0") == e.n_sorted and len(stream) < 2 * PAYLOAD
        assert len(bairef.parse(bai)[0][1][1]) == 7 and len(bairef.parse(plain)[0][1][1]) == 7  # clipped at 100000 or not: the last window is 6
        assert len(bai) != len(plain) or bai != plain
        e.set_tag_filter()
        _index_of(e, 2, 5)
    finally:
        e.close()


def _raw(e, bz, base, out, cap=None):
    n = C.c_uint64(0)
    bz = np.ascontiguousarray(bz, np.uint8)
    return e.L.elp_index_sorted_bgzf(e.h, _vp(bz), bz.size, base, _vp(out) if out is not None else C.c_void_p(0), out.size if cap is None else cap, C.byref(n)), int(n.value)


def test_refusals_and_sizes():
    h = _header()
    recs = _random_set(300)
    e, other = _engine(h, recs), _engine(h, recs[:200])
    try:
        out = np.full(1 << 20, 0xAA, np.uint8)
        def refused(code, bz, base=0, eng=e):
            rc, _ = _raw(eng, bz, base, out)
            assert rc == code and (out == 0xAA).all(), (rc, code)
        empty = np.zeros(0, np.uint8)
        refused(ELP_ERR_ARG, empty)                                 # no permutation at all
        e.sort_queryname(fetch=False)
        bz_q = e.emit_sorted_bgzf()
        refused(ELP_ERR_ARG, bz_q)                                  # a queryname permutation
        e.order_keep(by_split=True, fetch=False)
        refused(ELP_ERR_ARG, e.emit_sorted_bgzf())                  # a permutation by split
        e.sort_coordinate(fetch=False)
        other.sort_coordinate(fetch=False)
        bz, bz_other = e.emit_sorted_bgzf(), other.emit_sorted_bgzf()
        refused(ELP_ERR_ARG, bz_other)                              # another context's stream
        refused(ELP_ERR_ARG, bz[:0])
        refused(ELP_ERR_ARG, bz, 1 << 48)
        refused(ELP_ERR_DATA, bz[:-1])                              # damaged members
        bad = bz.copy()
        bad[0] ^= 1
        refused(ELP_ERR_DATA, bad)
        # the size query is exact; one byte less room is refused and writes nothing
        rc, size = _raw(e, bz, 0, None, 0)
        assert rc == 0 and size == len(bairef.build(bz.tobytes(), 0, 3))
        rc, _ = _raw(e, bz, 0, out, size - 1)
        assert rc == ELP_ERR_ARG and (out == 0xAA).all()
        rc, n = _raw(e, bz, 0, out, size)
        assert (rc, n) == (0, size) and (out[size:] == 0xAA).all() and out[:size].tobytes() == bairef.build(bz.tobytes(), 0, 3)
        with pytest.raises(ElpError) as ei:
            e.index_sorted_bgzf(bz_other)
        assert ei.value.code == ELP_ERR_ARG and "not this context's stream" in str(ei.value)
    finally:
        e.close()
        other.close()


def test_a_record_that_ends_beyond_2_to_the_29_is_refused():
    h = _header()
    e = _engine(h, [rec(0, 100), rec(0, (1 << 29) - 5, span=10)])
    try:
        e.sort_coordinate(fetch=False)
        with pytest.raises(ElpError) as ei:
            e.index_sorted_bgzf(e.emit_sorted_bgzf())
        assert ei.value.code == ELP_ERR_UNSUPPORTED
    finally:
        e.close()


def test_keep_permutations():
    """input order: sorted input passes and gives the sort's index; unsorted input is refused"""
    h, recs = _header(), _random_set(400)
    e = _engine(h, recs)
    try:
        e.set_tuning("bgzf_stored", 1)  # (the same bytes from both contexts)
        e.sort_coordinate(fetch=False)
        want, _ = _index_of(e, 3)
    finally:
        e.close()
    for at in (None, 255, 256, 1):
        order = list(range(len(recs) - 2))
        if at is not None:
            order[at - 1], order[at] = order[at], order[at - 1]
        e = _engine(h, [recs[k] for k in order] + recs[-2:])
        try:
            e.set_tuning("bgzf_stored", 1)
            e.order_keep(fetch=False)
            if at is None:
                assert _index_of(e, 3)[0] == want
            else:
                with pytest.raises(ElpError) as ei:
                    e.index_sorted_bgzf(e.emit_sorted_bgzf())
                assert ei.value.code == ELP_ERR_DATA and "not in coordinate order" in str(ei.value)
        finally:
            e.close()


# ---- the merged stream
def _merged_check(eg, es, n_ref, base):
    for per_pass in (0, 97):
        eg.set_tuning("emit_pass", per_pass)
        bz = eg.emit_merged_bgzf(es)
        _check_index(eg.index_merged_bgzf(es, bz, base), bz, base, n_ref)
    eg.set_tuning("emit_pass", 0)
    return bz


@pytest.mark.parametrize("order", ["coordinate", "keep"])
def test_merged_index_on_the_keep_order_read_set(order):
    from tests.test_gpu_keep_order import _sorted_case, _split_on_device
    h, b, gof, n_groups, split, spread = _sorted_case()
    eg, es = _split_on_device(h, b, gof, n_groups)
    try:
        for e in (eg, es):
            sfm._order_call(e, order)(False)
        bz = _merged_check(eg, es, h.n_ref, BIG_BASE if order == "keep" else 0)
        assert len(bairef.members(bz.tobytes())[0]) > 3
        # the groups' own stream is another one
        with pytest.raises(ElpError) as ei:
            eg.index_merged_bgzf(es, eg.emit_sorted_bgzf())
        assert ei.value.code == ELP_ERR_ARG
        # a queryname permutation: as elp_emit_merged_bam refuses it
        es.sort_queryname(fetch=False)
        with pytest.raises(ElpError) as ei:
            eg.index_merged_bgzf(es, bz)
        assert ei.value.code == ELP_ERR_UNSUPPORTED
    finally:
        eg.close()
        es.close()


def test_merged_index_on_the_two_rank_read_set_and_through_sfm_rank():
    """the read set of the merge test across two ranks (tests/sfm_worker.py), here on one: through Engine, then one case through SfmRank"""
    import oracle as orc
    from tests import sfm_worker
    from tests.test_gpu_keep_order import _split_on_device
    cfg, gof, n_groups, owner, b = sfm_worker.make_rank_input(0, 1, pairs_per_rank=2500)
    h = cfg.header()
    eg, es = _split_on_device(h, b, gof, n_groups)
    try:
        for e in (eg, es):
            e.mark_duplicates(True, fetch=False)
            e.sort_coordinate(fetch=False)
        _merged_check(eg, es, h.n_ref, 0)
    finally:
        eg.close()
        es.close()
    rk = sfm.SfmRank(h, 0, sfm.Comm())
    try:
        raw = orc.bam_encode(b, h.rg_ids)
        for e in rk.engines:
            e.set_read_group_ids(h.rg_ids)
        rk.route(b, gof, n_groups, np.zeros(n_groups + 2, np.int32), stage=lambda e, x: e.stage_bam(raw))
        for e in rk.engines:
            e.sort_coordinate(fetch=False)
        bz = rk.emit_merged(gof, n_groups, np.zeros(n_groups + 2, np.int32), fmt="bgzf")
        _check_index(rk.index_merged(bz, 4096), bz, 4096, h.n_ref)
    finally:
        rk.close()
