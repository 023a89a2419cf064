"""tests/bairef.py pinned: the canonical index builder against bytes derived by hand, and the index reader against a scan over all
records.  The GPU tests (tests/test_gpu_bai.py) compare the device's index with build() and use it through query()."""
import random
import struct

from tests import bairef
from tests.bairef import bam_record, bgzf_write

M = 0  # CIGAR operation M


def _hand_file():
    """Ten records in one member.  A record with one CIGAR operation and the name "r" is 4 + 32 + 2 + 4 + 1 + 1 = 44 bytes, one without an
    operation 40.  Contig 0 holds one record per bin level, two of them in one smallest bin; contig 1 is empty; contig 2 holds an
    unmapped placed read and a mapped one; the last record is unplaced.

      #  refid  pos        CIGAR   [beg, end)             bin                         windows      starts at  ends at
      0  0      100        10M     100 .. 110             4681 + 0 = 4681             0            0          44
      1  0      200        10M     200 .. 210             4681                        0            44         88
      2  0      16000      1000M   16000 .. 17000         crosses 2^14: 585 + 0       0, 1         88         132
      3  0      130000     2000M   130000 .. 132000       crosses 2^17: 73 + 0        7, 8         132        176
      4  0      1048000    1000M   1048000 .. 1049000     crosses 2^20: 9 + 0         63, 64       176        220
      5  0      8388000    1000M   8388000 .. 8389000     crosses 2^23: 1 + 0         511, 512     220        264
      6  0      67108000   1000M   67108000 .. 67109000   crosses 2^26: 0             4095, 4096   264        308
      7  2      500        -, 0x4  500 .. 501             4681                        0            308        348
      8  2      20000      10M     20000 .. 20010         4681 + 1 = 4682             1            348        392
      9  -1                                                                                        392        432
    """
    recs = [bam_record(0, 100, cigar=[(10, M)]), bam_record(0, 200, cigar=[(10, M)]), bam_record(0, 16000, cigar=[(1000, M)]),
            bam_record(0, 130000, cigar=[(2000, M)]), bam_record(0, 1048000, cigar=[(1000, M)]), bam_record(0, 8388000, cigar=[(1000, M)]),
            bam_record(0, 67108000, cigar=[(1000, M)]), bam_record(2, 500, flag=4), bam_record(2, 20000, cigar=[(10, M)]), bam_record(-1, -1, flag=4)]
    assert [len(r) for r in recs] == [44] * 7 + [40, 44, 40]
    return bgzf_write(b"".join(recs))


def test_build_against_bytes_derived_by_hand():
    """The members stand at file offset 1000: the one member's virtual offsets are 1000 << 16 | place.  Contig 0: bins ascending 0, 1, 9,
    73, 585, 4681 - the two records of bin 4681 follow each other in one member: one chunk (0, 88) -, the pseudo-bin with the extent
    (0, 308) and 7 mapped, 0 unmapped; 4097 windows: window 0 is touched by records 0, 1 and 2 -> 0; window 1 by record 2 -> 88; 2 .. 6
    by nobody -> the value of window 7; 7, 8 -> 132; 9 .. 62 untouched, 63, 64 -> 176; 65 .. 510, 511, 512 -> 220; 513 .. 4094, 4095,
    4096 -> 264.  Contig 1: n_bin 0, n_intv 0.  Contig 2: bins 4681 (308, 348) and 4682 (348, 392), the pseudo-bin (308, 392), 1
    mapped, 1 unmapped; windows 0 -> 308, 1 -> 348.  One record without coordinates."""
    v = lambda place: 1000 << 16 | place
    q = lambda *x: struct.pack("<%dQ" % len(x), *x)
    bin_ = lambda number, *chunks: struct.pack("<Ii", number, len(chunks) // 2) + q(*chunks)
    want = b"BAI\1" + struct.pack("<i", 3)
    want += struct.pack("<i", 7) + bin_(0, v(264), v(308)) + bin_(1, v(220), v(264)) + bin_(9, v(176), v(220)) + bin_(73, v(132), v(176))
    want += bin_(585, v(88), v(132)) + bin_(4681, v(0), v(88)) + bin_(37450, v(0), v(308), 7, 0)
    want += struct.pack("<i", 4097) + q(*([v(0), v(88)] + [v(132)] * 7 + [v(176)] * 56 + [v(220)] * 448 + [v(264)] * 3584))
    want += struct.pack("<ii", 0, 0)
    want += struct.pack("<i", 3) + bin_(4681, v(308), v(348)) + bin_(4682, v(348), v(392)) + bin_(37450, v(308), v(392), 1, 1)
    want += struct.pack("<i", 2) + q(v(308), v(348))
    want += q(1)
    assert 2 + 7 + 56 + 448 + 3584 == 4097
    got = bairef.build(_hand_file(), 1000, 3)
    assert got == want
    # an empty stream: every contig empty
    assert bairef.build(b"", 5, 2) == b"BAI\1" + struct.pack("<iiiii", 2, 0, 0, 0, 0) + q(0)


def test_chunks_split_at_a_member_by_hand():
    """Records of 30000 bytes (40 + a ZP:Z field of 4 + 29956) of one smallest bin start at 0, 30000, 60000 and 90000: each starts where
    the one before ends, so each starts in the member the chunk ends in - one chunk, though the third ends at 90000 = place 24720 of
    member 1.  A fifth of 44 bytes at 120000 = place 54720 of member 1 extends it to place 54764.  Then a record of ANOTHER bin (20000M:
    10 .. 20010 crosses 2^14, bin 585; 44 + 4 + 29952 = 30000 bytes) runs to 150044 = 2 x 65280 + 19484 in member 2, and a seventh
    record of the first bin starts there: not the member its bin's chunk ends in - a second chunk.  Windows: 0 -> the first record, 1 ->
    the record of bin 585."""
    big = lambda pos: bam_record(0, pos, flag=4, pad=29956)
    recs = [big(10), big(10), big(10), big(10), bam_record(0, 10, cigar=[(1, M)]), bam_record(0, 10, cigar=[(20000, M)], pad=29952), big(10)]
    assert [len(r) for r in recs] == [30000] * 4 + [44, 30000, 30000]
    bz = bgzf_write(b"".join(recs))
    (c0, _), (c1, _), (c2, _) = bairef.members(bz)[0]
    bai = bairef.build(bz, 0, 1)
    contigs, n_no_coor = bairef.parse(bai)
    bins, io = contigs[0]
    assert c0 == 0 and n_no_coor == 0 and io == [0, c1 << 16 | 54764]
    assert bins[4681] == [(0, c1 << 16 | 54764), (c2 << 16 | 19484, c2 << 16 | 49484)]
    assert bins[585] == [(c1 << 16 | 54764, c2 << 16 | 19484)]
    assert bins[37450] == [(0, c2 << 16 | 49484), (2, 5)] and sorted(bins) == [585, 4681, 37450]
    assert bairef.query(bai, bz, 0, 0, 10, 11) == [0, 30000, 60000, c1 << 16 | 24720, c1 << 16 | 54720, c1 << 16 | 54764, c2 << 16 | 19484]
    assert bairef.query(bai, bz, 0, 0, 16384, 16385) == [c1 << 16 | 54764]
    # the last record ends with the stream, in a member that is not full: its end is a place in that member
    assert len(b"".join(recs)) == 180044 == 2 * 65280 + 49484


def test_reg2bins_holds_reg2bin():
    rng = random.Random(5)
    for _ in range(2000):
        beg = rng.randrange(0, 1 << 29)
        end = min(1 << 29, beg + 1 + rng.choice([0, 5, 20000, 200000, 3 << 20, 1 << 27]))
        assert bairef.reg2bin(beg, end) in bairef.reg2bins(beg, end)
        assert bairef.reg2bin(beg, end) in bairef.reg2bins(beg + (end - beg) // 2, beg + (end - beg) // 2 + 1)
    assert bairef.reg2bin(0, 1 << 29) == 0 and bairef.reg2bin(16383, 16385) == 585 and bairef.reg2bin(16384, 16385) == 4682


def _random_file(rng, n, n_ref, big_every):
    """n records in coordinate order over n_ref contigs (some left empty), spans from 1 to a few windows, some unmapped placed, some
    unplaced at the end; every big_every-th record padded to tens of kilobytes so that the stream has many members"""
    recs = []
    for refid in sorted(rng.sample(range(n_ref), max(1, n_ref - 2))):
        pos = sorted(rng.randrange(0, 400000) for _ in range(n // n_ref))
        for k, p in enumerate(pos):
            span = rng.choice([1, 30, 150, 16384, 40000])
            unm = rng.random() < 0.05
            recs.append(bam_record(refid, p, flag=4 if unm else 0, cigar=[] if unm else [(span, M)], name=b"n%d" % k,
                                   pad=rng.randrange(20000, 70000) if k % big_every == 0 else rng.randrange(0, 40)))
    recs += [bam_record(-1, -1, flag=4)] * 3
    return bgzf_write(b"".join(recs))


def test_query_against_a_scan_over_all_records():
    rng = random.Random(11)
    n_regions = 0
    for n, n_ref, big_every, base in ((300, 5, 7, 0), (500, 3, 40, (1 << 33) + 12345), (40, 4, 1, 77)):
        bz = _random_file(rng, n, n_ref, big_every)
        assert len(bairef.members(bz)[0]) >= 4
        bai = bairef.build(bz, base, n_ref)
        for _ in range(120):
            refid = rng.randrange(n_ref)
            beg = rng.choice([0, 16383, 16384, 16385, rng.randrange(0, 450000), rng.randrange(0, 450000)])
            end = beg + rng.choice([1, 2, 100, 16384, 100000, 1 << 20])
            assert bairef.query(bai, bz, base, refid, beg, end) == bairef.brute_force(bz, base, refid, beg, end), (n, refid, beg, end)
            n_regions += 1
        # far behind every record: a window the linear index does not have
        assert bairef.query(bai, bz, base, 0, 1 << 28, (1 << 28) + 5) == []
    assert n_regions >= 300
