"""The radix scatter kernel (k_radix_scatter_t, csrc/radix.hip) at the seams of its three forms, through the entries that use it:
sort_coordinate (the fused key << bits | index form), mark_duplicates (the pair list: pairs with values, a device-side length below the
launch's upper bound, the last pass's bucket bounds), dup_metrics and the queryname sort (pairs with identity values).  The tuning key
radix_tile = 1 / 2 / 3 pins the 4096- / 8192- / 16384-key form, so every form runs on small input.

Read counts: 1, 63, 64, 65 (the lanes of one wave) and tile - 1, tile, tile + 1, 3 tiles + 1 of the pinned form (a tile that is exactly
full takes the kernel's full-tile path, one key more adds a second tile with one valid lane, one key less leaves one invalid lane).

Key shapes: every read at one coordinate (every digit bit is the same in every lane; the expected result is the input order: the stability
of the passes), two coordinates that differ in one bit of the key - that bit placed lowest and highest in each digit of the sort's key -,
all reads unmapped, random reads.  Everything is compared with the oracle bit for bit, the queryname order with Python's stable sort of
the names (as tests/test_gpu_queryname_sort.py does)."""
import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch, Header
from elprep_amd.engine import Engine
from tests.common import dataset

pytestmark = pytest.mark.gpu

TILES = {1: 4096, 2: 8192, 3: 16384}
L_SEQ = 10
# the coordinate key is (contig code, POS, strand) from the top: POS bit k is key bit k + 1, the strand bit is key bit 0.  With POS_BASE
# the key has 32 live bits (four digits); lowest / highest bit of digit d = key bit 8 d / 8 d + 7
POS_BASE = 1 << 28
POS_BITS = (0, 6, 7, 14, 15, 22, 23, 27)  # key bits 1, 7 | 8, 15 | 16, 23 | 24, 28
REF_LEN = (1 << 30)


def _counts(rt):
    t = TILES[rt]
    return (1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 1)


def _header(n_ref=2):
    return Header(ref_len=np.full(n_ref, REF_LEN, np.int32), rg_lib=np.array([0], np.uint16), rg_cov=np.array([0], np.uint16))


def _reads(refid, pos, flag, names=None):
    """single-end reads (10M, quality 30) at the given coordinates; names: (n, w) bytes, default one name for all"""
    refid = np.asarray(refid, np.int32)
    n = refid.shape[0]
    if names is None:
        names = np.tile(np.frombuffer(b"same", np.uint8), (n, 1))
    w = names.shape[1]
    mapped = (np.asarray(flag, np.uint16) & 4) == 0
    off = lambda per: np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    return Batch(refid=refid, pos=np.asarray(pos, np.int32), next_refid=np.full(n, -1, np.int32), pnext=np.zeros(n, np.int32),
                 tlen=np.zeros(n, np.int32), flag=np.asarray(flag, np.uint16), mapq=np.full(n, 60, np.uint8), rgid=np.zeros(n, np.uint16),
                 has_sr=np.zeros(n, np.uint8), l_seq=np.full(n, L_SEQ, np.uint32), qname_off=off(np.full(n, w)),
                 qname=np.ascontiguousarray(names, np.uint8).reshape(-1), cigar_off=off(mapped.astype(np.int64)),
                 cigar=np.full(int(mapped.sum()), (L_SEQ << 4) | 0, np.uint32), seq_off=off(np.full(n, L_SEQ // 2)),
                 seq4=np.full(n * (L_SEQ // 2), 0x11, np.uint8), qual_off=off(np.full(n, L_SEQ)), qual=np.full(n * L_SEQ, 30, np.uint8))


def _names(b):
    q = b.qname.tobytes()
    off = b.qname_off.tolist()
    return [q[off[i]:off[i + 1]] for i in range(b.n)]


def _engine(b, h, rt, **tuning):
    e = Engine(h, tuning=dict(tuning, radix_tile=rt))
    e.stage(b)
    return e


def _check_all(b, h, rt, where, identity=False, queryname=True, **tuning):
    """mark duplicates, coordinate sort (which sees the duplicate bits), metrics, then the queryname sort of the same context"""
    e = _engine(b, h, rt, **tuning)
    try:
        oflags = orc.mark_duplicates(b, h)
        flags = e.mark_duplicates(True)
        assert np.array_equal(flags, oflags), (where, np.nonzero(flags != oflags)[0][:8].tolist())
        operm = orc.sort_coordinate(b, oflags)
        perm = e.sort_coordinate()
        assert np.array_equal(perm, operm), (where, np.nonzero(perm != operm)[0][:8].tolist())
        _, octr, _ = orc.dup_metrics(b, h, operm, 100)
        assert np.array_equal(e.dup_metrics(100), octr), where
        if queryname:
            names = _names(b)
            want = np.asarray(sorted(range(b.n), key=lambda i: names[i]), dtype=np.uint32)
            got = e.sort_queryname()
            assert np.array_equal(got, want), (where, np.nonzero(got != want)[0][:8].tolist())
            if identity:
                assert np.array_equal(got, np.arange(b.n, dtype=np.uint32)), where
    finally:
        e.set_tuning("radix_tile", 0)
        e.close()
    return flags, perm


@pytest.mark.parametrize("rt", [1, 2, 3])
def test_every_read_at_one_coordinate(rt):
    """every digit bit is wave-uniform in every pass; identical records: the permutation is the input order (stable passes, and a
    tie-break that finds nothing to break)"""
    h = _header()
    for n in _counts(rt):
        b = _reads(np.zeros(n), np.full(n, POS_BASE + 12345), np.zeros(n))
        ident = np.arange(n, dtype=np.uint32)
        e = _engine(b, h, rt)
        try:  # in front of mark duplicates the records are identical, flags included: the order is the input's
            assert np.array_equal(orc.sort_coordinate(b), ident)
            assert np.array_equal(e.sort_coordinate(), ident), (rt, n)
        finally:
            e.set_tuning("radix_tile", 0)
            e.close()
        # behind it the one record that is no duplicate sorts by its flags; the names are still one: queryname order = input order
        flags, _ = _check_all(b, h, rt, ("one coordinate", rt, n), identity=True)
        assert int(((flags & 0x400) != 0).sum()) == n - 1


@pytest.mark.parametrize("rt", [1, 2, 3])
def test_two_coordinates_that_differ_in_one_bit(rt):
    """the one live bit of the keys lowest and highest in each digit: POS bits, the strand bit (key bit 0) and the contig (top digit);
    distinct names, so the order inside a coordinate is by QNAME and the queryname sort has live digits of its own"""
    h = _header()
    rng = np.random.default_rng(rt)
    variants = [("pos", k) for k in POS_BITS] + [("strand", 0), ("contig", 0)]
    for n in _counts(rt):
        which = rng.integers(0, 2, n)
        names = np.frombuffer(b"".join(b"%05x" % v for v in rng.permutation(n).tolist()), np.uint8).reshape(n, 5)
        for kind, k in variants:
            refid, pos, flag = np.zeros(n, np.int64), np.full(n, POS_BASE + 5), np.zeros(n, np.int64)
            if kind == "pos":
                pos = pos ^ (which << k)
            elif kind == "strand":
                flag = which * 16
            else:
                refid = which
            b = _reads(refid, pos, flag, names)
            e = _engine(b, h, rt)
            try:
                perm, operm = e.sort_coordinate(), orc.sort_coordinate(b)
                assert np.array_equal(perm, operm), (kind, k, rt, n, np.nonzero(perm != operm)[0][:8].tolist())
            finally:
                e.set_tuning("radix_tile", 0)
                e.close()


@pytest.mark.parametrize("rt", [1, 2, 3])
def test_all_reads_unmapped(rt):
    h = _header()
    rng = np.random.default_rng(10 + rt)
    for n in _counts(rt):
        names = rng.integers(ord("a"), ord("e"), (n, 6)).astype(np.uint8)  # many equal names: ties keep staging order
        b = _reads(np.full(n, -1), np.zeros(n), np.full(n, 4), names)
        _check_all(b, h, rt, ("unmapped", rt, n))


@pytest.mark.parametrize("rt", [1, 2, 3])
def test_random_reads(rt):
    """synthetic pairs and fragments with duplicates and optical duplicates, cut at the seams (a cut pair leaves a lone mate)"""
    t = TILES[rt]
    cfg, b0, h, _, _ = dataset("tiny", (3 * t + 1) * 11 // 20 + 10, 4, 0.05)  # (a fragment is one read, a pair two)
    assert b0.n >= 3 * t + 1
    for n in _counts(rt):
        _check_all(b0.take(np.arange(n)), h, rt, ("random", rt, n))


@pytest.mark.parametrize("rt", [1, 2, 3])
def test_pair_list_far_shorter_than_its_upper_bound(rt):
    """few pairs among many single-end reads: the pair list's passes are launched over the upper bound of its length (every read), its
    device-side length is a handful - the tiles behind the end leave at once and nobody looks back at them"""
    t = TILES[rt]
    cfg, bp, h, _, _ = dataset("tiny", 40, 5, 0.0)
    rng = np.random.default_rng(20 + rt)
    n = 3 * t + 1
    frag = _reads(rng.integers(0, h.n_ref, n), rng.integers(1, 2000, n), rng.integers(0, 2, n) * 16,
                  np.frombuffer(b"".join(b"f%05x" % v for v in range(n)), np.uint8).reshape(n, 6))
    b = Batch.concat([frag.take(np.arange(0, n // 2)), bp, frag.take(np.arange(n // 2, n))])
    b = b.take(rng.permutation(b.n))  # mates apart: the pairs form in the table and go through the list
    flags, _ = _check_all(b, h, rt, ("short pair list", rt), queryname=False, mate_path=2)
    assert ((flags & 0x400) != 0).any()


@pytest.mark.parametrize("rt", [1, 2, 3])
def test_pair_list_bucket_bounds_over_more_than_one_tile(rt):
    """every pair through the table (mate_path = 2, mates apart): a pair list of more than one tile, whose last pass reports the buckets'
    bounds (RadixBounds) - a bucket that straddles two tiles gets its start from one workgroup and its end from another"""
    t = TILES[rt]
    pairs = t + t // 2 + 7
    cfg, b, h, _, _ = dataset("tiny", pairs, 6, 0.02)
    b = b.take(np.random.default_rng(30 + rt).permutation(b.n))
    flags, _ = _check_all(b, h, rt, ("bucket bounds", rt), queryname=False, mate_path=2)
    assert ((flags & 0x400) != 0).sum() > 10
