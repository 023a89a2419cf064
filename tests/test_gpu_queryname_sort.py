"""elp_sort_queryname (-m gpu): By(QNAMELess).ParallelStableSort (sam/filter-pipeline.go:118-122, sam/sam-types.go:475-481) on the device.

The expected order is computed here, not by the oracle: `sorted(range(n), key=(state != 0, QNAME bytes))` - Python's bytes order is
Go's string order (unsigned bytes, a proper prefix first) and `sorted` is stable, so ties keep staging order and the records that are
not output (sr-tagged copies, records rejected by elp_filter_records) follow the others in their own QNAME order."""
import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import NIL16, Batch, batch_from_records
from elprep_amd.engine import BqsrTables, ElpError, Engine
from tests.common import dataset
from tools import synth

pytestmark = pytest.mark.gpu

ELP_ERR_UNSUPPORTED = -5
MAX_QNAME = 1000


def _names(b):
    q = b.qname.tobytes()
    off = b.qname_off.tolist()
    return [q[off[i]:off[i + 1]] for i in range(b.n)]


def _want(b, state=None):
    state = b.has_sr if state is None else state
    names = _names(b)
    out = np.asarray(sorted(range(b.n), key=lambda i: (state[i] != 0, names[i])), dtype=np.uint32)
    return out, int((state == 0).sum())


def _names_batch(names, has_sr=None):
    """unmapped records with the given QNAMEs and nothing else"""
    n = len(names)
    z32 = np.zeros(n, np.int32)
    qo = np.zeros(n + 1, np.uint64)
    qo[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    zo = np.zeros(n + 1, np.uint64)
    return Batch(refid=np.full(n, -1, np.int32), pos=z32, next_refid=np.full(n, -1, np.int32), pnext=z32, tlen=z32,
                 flag=np.full(n, 4, np.uint16), mapq=np.zeros(n, np.uint8), rgid=np.full(n, NIL16, np.uint16),
                 has_sr=np.zeros(n, np.uint8) if has_sr is None else np.asarray(has_sr, np.uint8), l_seq=np.zeros(n, np.uint32),
                 qname_off=qo, qname=np.frombuffer(b"".join(names), np.uint8), cigar_off=zo, cigar=np.zeros(0, np.uint32),
                 seq_off=zo, seq4=np.zeros(0, np.uint8), qual_off=zo, qual=np.zeros(0, np.uint8))


def _stage_in_parts(e, b, parts):
    cuts = np.linspace(0, b.n, parts + 1).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        e.stage(b.take(np.arange(lo, hi)))


def _check(b, h, parts=1, flat=False):
    want, n_out = _want(b)
    e = Engine(h, 0, flat_abi=flat)
    _stage_in_parts(e, b, parts)
    got = e.sort_queryname()
    assert e.n_sorted == n_out
    e.close()
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("first difference at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]])) if bad.size else None


# ---- 1. synthetic reads, as staged and shuffled
@pytest.mark.parametrize("pairs,seed,pfrag", [(40, 0, 0.0), (3000, 1, 0.05), (3000, 7, 0.3), (60_000, 2, 0.02), (200_000, 3, 0.01)])
@pytest.mark.parametrize("shuffled", [False, True])
def test_queryname_order_of_synthetic_reads(pairs, seed, pfrag, shuffled):
    cfg, b, h, _, _ = dataset("tiny", pairs, seed, pfrag)
    if shuffled:
        b = b.take(np.random.default_rng(seed).permutation(b.n))
    _check(b, h, parts=3)


# ---- 2. hand-made names, through elp_stage and elp_stage_columns
HAND = [b"b", b"a0", b"a", b"a00", b"a", b"", b"\xff", b"\x80x", b"a\x7f", b"a\x00", b"a\x00\x00", b"a\x00", b"\x00", b"Z", b"z", b"",
        b"A" * MAX_QNAME, b"A" * (MAX_QNAME - 1) + b"B", b"A" * (MAX_QNAME - 1), b"A" * (MAX_QNAME - 1) + b"\x00", b"A" * MAX_QNAME, b"0", b"9"]


@pytest.mark.parametrize("flat", [False, True])
def test_queryname_order_of_hand_made_names(flat):
    """prefix chains, one-byte names, names of MAX_QNAME bytes, bytes >= 0x80, the empty name and NUL bytes inside a name (staging
    accepts all of them; Go orders "a" < "a\\x00" < "a\\x00\\x00" < "a0")"""
    h = synth.config("tiny").header()
    recs = [dict(qname=q, flag=4, has_sr=(i % 7 == 3)) for i, q in enumerate(HAND)]
    b = batch_from_records(recs)
    assert b.has_sr.any()
    _check(b, h, flat=flat)
    # the same names many times over (groups of equal keys, and the whole set behind the comparison cap)
    rng = np.random.default_rng(1)
    b = _names_batch([HAND[k] for k in rng.integers(0, len(HAND), 5000)], has_sr=rng.random(5000) < 0.1)
    _check(b, h, parts=2, flat=flat)


def test_queryname_sort_rejects_a_name_over_the_limit():
    h = synth.config("tiny").header()
    e = Engine(h)
    with pytest.raises(ElpError) as ei:
        e.stage(_names_batch([b"a", b"x" * (MAX_QNAME + 1)]))
    assert ei.value.code == ELP_ERR_UNSUPPORTED
    e.close()


# ---- 3. adversarial sets of >= 2^20 records
N_BIG = (1 << 20) + 3


def _adversarial(kind, rng):
    if kind == "all_equal":
        return [b"SAME:NAME:1"] * N_BIG
    if kind == "long_prefix":
        pre = b"P" * 200
        tails = rng.integers(0, 10, (N_BIG, 12)) + ord("0")
        lens = rng.integers(1, 13, N_BIG)
        return [pre + bytes(tails[i, :lens[i]].astype(np.uint8)) for i in range(N_BIG)]
    if kind == "last_byte":
        pre = b"Q" * 63
        last = rng.integers(0, 256, N_BIG).astype(np.uint8)
        return [pre + bytes([int(v)]) for v in last]
    if kind == "last_byte_of_1000":
        pre = b"R" * (MAX_QNAME - 1)
        return [pre + bytes([int(v)]) for v in rng.integers(0, 256, 20_000)]
    if kind == "illumina":
        out = []
        tiles = rng.integers(1101, 2679, N_BIG // 2 + 2)
        xs, ys = rng.integers(1, 40_000, N_BIG // 2 + 2), rng.integers(1, 40_000, N_BIG // 2 + 2)
        lanes = rng.integers(1, 5, N_BIG // 2 + 2)
        for k in range(N_BIG // 2 + 2):
            name = b"A00123:45:HXXXXXXX:%d:%d:%d:%d" % (lanes[k], tiles[k], xs[k], ys[k])
            out += [name, name]  # the two mates
        out = out[:N_BIG]
        return [out[i] for i in rng.permutation(N_BIG)]
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["all_equal", "long_prefix", "last_byte", "last_byte_of_1000", "illumina"])
def test_queryname_order_of_adversarial_name_sets(kind):
    """all names equal (staging order), a 200-byte shared prefix with a 1-12 byte tail, names that differ in their last byte only (64 and
    1000 bytes: groups of thousands of equal names, behind the comparison cap), Illumina names with x / y fields of varying width"""
    rng = np.random.default_rng(11)
    names = _adversarial(kind, rng)
    sr = rng.random(len(names)) < 0.03
    b = _names_batch(names, has_sr=sr)
    _check(b, synth.config("tiny").header(), parts=2)


# ---- 4. records that are not output: sr-tagged copies and elp_filter_records rejections
@pytest.mark.parametrize("seed", [0, 5])
def test_queryname_order_puts_sr_copies_and_filtered_records_behind(seed):
    from elprep_amd import sfm
    from oracle import simple_filters as sf
    cfg, b, h, _, _ = dataset("tiny", 3000, seed, 0.05)
    b = sfm.with_sr(b, np.arange(b.n) % 13 == 4)
    keep = sf.keep_mask(b, min_mapq=30)
    state = ((b.has_sr != 0) | ~keep).astype(np.uint8)
    assert 0 < (state == 0).sum() < b.n and (b.has_sr != 0).any() and (~keep & (b.has_sr == 0)).any()
    want, n_out = _want(b, state)
    e = Engine(h)
    _stage_in_parts(e, b, 2)
    e.filter_records(min_mapq=30)
    assert e.n_sorted == n_out
    got = e.sort_queryname()
    e.close()
    assert np.array_equal(got[:n_out], want[:n_out]), "output order"
    assert np.array_equal(got[n_out:], want[n_out:]), "order of the records behind"


# ---- 5. edge sizes
@pytest.mark.parametrize("n", [0, 1, 2])
def test_queryname_sort_of_zero_one_and_two_records(n):
    h = synth.config("tiny").header()
    e = Engine(h)
    if n:
        e.stage(_names_batch([b"r2", b"r1"][2 - n:]))
    got = e.sort_queryname()
    e.close()
    assert got.tolist() == [[], [0], [1, 0]][n]


# ---- 6. emit after a queryname sort
def _bam_split(stream):
    out, p = [], 0
    while p < len(stream):
        size = 4 + int(np.frombuffer(stream[p:p + 4], np.uint32)[0])
        out.append(stream[p:p + size])
        p += size
    return out


def _members(bz):
    import struct
    import zlib
    out, p = [], 0
    while p < len(bz):
        assert bz[p:p + 4] == b"\x1f\x8b\x08\x04"
        bsize = struct.unpack_from("<H", bz, p + 16)[0] + 1
        out.append(zlib.decompress(bz[p:p + bsize], wbits=31))
        p += bsize
    return b"".join(out)


def test_emit_sorted_bam_and_bgzf_after_a_queryname_sort():
    """the BAM records of a queryname-sorted context are the input's records (as the coordinate-sorted emission of the same context gives
    them) in the queryname permutation, byte for byte; the BGZF form inflates to the same bytes"""
    from elprep_amd import sfm
    cfg, b, h, _, _ = dataset("tiny", 3000, 4, 0.03)
    b = sfm.with_sr(b, np.arange(b.n) % 41 == 7)
    raw, rec_off = synth.bam_records(b, h.rg_ids)
    e = Engine(h)
    e.set_read_group_ids(h.rg_ids)
    e.stage_bam(raw, rec_off=rec_off)
    cperm = e.sort_coordinate()
    n_out = e.n_sorted
    recs = _bam_split(e.emit_sorted_bam().tobytes())
    assert len(recs) == n_out
    by_index = {int(cperm[k]): recs[k] for k in range(n_out)}
    qperm = e.sort_queryname()
    want, want_n = _want(b)
    assert want_n == n_out and np.array_equal(qperm, want)
    got = e.emit_sorted_bam().tobytes()
    assert got == b"".join(by_index[int(i)] for i in qperm[:n_out])
    assert _members(e.emit_sorted_bgzf().tobytes()) == got
    e.close()


# ---- 7. merging refuses queryname permutations (cmd/merge.go:175-176)
def test_merge_refuses_a_queryname_sorted_context():
    cfg, b, h, _, _ = dataset("tiny", 500, 1, 0.0)
    raw, rec_off = synth.bam_records(b, h.rg_ids)
    eg, es = Engine(h), Engine(h)
    for e in (eg, es):
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw, rec_off=rec_off)
    eg.sort_coordinate()
    es.sort_queryname()
    for groups, spread in ((eg, es), (es, eg)):
        for call in (groups.merge_spread, groups.emit_merged_bam):
            with pytest.raises(ElpError) as ei:
                call(spread)
            assert ei.value.code == ELP_ERR_UNSUPPORTED and "queryname" in str(ei.value)
    es.sort_coordinate()  # a coordinate permutation again: the merge runs
    eg.merge_spread(es)
    eg.close()
    es.close()


# ---- 8. switching orders on one context
@pytest.mark.parametrize("ahead", [False, True])
def test_coordinate_then_queryname_then_coordinate(ahead):
    cfg, b, h, _, _ = dataset("tiny", 4000, 6, 0.04)
    oflags = orc.mark_duplicates(b, h)
    operm = orc.sort_coordinate(b, oflags)
    want, _ = _want(b)
    e = Engine(h)
    _stage_in_parts(e, b, 3)
    e.snapshot()
    e.sort_ahead(ahead)
    for rnd in range(3):
        e.rollback()
        e.mark_duplicates(True, fetch=False)  # (ahead: the coordinate key passes are queued on the sort lane here)
        if rnd == 1:
            assert np.array_equal(e.sort_queryname(), want), ("queryname before coordinate", rnd)
        assert np.array_equal(e.sort_coordinate(), operm), ("coordinate", rnd)
        assert np.array_equal(e.sort_queryname(), want), ("queryname", rnd)
        assert np.array_equal(e.sort_coordinate(), operm), ("coordinate again", rnd)
        assert np.array_equal(e.flags(), oflags), ("flags", rnd)
    e.close()


# ---- 9. on its own thread, while the metrics pass and gather -> finalize -> apply run on the same context
@pytest.mark.parametrize("pairs,seed,pfrag", [(3000, 0, 0.05), (40_000, 3, 0.02)])
def test_queryname_sort_metrics_and_the_bqsr_chain_at_once(pairs, seed, pfrag):
    from concurrent.futures import ThreadPoolExecutor
    cfg = synth.config("tiny", seed)
    cfg.p_frag = pfrag
    b = synth.generate(cfg, 0, pairs)
    h = cfg.header()
    refs = [synth.reference(cfg, r) for r in range(h.n_ref)]
    sites = [orc.flatten(orc.sort_by_start(synth.known_sites_raw(cfg, r))) for r in range(h.n_ref)]
    oflags = orc.mark_duplicates(b, h)
    operm = orc.sort_coordinate(b, oflags)
    _, octr, _ = orc.dup_metrics(b, h, operm, 100)
    oq, oc, ox = orc.bqsr_gather(b, h, orc.BqsrRef(refs, sites), oflags, 500)
    oqual = orc.BqsrFinal(oq, oc, ox, 500).apply(b, h, 0)
    want, _ = _want(b)
    e = Engine(h, 0)
    _stage_in_parts(e, b, 3)
    for r in range(h.n_ref):
        e.set_reference(r, refs[r])
        e.set_known_sites(r, sites[r])
    e.snapshot()
    with ThreadPoolExecutor(1) as sort_pool, ThreadPoolExecutor(1) as mx_pool:
        for rnd in range(3):
            e.rollback()
            e.mark_duplicates(True, fetch=False)
            st = sort_pool.submit(e.sort_queryname)
            mx = mx_pool.submit(e.dup_metrics, 100)
            qt, ct, xt = e.recalibrate(500)
            lut, present = BqsrTables(qt, ct, xt, 500).finalize().build_lut(0)
            qual = e.apply_bqsr(lut, present, 500)
            perm, ctr = st.result(), mx.result()
            assert np.array_equal(e.flags(), oflags), ("flags", rnd)
            assert np.array_equal(perm, want), ("order", rnd)
            assert np.array_equal(ctr, octr), ("counters", rnd)
            assert np.array_equal(qt, oq) and np.array_equal(ct, oc) and np.array_equal(xt, ox), ("tables", rnd)
            assert np.array_equal(qual, oqual), ("qualities", rnd)
    e.close()
