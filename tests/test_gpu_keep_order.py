"""elp_order_keep, the merges that take its permutations, and the BGZF forms of the merged streams (-m gpu).

`--sorting-order keep / unknown / unsorted` and a requested `coordinate` on an input that is sorted already write the records in the
order they came (sam/filter-pipeline.go:110-124, :208-225).  The expected orders are the numpy restatements of tests/keep_ref.py and
sfm.merge_splits / sfm.merge_splits_unsorted on Batch payloads; the expected bytes are the oracle's BAM encoder on the records in that
order.  Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from elprep_amd import sfm
from elprep_amd.batch import NIL16, Batch, Header
from elprep_amd.engine import BqsrTables, ElpError, Engine
from tests import keep_ref, tagref
from tests.common import dataset
from tests.keep_ref import KEEP_W, MERGE_CHECK_W, SCAN_TILE
from tests.test_gpu_round4 import _members
from tools import synth

pytestmark = pytest.mark.gpu

ELP_ERR_ARG, ELP_ERR_DATA, ELP_ERR_UNSUPPORTED = -1, -4, -5
W = KEEP_W  # records per workgroup of the partition kernels (tests/test_keep_order_cpu.py checks the constants against the sources)
# the tiles' counts are scanned by exclusive_scan_u32, SCAN_TILE counts per workgroup: with more than SCAN_TILE tiles - more than
# SCAN_TILE * W = 2^20 records - the scan runs a second level.  N_BIG has SCAN_TILE + 3 tiles, the last one partly filled.
N_BIG = SCAN_TILE * W + 2 * W + 5
assert N_BIG <= 1 << 21 and -(-N_BIG // W) > SCAN_TILE


def _tiny_header():
    return synth.config("tiny").header()


def _one_base_batch(has_sr, mapq, split=None):
    """unmapped records of one base each with the given record states-to-be: has_sr as staged, MAPQ for elp_filter_records to reject by"""
    n = len(has_sr)
    z32 = np.zeros(n, np.int32)
    one = np.arange(n + 1, dtype=np.uint64)
    return Batch(refid=np.full(n, -1, np.int32), pos=z32, next_refid=np.full(n, -1, np.int32), pnext=z32, tlen=z32,
                 flag=np.full(n, 4, np.uint16), mapq=np.asarray(mapq, np.uint8), rgid=np.full(n, NIL16, np.uint16),
                 has_sr=np.asarray(has_sr, np.uint8), l_seq=np.ones(n, np.uint32), qname_off=one, qname=np.full(n, ord("r"), np.uint8),
                 cigar_off=np.zeros(n + 1, np.uint64), cigar=np.zeros(0, np.uint32), seq_off=one, seq4=np.full(n, 0x10, np.uint8),
                 qual_off=one, qual=np.full(n, 30, np.uint8), split=None if split is None else np.asarray(split, np.uint16))


def _state(has_sr, mapq):
    """the record states behind elp_filter_records(min_mapq=1)"""
    return np.where(np.asarray(mapq) < 1, 2, np.asarray(has_sr)).astype(np.uint8)


def _patterns(n):
    """(name, has_sr, mapq) for n records"""
    z, hi = np.zeros(n, np.uint8), np.full(n, 60, np.uint8)
    yield "all output", z, hi
    yield "all sr", np.ones(n, np.uint8), hi
    yield "all rejected", z, z
    yield "alternating", (np.arange(n) % 2).astype(np.uint8), hi
    yield "alternating, output second", ((np.arange(n) + 1) % 2).astype(np.uint8), hi
    for p in sorted({0, n - 1, W - 1, W}):  # one output record: first, last, either side of a workgroup boundary
        if 0 <= p < n:
            sr = (np.arange(n) % 3 != 0).astype(np.uint8)   # the others: sr-tagged copies and rejected records mixed
            mq = np.where(np.arange(n) % 3 == 0, 0, 60).astype(np.uint8)
            sr[p], mq[p] = 0, 60
            yield "one output record at %d" % p, sr, mq
    rng = np.random.default_rng(1000 + n)
    kind = rng.choice(4, n, p=[0.5, 0.25, 0.15, 0.1])      # output, sr, rejected, sr and rejected
    yield "random mix", np.isin(kind, (1, 3)).astype(np.uint8), np.where(np.isin(kind, (2, 3)), 0, 60).astype(np.uint8)


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, "first difference at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


# ---- 1. by_split = 0 at the seams of the partition kernels
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, W - 1, W, W + 1, 3 * W + 17, N_BIG])
def test_keep_order_at_the_partition_seams(n):
    e = Engine(_tiny_header())
    try:
        for name, sr, mq in _patterns(n):
            e.reset()
            if n:
                e.stage(_one_base_batch(sr, mq))
            e.filter_records(min_mapq=1)
            want, n_out = keep_ref.keep_order(_state(sr, mq))
            got = e.order_keep()
            assert e.n_sorted == n_out, name
            _same(got, want, name)
            if n and n <= 3 * W + 17:  # every split id 0: the same path, and the same order
                _same(e.order_keep(by_split=True), want, name + ", by split")
    finally:
        e.close()


# ---- 2. by_split = 1
def _split_cases(max_split, n, rng):
    if max_split == 0:
        yield "all zero", np.zeros(n, np.uint16)
        return
    ids = np.unique(np.concatenate([[0, max_split], rng.integers(0, max_split + 1, 6)]))  # a few ids, empty ones in between
    yield "a few ids", rng.choice(ids, n).astype(np.uint16)
    yield "one id", np.full(n, max_split, np.uint16)
    yield "ids descending", np.sort(rng.integers(0, max_split + 1, n))[::-1].astype(np.uint16)
    if max_split >= 255:
        yield "every id", (np.arange(n) * 7919 % (max_split + 1)).astype(np.uint16)[::-1]


@pytest.mark.parametrize("max_split", [0, 1, 255, 256, 65535])
def test_keep_order_by_split(max_split):
    """max_split 1: keys of two bits; 255 / 256: nine and ten bits, two radix passes; 65535: seventeen bits, three passes"""
    n = 2 * 4096 + 77  # (three radix tiles)
    rng = np.random.default_rng(max_split)
    e = Engine(_tiny_header())
    try:
        for name, split in _split_cases(max_split, n, rng):
            kind = rng.choice(3, n, p=[0.6, 0.25, 0.15])
            sr, mq = (kind == 1).astype(np.uint8), np.where(kind == 2, 0, 60).astype(np.uint8)
            e.reset()
            cut = n // 3
            e.stage(_one_base_batch(sr[:cut], mq[:cut], split[:cut]))
            e.stage(_one_base_batch(sr[cut:], mq[cut:], split[cut:]))
            e.filter_records(min_mapq=1)
            state = _state(sr, mq)
            want, n_out = keep_ref.keep_order(state, split, by_split=True)
            got = e.order_keep(by_split=True)
            assert e.n_sorted == n_out, name
            _same(got, want, name)
            _same(e.order_keep(), keep_ref.keep_order(state)[0], name + ", plain behind it")
    finally:
        e.close()


@pytest.mark.parametrize("n", [0, 1])
def test_keep_order_by_split_of_zero_and_one_record(n):
    e = Engine(_tiny_header())
    if n:
        e.stage(_one_base_batch([0], [60], [9]))
    assert e.order_keep(by_split=True).tolist() == list(range(n)) and e.n_sorted == n
    e.close()


# ---- 3. what the feature is for: a file sorted by (refid, POS) alone goes out as it came
def _by_position(b, names_descending=False):
    """staging order of `b` sorted by (refid with -1 last, POS) as samtools sorts; ties in staging order, or by QNAME descending"""
    ref = np.where(b.refid < 0, 1 << 30, b.refid).astype(np.int64)
    if not names_descending:
        return np.lexsort((b.pos, ref))
    names = [b.qname_of(i) for i in range(b.n)]
    rank = np.empty(b.n, np.int64)
    rank[np.asarray(sorted(range(b.n), key=lambda i: names[i]), np.int64)] = np.arange(b.n)
    return np.lexsort((-rank, b.pos, ref))


def _expected(b, rg_ids, order, flags=None, qual=None):
    return tagref.records(orc.bam_encode(b, rg_ids, order=np.asarray(order, np.uint32), flags=flags, qual=qual, normalize_tags=True).tobytes())


def _one_group_header(h, rg_id="new"):
    return Header.from_read_groups(h.ref_names, h.ref_len, [{"ID": rg_id, "LB": "libN", "PU": "FC9.1"}])


@pytest.mark.parametrize("option", ["plain", "tag_filter", "replace_read_group"])
def test_sorted_input_goes_out_in_input_order(option):
    cfg, b0, h, _, _ = dataset("tiny", 1500, 21, 0.03)
    b0 = sfm.with_sr(b0, np.arange(b0.n) % 37 == 5)
    b = b0.take(_by_position(b0, names_descending=True))
    # pairs of neighbours equal in refid, POS and strand whose QNAMEs descend: CoordinateLess puts the smaller name first
    same = (b.refid[1:] == b.refid[:-1]) & (b.pos[1:] == b.pos[:-1]) & ((b.flag[1:] & 16) == (b.flag[:-1] & 16)) & (b.has_sr[1:] == 0) & (b.has_sr[:-1] == 0)
    desc = np.asarray([b.qname_of(i) > b.qname_of(i + 1) for i in range(b.n - 1)])
    assert (same & desc).sum() > 20
    out_idx = np.flatnonzero(b.has_sr == 0)
    raw = orc.bam_encode(b, h.rg_ids)
    hdr = _one_group_header(h) if option == "replace_read_group" else h
    want = _expected(b, h.rg_ids, out_idx)
    f = dict(remove=["AS", "XT"], keep=["NM", "RG", "AS", "MD"])
    if option == "replace_read_group":
        want = [tagref.replace_read_group(r, "new") for r in want]
    if option == "tag_filter":
        want = [tagref.apply_tag_filter(r, **f) for r in want]
    want = b"".join(want)
    e = Engine(hdr)
    try:
        if option == "replace_read_group":
            e.set_replace_read_group("new")
        else:
            e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw)
        if option == "tag_filter":
            e.set_tag_filter(**f)
        perm = e.order_keep()
        _same(perm, keep_ref.keep_order(b.has_sr)[0], "permutation")
        assert e.n_sorted == out_idx.size
        for per_pass in (0, 211, 1000):
            e.set_tuning("emit_pass", per_pass)
            assert e.emit_sorted_bam().tobytes() == want, per_pass
            n = C.c_uint64()
            e._check(e.L.elp_emit_sorted_bgzf(e.h, C.c_void_p(0), 0, C.byref(n)))
            bz = e.emit_sorted_bgzf().tobytes()
            mem = _members(bz)
            assert b"".join(m for _, m in mem) == want and int(n.value) >= len(bz), per_pass
            assert len(mem) >= 3 and all(len(m) == 65280 for _, m in mem[:-1])
        e.set_tuning("emit_pass", 0)
        e.sort_coordinate()  # the only call there was in front of an emit: it reorders what the reference leaves alone
        assert e.emit_sorted_bam().tobytes() != want
    finally:
        e.set_tuning("emit_pass", 0)
        e.close()


# ---- 4. the kinds replace each other; what drops a keep permutation
def test_keep_coordinate_keep_queryname_on_one_context():
    cfg, b, h, _, _ = dataset("tiny", 1500, 6, 0.04)
    b = sfm.with_sr(b, np.arange(b.n) % 29 == 3)
    keep, _ = keep_ref.keep_order(b.has_sr)
    n_out = orc.num_sorted(b)
    coord = orc.sort_coordinate(b)[:n_out]  # (the oracle orders the output records only)
    names = [b.qname_of(i) for i in range(b.n)]
    qn = np.asarray(sorted(range(b.n), key=lambda i: (b.has_sr[i] != 0, names[i])), np.uint32)
    e = Engine(h)
    try:
        e.stage(b)
        with pytest.raises(ElpError) as ei:
            e.permutation()
        assert ei.value.code == ELP_ERR_ARG and "elp_order_keep" in str(ei.value)
        _same(e.order_keep(), keep, "keep")
        _same(e.sort_coordinate()[:n_out], coord, "coordinate")
        _same(e.order_keep(), keep, "keep again")
        _same(e.sort_queryname(), qn, "queryname")
        _same(e.order_keep(by_split=True), keep, "keep by split (one split)")
        _same(e.permutation(), keep, "fetched again")
    finally:
        e.close()


def test_what_drops_a_keep_permutation():
    cfg, b, h, _, _ = dataset("tiny", 800, 8, 0.0)
    n_groups, gof = orc.contig_groups(cfg.ref_len, 80000)
    raw = orc.bam_encode(b, h.rg_ids)
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw, split_id=3)
        for by_split in (True, False):
            # elp_filter_records changes the states: either kind goes
            e.order_keep(by_split=by_split)
            e.emit_sorted_bam()
            e.filter_records(min_mapq=0)
            for call in (e.emit_sorted_bam, e.emit_sorted_bgzf, e.permutation):
                with pytest.raises(ElpError) as ei:
                    call()
                assert ei.value.code == ELP_ERR_ARG, (by_split, call)
        # elp_split_classify rewrites the split column: the order made from it goes, the plain one stays
        e.order_keep(by_split=True)
        e.split_classify(gof, n_groups)
        with pytest.raises(ElpError) as ei:
            e.emit_sorted_bam()
        assert ei.value.code == ELP_ERR_ARG
        with pytest.raises(ElpError) as ei:
            e.permutation()
        assert ei.value.code == ELP_ERR_ARG
        want = e.order_keep()
        e.split_classify(gof, n_groups)
        _same(e.permutation(), want, "plain, behind elp_split_classify")
        assert e.emit_sorted_bam().tobytes() == b"".join(_expected(b, h.rg_ids, np.arange(b.n)))
    finally:
        e.close()


# ---- 5. the whole path without a sort
def test_order_keep_metrics_and_the_bqsr_chain_at_once():
    """behind elp_mark_duplicates three host threads at once on one context: elp_order_keep (the sort lane), elp_dup_metrics, and
    gather -> finalize -> apply; two rounds (snapshot / rollback); every output against the oracle, the emitted records = the input in
    input order with the oracle's FLAGs and QUALs"""
    from concurrent.futures import ThreadPoolExecutor
    cfg, b, h, refs, sites = dataset("tiny", 2000, 3, 0.02)
    oflags = orc.mark_duplicates(b, h)
    _, octr, _ = orc.dup_metrics(b, h, orc.sort_coordinate(b, oflags), 100)
    oq, oc, ox = orc.bqsr_gather(b, h, orc.BqsrRef(refs, sites), oflags, 500)
    oqual = orc.BqsrFinal(oq, oc, ox, 500).apply(b, h, 0)
    want = b"".join(_expected(b, h.rg_ids, np.arange(b.n), oflags, oqual))
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(orc.bam_encode(b, h.rg_ids))
        for r in range(h.n_ref):
            e.set_reference(r, refs[r])
            e.set_known_sites(r, sites[r])
        e.snapshot()
        with ThreadPoolExecutor(1) as order_pool, ThreadPoolExecutor(1) as mx_pool:
            for rnd in range(2):
                e.rollback()
                e.mark_duplicates(True, fetch=False)
                st = order_pool.submit(e.order_keep)
                mx = mx_pool.submit(e.dup_metrics, 100)
                qt, ct, xt = e.recalibrate(500)
                lut, present = BqsrTables(qt, ct, xt, 500).finalize().build_lut(0)
                qual = e.apply_bqsr(lut, present, 500)
                perm, ctr = st.result(), mx.result()
                assert np.array_equal(e.flags(), oflags), ("flags", rnd)
                assert np.array_equal(perm, np.arange(b.n, dtype=np.uint32)), ("order", rnd)
                assert np.array_equal(ctr, octr), ("counters", rnd)
                assert np.array_equal(qt, oq) and np.array_equal(ct, oc) and np.array_equal(xt, ox), ("tables", rnd)
                assert np.array_equal(qual, oqual), ("qualities", rnd)
                assert e.emit_sorted_bam().tobytes() == want, ("records", rnd)
    finally:
        e.close()


# ---- 6. the coordinate merge on keep permutations
def _with_col(b, name, values):
    cols = {k: getattr(b, k) for k in b.__dataclass_fields__}
    cols[name] = np.ascontiguousarray(values, dtype=cols[name].dtype)
    return Batch(**cols)


def _with_pos(b, pos):
    return _with_col(b, "pos", pos)


def _with_ids(b):
    """`b` with every record's index in its TLEN column (which no merge reads): the payload restatements of sfm move whole records, and
    the index that comes out says which record of `b` stands where.  The expected bytes are then the oracle's encoding of THOSE records
    of `b` (its encoder derives a record's optional fields from the record's index in the batch it is given)."""
    return _with_col(b, "tlen", np.arange(b.n))


def _sorted_case():
    """a (refid, POS)-sorted read set and its split: (header, batch, group_of_ref, n_groups, split ids, spread mask), with a spread read
    on the position of a group read and one behind the last group read of its contig"""
    from oracle import simple_filters as sf
    cfg, b, h, _, _ = dataset("tiny", 1500, 17, 0.03)
    n_groups, gof = orc.contig_groups(cfg.ref_len, 0)
    split, spread = sf.split_records(b, gof)
    spread = spread.astype(bool)
    pos = b.pos.copy()
    sp0 = np.flatnonzero(spread & (b.refid == 0))
    grp0 = np.flatnonzero(~spread & (b.refid == 0))
    pos[sp0[0]] = pos[grp0[len(grp0) // 2]]            # on the position of a group read
    pos[sp0[1]] = pos[b.refid == 0].max() + 10          # behind the last group read of contig 0
    b = _with_pos(b, pos)
    order = _by_position(b)
    b, split, spread = b.take(order), split[order], spread[order]
    g0 = ~spread & (b.refid == 0)
    assert np.isin(b.pos[spread & (b.refid == 0)], b.pos[g0]).any() and b.pos[spread & (b.refid == 0)].max() > b.pos[g0].max()
    assert spread.sum() > 20 and (split == 0).sum() > 5
    return h, b, gof, n_groups, split, spread


def _split_on_device(h, b, gof, n_groups):
    """the split phase on one GPU (sfm.route_device: elp_split_classify, elp_copy_records): the groups and the spread context"""
    reader, eg, es = Engine(h), Engine(h), Engine(h)
    for e in (reader, eg, es):
        e.set_read_group_ids(h.rg_ids)
    raw = orc.bam_encode(b, h.rg_ids)
    sfm.route_device(reader, b, gof, n_groups, np.zeros(n_groups + 2, np.int32), 0, 1, eg, es, stage=lambda e, x: e.stage_bam(raw))
    reader.close()
    return eg, es


def _merged_want(h, b, n_groups, split, spread, spread_order=None, with_spread=True):
    """sfm.merge_splits of the per-split input-order outputs -> (the stream's bytes, the group batches, the spread batch)"""
    bi = _with_ids(b)
    groups = [bi.take(np.flatnonzero((split == g) & ~spread)) for g in range(1, n_groups + 1)]
    sp = bi.take(np.flatnonzero(spread))
    if spread_order is not None:
        sp = sp.take(spread_order)
    merged = sfm.merge_splits(groups, sp if with_spread else sp.take(np.zeros(0, np.int64)), bi.take(np.flatnonzero(split == 0)))
    return b"".join(_expected(b, h.rg_ids, merged.tlen)), groups, sp


def test_coordinate_merge_of_keep_ordered_contexts():
    h, b, gof, n_groups, split, spread = _sorted_case()
    want, groups, sp = _merged_want(h, b, n_groups, split, spread)
    eg, es = _split_on_device(h, b, gof, n_groups)
    e0 = Engine(h)
    try:
        assert eg.n == b.n and eg.n_sorted == b.n - int(spread.sum()) and es.n == int(spread.sum())
        eg.order_keep(fetch=False)
        es.order_keep(fetch=False)
        assert eg.emit_merged_bam(es).tobytes() == want
        # the same slots from elp_merge_spread
        mapped = Batch.concat(groups)
        code = sfm.merge_order(mapped.refid, mapped.pos, sp.refid, sp.pos)
        assert np.array_equal(eg.merge_spread(es), np.flatnonzero(code < 0).astype(np.uint64))
        # a coordinate permutation on one side, a keep permutation on the other
        es.sort_coordinate(fetch=False)
        want_mixed, _, _ = _merged_want(h, b, n_groups, split, spread, orc.sort_coordinate(b.take(np.flatnonzero(spread))))
        assert eg.emit_merged_bam(es).tobytes() == want_mixed
        # an empty spread
        e0.set_read_group_ids(h.rg_ids)
        e0.order_keep(fetch=False)
        assert eg.emit_merged_bam(e0).tobytes() == _merged_want(h, b, n_groups, split, spread, with_spread=False)[0]
        # a permutation by split is not the merge's order
        eg.order_keep(by_split=True, fetch=False)
        es.order_keep(fetch=False)
        for call in (eg.emit_merged_bam, eg.emit_merged_bgzf, eg.merge_spread):
            with pytest.raises(ElpError) as ei:
                call(es)
            assert ei.value.code == ELP_ERR_ARG, call
        # queryname stays unsupported
        eg.sort_queryname(fetch=False)
        with pytest.raises(ElpError) as ei:
            eg.emit_merged_bam(es)
        assert ei.value.code == ELP_ERR_UNSUPPORTED
    finally:
        for e in (eg, es, e0):
            e.close()


@pytest.mark.parametrize("side", ["groups", "spread"])
@pytest.mark.parametrize("at", [MERGE_CHECK_W - 1, MERGE_CHECK_W, 1, 3 * MERGE_CHECK_W + 40])
def test_coordinate_merge_refuses_keep_ordered_records_with_an_inversion(side, at):
    """one pair of neighbours exchanged, at either side of a workgroup boundary of the check kernel (entry k is compared with entry k - 1 by
    thread k % MERGE_CHECK_W of workgroup k / MERGE_CHECK_W), at the front and in the last, partly filled workgroup"""
    cfg, b, h, _, _ = dataset("tiny", 1500, 17, 0.03)
    n = 3 * MERGE_CHECK_W + 41
    b = b.take(np.flatnonzero(b.refid == 0)[:n])
    assert b.n == n
    b = _with_pos(b, 10 + 2 * np.arange(n))
    order = np.arange(n)
    order[[at - 1, at]] = order[[at, at - 1]]
    bad, good = orc.bam_encode(b.take(order), h.rg_ids), orc.bam_encode(b, h.rg_ids)
    eg, es = Engine(h), Engine(h)
    try:
        for e, raw in ((eg, bad if side == "groups" else good), (es, bad if side == "spread" else good)):
            e.set_read_group_ids(h.rg_ids)
            e.stage_bam(raw)
            e.order_keep(fetch=False)
        for call in (eg.emit_merged_bam, eg.merge_spread, eg.emit_merged_bgzf):
            with pytest.raises(ElpError) as ei:
                call(es)
            assert ei.value.code == ELP_ERR_DATA and "records are not in coordinate order" in str(ei.value), call
        (eg if side == "groups" else es).sort_coordinate(fetch=False)  # sorted on the device: the merge runs
        assert len(tagref.records(eg.emit_merged_bam(es).tobytes())) == 2 * n
    finally:
        eg.close()
        es.close()


# ---- 7. the merge of unsorted splits
def _unsorted_case(with_unmapped=True, with_spread=True):
    """an unsorted read set cut into split files 0 (unmapped), 1, 2, 3 and a spread file; the group files hold sr-tagged copies of the
    spread reads.  -> header, the read set with the copies tagged, the group files in the order they are staged [(id, indices)], the
    spread mask, the expected stream's bytes"""
    cfg, b, h, _, _ = dataset("tiny", 1500, 9, 0.03)
    split = np.where(b.refid < 0, 0, b.refid + 1).astype(np.uint16)
    if not with_unmapped:
        keep = np.flatnonzero(split != 0)
        b, split = b.take(keep), split[keep]
    spread = (split != 0) & (np.arange(b.n) % 7 == 2) & with_spread
    files = [(g, np.flatnonzero(split == g)) for g in (2, 0, 3, 1)]  # (staged in this order)
    bi = _with_ids(b)
    groups = [bi.take(np.flatnonzero((split == g) & ~spread)) for g in (1, 2, 3)]
    merged = sfm.merge_splits_unsorted(groups, bi.take(np.flatnonzero(spread)), bi.take(np.flatnonzero(split == 0)))
    assert with_unmapped == bool((split == 0).sum()) and with_spread == bool(spread.sum())
    return h, b, files, spread, b"".join(_expected(b, h.rg_ids, merged.tlen))


def _stage_unsorted(h, b, files, spread):
    """(a record's bytes are the oracle's encoding of it as a record of the whole read set, in its group file with the sr tag if it is
    also a spread read)"""
    tagged, sp_idx = sfm.with_sr(b, spread), np.flatnonzero(spread)
    eg, es = Engine(h), Engine(h)
    for e in (eg, es):
        e.set_read_group_ids(h.rg_ids)
    for g, idx in files:
        if idx.size:
            eg.stage_bam(orc.bam_encode(tagged, h.rg_ids, order=idx.astype(np.uint32)), split_id=g)
    if sp_idx.size:
        es.stage_bam(orc.bam_encode(b, h.rg_ids, order=sp_idx.astype(np.uint32)), split_id=0)
    return eg, es


@pytest.mark.parametrize("with_unmapped,with_spread", [(True, True), (False, True), (True, False)])
def test_concat_of_unsorted_splits(with_unmapped, with_spread):
    h, b, files, spread, want = _unsorted_case(with_unmapped, with_spread)
    eg, es = _stage_unsorted(h, b, files, spread)
    try:
        sp_idx = np.flatnonzero(spread)
        g_state = np.concatenate([spread[idx].astype(np.uint8) for _, idx in files])
        g_split = np.concatenate([np.full(idx.size, g, np.uint16) for g, idx in files])
        _same(eg.order_keep(by_split=True), keep_ref.keep_order(g_state, g_split, by_split=True)[0], "groups")
        es.order_keep(fetch=False)
        got = eg.emit_concat_bam(es).tobytes()
        # keep_ref's restatement of the stream names the same records as sfm.merge_splits_unsorted
        staged = np.concatenate([idx for _, idx in files])
        ids = [int(staged[k]) if src == "g" else int(sp_idx[k]) for src, k in keep_ref.concat_stream(g_state, g_split, np.zeros(sp_idx.size, np.uint8))]
        assert b"".join(_expected(b, h.rg_ids, ids)) == want
        assert got == want
    finally:
        eg.close()
        es.close()


def test_concat_refuses_other_permutation_kinds():
    h, b, files, spread, want = _unsorted_case()
    eg, es = _stage_unsorted(h, b, files, spread)

    def refused():
        for call in (eg.emit_concat_bam, eg.emit_concat_bgzf):
            with pytest.raises(ElpError) as ei:
                call(es)
            assert ei.value.code == ELP_ERR_ARG, call
    try:
        refused()                                   # no permutation at all
        eg.order_keep(by_split=True, fetch=False)
        refused()                                   # none on the spread side
        es.order_keep(by_split=True, fetch=False)
        refused()                                   # by split on the spread side
        es.sort_coordinate(fetch=False)
        refused()
        es.order_keep(fetch=False)
        assert eg.emit_concat_bam(es).tobytes() == want
        for order in (lambda: eg.order_keep(fetch=False), lambda: eg.sort_coordinate(fetch=False), lambda: eg.sort_queryname(fetch=False)):
            order()
            refused()                               # plain keep, coordinate, queryname on the groups side
    finally:
        eg.close()
        es.close()


# ---- 8. the BGZF forms
def _check_bgzf(eg, es, fn_bam, fn_bgzf, name):
    want = fn_bam(es).tobytes()
    assert len(want) > 3 * 65280
    for per_pass in (0, 97):  # 97 records are ~25 KB: most members straddle two or three passes
        eg.set_tuning("emit_pass", per_pass)
        n = C.c_uint64()
        eg._check(getattr(eg.L, name)(eg.h, es.h, C.c_void_p(0), 0, C.byref(n)))
        bz = fn_bgzf(es).tobytes()
        mem = _members(bz)
        assert b"".join(m for _, m in mem) == want, (name, per_pass)
        assert all(len(m) == 65280 for _, m in mem[:-1]) and 0 < len(mem[-1][1]) <= 65280, (name, per_pass)
        assert int(n.value) >= len(bz), (name, per_pass)
        assert fn_bam(es).tobytes() == want, (name, per_pass)
    eg.set_tuning("emit_pass", 0)


@pytest.mark.parametrize("order", ["coordinate", "keep"])
def test_merged_bgzf_inflates_to_the_merged_bam(order):
    h, b, gof, n_groups, split, spread = _sorted_case()
    eg, es = _split_on_device(h, b, gof, n_groups)
    try:
        for e in (eg, es):
            sfm._order_call(e, order)(False)
        if order == "keep":
            assert eg.emit_merged_bam(es).tobytes() == _merged_want(h, b, n_groups, split, spread)[0]
        _check_bgzf(eg, es, eg.emit_merged_bam, eg.emit_merged_bgzf, "elp_emit_merged_bgzf")
    finally:
        eg.set_tuning("emit_pass", 0)
        eg.close()
        es.close()


def test_concat_bgzf_inflates_to_the_concat_bam():
    h, b, files, spread, want = _unsorted_case()
    eg, es = _stage_unsorted(h, b, files, spread)
    try:
        eg.order_keep(by_split=True, fetch=False)
        es.order_keep(fetch=False)
        assert eg.emit_concat_bam(es).tobytes() == want
        _check_bgzf(eg, es, eg.emit_concat_bam, eg.emit_concat_bgzf, "elp_emit_concat_bgzf")
    finally:
        eg.set_tuning("emit_pass", 0)
        eg.close()
        es.close()
