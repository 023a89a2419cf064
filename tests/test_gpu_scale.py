"""GPU parity at the bench's own scale (-m gpu): the whole path against the oracle on read sets whose QUAL column, packed SEQ and BAM
record streams lie far past 2^32 bytes.  Every other oracle comparison stays below 1.2 GB of QUAL; here 15 M pairs of the bench's read set
(genome c3, 150 bp, binned qualities: 30 M reads, 4.5 GB of QUAL, 4.5 G SEQ nibbles, 9.8 GB of BAM records) go through

  * the production step (sort_ahead, the three-lane order, the rows-form LUT, the one-length kernels) and, after a rollback, the general
    flat kernels with the (key, index) pair sort, then the queryname sort and a coordinate sort behind it;
  * stage_bam over many 1 GiB calls, emit_sorted_bam in many 2^21-record passes, emit_sorted_bgzf, and stage_bgzf of that stream;
  * and, on the hg38-sized genome c4, the five-pass coordinate sort with 16384-key radix tiles.

A mismatch names the first differing read and whether its QUAL starts past 2^32.  The names hold `full_size` / `hg38`: conftest.py runs
them once, on a fresh context.  Host memory: the planned peak is checked against MemAvailable up front."""
import os
import resource
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as orc
from elprep_amd.batch import Batch
from elprep_amd.engine import BqsrTables, Engine

pytestmark = pytest.mark.gpu

PAIRS = 15_000_000          # the first 15 M pairs of the bench's read set: 30.1 M reads
HG38_PAIRS = 9_000_000      # 18.1 M reads on genome c4: more than 2^24 + 1 M keys, so the coordinate sort uses 16384-key tiles
CHUNK = 500_000             # pairs per generated batch
STAGE = 2_000_000           # reads per stage() call
MAX_CYCLE = 500
WRAP = 1 << 32
PEAK_GB = 44                # planned host peak of this file (measured on the MI355X host: 31 GB)
THREADS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 16)))


def _log(msg):
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6
    sys.stderr.write("[scale %.0fs, peak RSS %.1f GB] %s\n" % (time.perf_counter() - _T0, rss, msg))


_T0 = time.perf_counter()


def _need_memory(gb):
    with open("/proc/meminfo") as f:
        avail = next(int(line.split()[1]) * 1024 for line in f if line.startswith("MemAvailable:"))
    if avail < gb * 1e9:
        pytest.skip("host memory: %.1f GB available, the planned peak is %d GB" % (avail / 1e9, gb))


def _generate(cfg, pairs):
    from tools import synth
    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(lambda lo: synth.generate(cfg, lo, min(lo + CHUNK, pairs)), range(0, pairs, CHUNK)))
    b = Batch.concat(parts)
    del parts
    return b


def _refs_sites(cfg, h):
    from tools import synth
    with ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(lambda r: (r, synth.reference(cfg, r), orc.flatten(orc.sort_by_start(synth.known_sites_raw(cfg, r)))), range(h.n_ref)))


def _oracle(b, h, refs_sites):
    """the oracle's path as bench.cpu_baseline runs it: flags, permutation, counters, the three tables, QUAL"""
    flags0 = orc.mark_duplicates_mt(b, h, THREADS)
    perm = orc.sort_coordinate_mt(b, flags0, THREADS)
    del flags0
    flags, ctr = orc.dup_metrics_mt(b, h, perm, 100, THREADS)
    tables = orc.bqsr_gather_mt(b, h, orc.BqsrRef([r for _, r, _ in refs_sites], [s for _, _, s in refs_sites]), flags, MAX_CYCLE, THREADS)
    qual = orc.bqsr_apply_mt(orc.BqsrFinal(*tables, MAX_CYCLE), b, h, 0, (), THREADS)
    return SimpleNamespace(flags=flags, perm=perm, ctr=ctr, tables=tables, qual=qual)


def _slice(b, lo, hi):
    """records [lo, hi) of b as a batch of views (offsets rebased): no copy of the payload"""
    cols = {k: getattr(b, k)[lo:hi] for k in ("refid", "pos", "next_refid", "pnext", "tlen", "flag", "mapq", "rgid", "has_sr", "l_seq", "split")}
    for off, dat in (("qname_off", "qname"), ("cigar_off", "cigar"), ("seq_off", "seq4"), ("qual_off", "qual")):
        o = getattr(b, off)[lo:hi + 1]
        cols[off] = o - o[0]
        cols[dat] = getattr(b, dat)[int(o[0]):int(o[-1])]
    return Batch(**cols)


def _preconditions(b, min_reads=16 << 20):
    """what the file claims to cover, asserted so that it cannot quietly shrink"""
    L = int(b.l_seq[0])
    assert (b.l_seq == L).all(), "reads of more than one length"
    assert int(b.qual_off[-1]) > WRAP and int((b.qual_off[:-1] >= WRAP).sum()) > 1_000_000, "QUAL does not reach far enough past 2^32"
    assert int(b.l_seq.sum(dtype=np.uint64)) > WRAP, "SEQ nibbles do not pass 2^32"
    assert b.n >= min_reads
    return L


def _first_diff(got, want, step=1 << 28):
    assert got.shape == want.shape, (got.shape, want.shape)
    for lo in range(0, got.size, step):
        d = np.flatnonzero(got[lo:lo + step] != want[lo:lo + step])
        if d.size:
            return lo + int(d[0])
    return -1


def _expect(what, got, want, qual_off, read_of=lambda k: k, beyond=None):
    """got == want element by element, compared in slices; a mismatch names the first differing read and where its QUAL starts.
    beyond: the first element whose read's QUAL starts past 2^32 - the first difference from there on is named as well (a 32-bit wrap
    can make its first visible damage at the start of the buffer)"""
    k = _first_diff(got, want)
    if k >= 0:
        r = int(read_of(k))
        q = int(qual_off[r])
        msg = "%s: first difference at element %d (got %d, want %d): read %d, whose QUAL starts at byte %d, %s 2^32" % (
            what, k, int(got[k]), int(want[k]), r, q, "PAST" if q >= WRAP else "below")
        if beyond is not None and k < beyond < got.size:
            k2 = _first_diff(got[beyond:], want[beyond:])
            msg += "; past 2^32 the first difference is %s" % ("in read %d" % int(read_of(beyond + k2)) if k2 >= 0 else "nowhere")
        pytest.fail(msg)


def _expect_qual(what, got, want, qual_off, first=0):
    """got / want: bytes [first, first + got.size) of a QUAL column whose reads start at qual_off; reads are named by their index in it"""
    r_wrap = int(np.searchsorted(qual_off, WRAP))  # the first read that starts past 2^32
    _expect(what, got, want, qual_off, lambda k: np.searchsorted(qual_off, first + k, side="right") - 1,
            beyond=int(qual_off[r_wrap]) - first if r_wrap < qual_off.size - 1 else None)


def _expect_path(what, e, o, qual_off, ctr, tables):
    _expect(what + " flags", e.flags(), o.flags, qual_off)
    _expect(what + " permutation", e.permutation(), o.perm, qual_off, lambda k: o.perm[k])
    assert np.array_equal(ctr, o.ctr), what + " duplication counters"
    for name, got, want in zip(("quality", "cycle", "context"), tables, o.tables):
        assert np.array_equal(got, want), "%s %s table" % (what, name)
    q = e.qual()
    _expect_qual(what + " QUAL", q, o.qual, qual_off)
    del q


def _launched(e):
    e.sync()
    return {k: v[0] for k, v in e.profile().items() if v[0]}


def test_full_size_hg38_five_pass_sort_against_the_oracle():
    """genome c4 (hg38's contig lengths: 34 live key bits, five radix passes) with more than 2^24 + 1 M reads (16384-key tiles), the
    production step with sort_ahead on: every output against the oracle"""
    from tools import synth
    _need_memory(PEAK_GB)
    cfg = synth.config("c4")
    h = cfg.header()
    b = _generate(cfg, HG38_PAIRS)
    assert b.n >= (1 << 24) + (1 << 20) and int(b.pos.max()) >= 1 << 27
    rs = _refs_sites(cfg, h)
    o = _oracle(b, h, rs)
    _log("hg38: %d reads, oracle done" % b.n)
    e = Engine(h)
    try:
        _stage_batches(e, b)
        _set_refs(e, rs)
        del rs
        e.profile_enable(True)
        e.profile_reset()
        ctr = _production_step(e, h)
        ran = _launched(e)
        e.profile_enable(False)
        _log("hg38 kernels: %s" % sorted(ran.items()))
        assert ran["radix_scatter"] >= 5
        _expect_path("hg38", e, o, b.qual_off, ctr, e.tables_fetch())
        _log("hg38 equal")
    finally:
        e.close()


@pytest.fixture(scope="module")
def c3():
    """15 M pairs of the bench's read set, staged nowhere yet, and the oracle's outputs on them"""
    from tools import synth
    _need_memory(PEAK_GB)
    cfg = synth.config("c3")
    h = cfg.header()
    b = _generate(cfg, PAIRS)
    rs = _refs_sites(cfg, h)
    _log("generated %d reads, %d QUAL bytes" % (b.n, int(b.qual_off[-1])))
    o = _oracle(b, h, rs)
    _log("oracle done")
    yield SimpleNamespace(cfg=cfg, h=h, b=b, refs_sites=rs, o=o)


def _stage_batches(e, b):
    for lo in range(0, b.n, STAGE):
        e.stage(_slice(b, lo, min(lo + STAGE, b.n)))


def _set_refs(e, refs_sites):
    for r, ref, sites in refs_sites:
        e.set_reference(r, ref)
        e.set_known_sites(r, sites)


def _production_step(e, h):
    """bench.py's step_full in the order "three" with sort_ahead on: the sort and the metrics pass on two host threads, the BQSR chain with
    the rows-form LUT on this one -> the duplication counters"""
    with ThreadPoolExecutor(2) as side:
        e.sort_ahead(True)
        e.mark_duplicates(True, fetch=False)
        st = side.submit(e.sort_coordinate, False)
        mx = side.submit(e.dup_metrics, 100)
        e.recalibrate_device(MAX_CYCLE)
        quals = e.quals_counted()
        rows = e.tables_fetch_rows(quals)
        assert rows is not None
        tb = BqsrTables.from_rows(h.n_cov, quals, *rows, MAX_CYCLE).finalize()
        e.lut_upload_rows(quals, *tb.build_lut_rows(quals, 0), MAX_CYCLE)
        e.apply_bqsr(None, None, MAX_CYCLE, fetch=False)
        st.result()
        ctr = mx.result()
    e.sync()
    return ctr


def test_full_size_whole_path_against_the_oracle(c3):
    """Pass A: the production step.  Pass B, after rollback: the general flat count / apply / score kernels, the sort-first adapt stage
    (mark duplicates behind it: the front pass without its adapt part) and the (key, index) pair sort, in the serial order with the dense
    LUT.  Then the queryname sort and a coordinate sort behind it."""
    from tools.prof.qname_sort_speed import _check, _name_rows
    b, h, o = c3.b, c3.h, c3.o
    _preconditions(b)
    e = Engine(h)
    try:
        _stage_batches(e, b)
        assert e.n == b.n
        _set_refs(e, c3.refs_sites)
        e.sync()
        e.snapshot()

        e.profile_enable(True)
        e.profile_reset()
        ctr = _production_step(e, h)
        ran = _launched(e)
        _log("pass A kernels: %s" % sorted(ran))
        # the one-length kernels: the score kernel (adapt_score; the flat one is adapt_score_flat), count3 (its segment offsets), and apply3
        # on the records the score kernel wrote (with those it launches no bqsr_apply_records of its own; its launch carries the flat
        # kernel's name, bqsr_apply); the coordinate sort in its word form (the pair form's passes are booked as sort_pairs_*)
        for k in ("md_front", "adapt_score", "bqsr_seg_offsets", "bqsr_apply", "radix_scatter"):
            assert k in ran, "pass A did not launch " + k
        for k in ("adapt_fixed", "adapt_score_flat", "bqsr_apply_records", "sort_pairs_radix_scatter"):
            assert k not in ran, "pass A launched " + k
        _expect_path("pass A", e, o, b.qual_off, ctr, e.tables_fetch())
        _log("pass A equal")

        # pass B.  rollback() clears the context's adapted state, and set_tuning("score_kernel") clears it again: the first sort below runs
        # the adapt stage (adapt_fixed, and the score kernel) anew, now with the flat kernel (adapt_score_flat), and mark duplicates then
        # takes the front pass without the adapt part; the sort behind mark duplicates is the one that is checked.  The pair sort's passes
        # are booked as sort_pairs_*; count_kernel=1 shows as the missing count3 segment offsets.  The flat apply kernel and apply3 both
        # launch as bqsr_apply: the profile shows only that apply3's own record kernel did not run.
        e.rollback()
        for k in ("count_kernel", "apply_kernel", "score_kernel", "sort_pairs"):
            e.set_tuning(k, 1)
        e.sort_ahead(False)
        e.profile_reset()
        e.sort_coordinate(fetch=False)
        e.mark_duplicates(True, fetch=False)
        e.sort_coordinate(fetch=False)
        ctr = e.dup_metrics(100)
        tables = e.recalibrate(MAX_CYCLE)
        lut, present = BqsrTables(*tables, MAX_CYCLE).finalize().build_lut(0)
        e.apply_bqsr(lut, present, MAX_CYCLE, fetch=False)
        del lut
        ran = _launched(e)
        e.profile_enable(False)
        _log("pass B kernels: %s" % sorted(ran))
        for k in ("md_front", "adapt_fixed", "adapt_score_flat", "bqsr_count", "bqsr_apply", "sort_pairs_radix_scatter"):
            assert k in ran, "pass B did not launch " + k
        for k in ("adapt_score", "bqsr_seg_offsets", "bqsr_apply_records"):
            assert k not in ran, "pass B launched " + k
        _expect_path("pass B", e, o, b.qual_off, ctr, tables)
        _log("pass B equal")

        perm = e.sort_queryname()
        rows = _name_rows(b, int(np.diff(b.qname_off).max()))
        _check(perm, rows)
        del perm, rows
        _expect("coordinate sort behind the queryname sort", e.sort_coordinate(), o.perm, b.qual_off, lambda k: o.perm[k])
        _log("queryname and coordinate sorts equal")
    finally:
        e.close()


def test_full_size_bam_in_bam_out_against_the_oracle(c3):
    """The same reads as BAM records, staged over ~1 GiB stage_bam calls (half of them walking the block_size chain, half given the record
    offsets), through the path; the sorted BAM and BGZF streams against the oracle's encoding; the BGZF stream staged again."""
    b, h, o = c3.b, c3.h, c3.o
    L = _preconditions(b)
    rg = h.rg_ids
    off = orc.bam_offsets(b, rg)
    assert int(off[-1]) > 2 * WRAP
    cuts = [0]
    while cuts[-1] < b.n:
        cuts.append(min(b.n, int(np.searchsorted(off, off[cuts[-1]] + (1 << 30), side="right")) - 1))
    assert len(cuts) > 8
    ns = orc.num_sorted(b)
    e = Engine(h)
    try:
        e.set_read_group_ids(rg)
        for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            raw = orc.bam_encode(b, rg, order=np.arange(lo, hi, dtype=np.uint32))
            assert raw.size == int(off[hi] - off[lo])
            e.stage_bam(raw, rec_off=(off[lo:hi + 1] - off[lo]) if k % 2 else None)
            del raw
        assert e.n == b.n
        _set_refs(e, c3.refs_sites)
        e.mark_duplicates(True, fetch=False)
        e.sort_coordinate(fetch=False)
        e.recalibrate_device(MAX_CYCLE)
        tables = e.tables_fetch()
        lut, present = BqsrTables(*tables, MAX_CYCLE).finalize().build_lut(0)
        e.apply_bqsr(lut, present, MAX_CYCLE, fetch=False)
        del lut
        _expect("stage_bam flags", e.flags(), o.flags, b.qual_off)
        _expect("stage_bam permutation", e.permutation(), o.perm, b.qual_off, lambda k: o.perm[k])
        for name, got, want in zip(("quality", "cycle", "context"), tables, o.tables):
            assert np.array_equal(got, want), "stage_bam %s table" % name
        q = e.qual()
        _expect_qual("stage_bam QUAL", q, o.qual, b.qual_off)
        del q
        _log("stage_bam path equal")

        bam = e.emit_sorted_bam()
        assert bam.size > WRAP
        pos = 0
        step = 1 << 21
        for lo in range(0, ns, step):
            want = orc.bam_encode(b, rg, order=o.perm[lo:min(lo + step, ns)], flags=o.flags, qual=o.qual, normalize_tags=True)
            got = bam[pos:pos + want.size]
            k = _first_diff(got, want)
            if k >= 0:
                j, p = lo, 0  # (the record that holds byte k: walk the block_size chain of the oracle's slice)
                while p + 4 + int(want[p:p + 4].view(np.uint32)[0]) <= k:
                    p += 4 + int(want[p:p + 4].view(np.uint32)[0])
                    j += 1
                r = int(o.perm[j])
                pytest.fail("emit_sorted_bam: first difference at stream byte %d, in read %d (QUAL at byte %d, %s 2^32)"
                            % (pos + k, r, int(b.qual_off[r]), "PAST" if b.qual_off[r] >= WRAP else "below"))
            pos += want.size
            del want, got
        assert pos == bam.size
        _log("emit_sorted_bam equal: %d bytes" % bam.size)

        bz = e.emit_sorted_bgzf()
        e.close()
        _log("emit_sorted_bgzf: %d bytes" % bz.size)
        starts = [0]
        while starts[-1] < bz.size:
            p = starts[-1]
            assert bz[p] == 0x1F and bz[p + 1] == 0x8B and bz[p + 12] == ord("B") and bz[p + 13] == ord("C")
            starts.append(p + int(bz[p + 16]) + 256 * int(bz[p + 17]) + 1)
        assert starts[-1] == bz.size
        cut = 65280

        def member(k):
            data = zlib.decompress(bz[starts[k]:starts[k + 1]].tobytes(), wbits=31)
            return len(data) == min(cut, bam.size - k * cut) and data == bam[k * cut:k * cut + len(data)].tobytes()
        with ThreadPoolExecutor(THREADS) as pool:
            ok = list(pool.map(member, range(len(starts) - 1)))
        bad = [k for k, v in enumerate(ok) if not v]
        assert not bad, "BGZF member %d does not inflate to bytes %d.. of the BAM stream" % (bad[0], bad[0] * cut)
        assert len(ok) == (bam.size + cut - 1) // cut
        del bam, ok

        e = Engine(h)
        e.set_read_group_ids(rg)
        e.stage_bgzf(bz)
        del bz
        assert e.n == ns
        assert np.array_equal(e.sort_coordinate(), np.arange(ns, dtype=np.uint32)), "stable sort of sorted records is not the identity"
        sorted_off = np.arange(ns + 1, dtype=np.uint64) * L
        _expect("stage_bgzf flags", e.flags(), o.flags[o.perm[:ns]], sorted_off, lambda k: k)
        q = e.qual()
        oq = o.qual.reshape(b.n, L)
        for lo in range(0, ns, STAGE):
            hi = min(lo + STAGE, ns)
            _expect_qual("stage_bgzf QUAL", q[lo * L:hi * L], oq[o.perm[lo:hi]].reshape(-1), sorted_off, first=lo * L)
        del q
        _log("stage_bgzf round trip equal")
    finally:
        e.close()
