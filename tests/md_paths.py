"""The smallest read sets that take each host path of mark duplicates (markdup_impl, csrc/markdup.hip; the decisions are
csrc/markdup_plan.hpp's): every one holds duplicate pairs, so a path that does nothing shows in the flags.

Shared by tests/test_md_paths_cpu.py (the read sets are what they claim: oracle only) and tests/test_gpu_md_paths.py (device against oracle,
and the kernels that ran)."""
import functools

from elprep_amd.batch import batch_from_records
from tests.kat_cases import Q20, Q40, SEQ
from tests.md_seams import ReadSet, header  # noqa: F401  (two contigs of 2000 bases)

SEPARATED_AT = (20, 61)  # where the listed set's far-apart mates stand: 40 records between them


def _rec(name, flag, pos, pnext, tlen, qual):
    return dict(qname=name, flag=flag, refid=0, pos=pos, cigar="10M", mapq=60, next_refid=0, pnext=pnext, tlen=tlen, seq=SEQ, qual=qual, rgid=0)


def _pair(name, k, qual):
    """a true pair at place k: first end forward at 100 + k, mate reverse at 700 + k"""
    p1, p2 = 100 + k, 700 + k
    return [_rec(name, 99, p1, p2, p2 + 10 - p1, qual), _rec(name, 147, p2, p1, p1 - p2 - 10, qual)]


def adjacent_pairs(npairs):
    """npairs pairs in aligner order (mates next to each other), names all different.  Pair k stands at place k, except that every
    fourth pair (k = 1, 5, ...) repeats the place of the pair in front of it with lower qualities: a duplicate pair."""
    out = []
    for k in range(npairs):
        out += _pair("p%d" % k, k - 1, Q20) if k % 4 == 1 else _pair("p%d" % k, k, Q40)
    return out


def listed_records():
    """64 adjacent pairs and one more pair, a low-quality copy of pair 2, whose ends stand at SEPARATED_AT: two records for the mate table"""
    out = adjacent_pairs(64)
    x = _pair("x", 2, Q20)
    out.insert(SEPARATED_AT[0], x[0])
    out.insert(SEPARATED_AT[1], x[1])
    return out


def big_group_records():
    """kat_cases.toggling_cases' first: pair a, then three records t0 t1 t2 of one name - (t0, t1) pair up and lose against a"""
    a = _pair("a", 0, Q40)
    t = _pair("t", 0, Q20)
    return a + t + [dict(t[0], pos=1300)]


RECORDS = {
    "fast": lambda: adjacent_pairs(4),       # 8 records: the least n with n / 8 > 0
    "below_the_cut": lambda: adjacent_pairs(3),
    "listed": listed_records,
    "big_group": big_group_records,
    "one_bucket": lambda: adjacent_pairs(383),   # 766 records: the most whose pair list is one bucket (ndig == 0)
    "two_buckets": lambda: adjacent_pairs(384),  # 768: the least with a radix pass
}


@functools.lru_cache(maxsize=None)
def read_set(name: str) -> ReadSet:
    return ReadSet(batch_from_records(RECORDS[name]()))
