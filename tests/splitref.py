"""`elprep split`'s files restated in plain Python on BAM record bytes (test infrastructure: no device code; of elprep_amd nothing).
Written from the Go sources, statement by statement where a statement decides a byte or a file:

    route          SplitFilePerChromosome's loop body           sam/split-merge.go:280-293
                   contigToGroup["*"] = "unmapped"              sam/split-merge.go:254
                   RNEXT "=" is next_refid == refid             sam/bam-files.go:344-346
    split_files    ... and SplitSingleEndFilePerChromosome's    sam/split-merge.go:696-707
    set_sr         aln.TAGS.Set(sr, int64(1))                   sam/split-merge.go:290
                   SmallMap.Set                                 utils/small-map.go:59-67
                   formatBamTag: 1 is type C                    sam/bam-files.go:509-513

Built on tests/tagref.py (records, parse_fields, with_fields, normalize; replace_read_group is the model of Set) and, for the SAM form,
tests/samref.py.  A record is its bytes with the block_size field in front.  File 0 is the unmapped file, files 1 .. n_groups are the group
files, file n_groups + 1 (paired input only) is the spread file; group_of_ref[refid] = 1 .. n_groups."""
import struct

from tests import samref, tagref


def refids(rec):
    """(refid, next_refid) of a record; below 0 is "*" """
    return struct.unpack_from("<i", rec, 4)[0], struct.unpack_from("<i", rec, 24)[0]


def route(rec, group_of_ref):
    """-> (file of the record's contig group, whether it also goes to the spread file)"""
    refid, nref = refids(rec)
    group = group_of_ref[refid] if refid >= 0 else 0                  # contigToGroup[aln.RNAME]
    if nref != refid and refid >= 0:                                  # aln.RNEXT != "=" && aln.RNAME != "*"  (:286)
        group_next = group_of_ref[nref] if nref >= 0 else 0           # contigToGroup[aln.RNEXT]
        return int(group), int(group_next) != int(group)
    return int(group), False


def written(rec):
    """the record as formatBamAlignment(parseBamAlignment(record)) writes it: integers in their smallest type"""
    return tagref.with_fields(rec, tagref.normalize(tagref.parse_fields(rec)))


def set_sr(rec):
    """aln.TAGS.Set(sr, int64(1)): the first entry of the key takes the value (an int64 1: type C), else a new entry at the end"""
    fields = tagref.parse_fields(rec)
    for index in range(len(fields)):
        if fields[index][0] == b"sr":
            fields[index] = (b"sr", b"C", b"\x01")
            return tagref.with_fields(rec, fields)
    fields.append((b"sr", b"C", b"\x01"))
    return tagref.with_fields(rec, fields)


def split_files(bam_bytes, group_of_ref, n_groups, single_end=False, rejected=()):
    """-> the files as lists of record bytes.  rejected: indices of records an earlier filter took out (they appear nowhere)"""
    files = [[] for _ in range(n_groups + (1 if single_end else 2))]
    rejected = set(int(i) for i in rejected)
    for i, rec in enumerate(tagref.records(bam_bytes)):
        if i in rejected:
            continue
        group, spread = route(rec, group_of_ref)
        if single_end:                                                # :696-707: the group's file, nothing else
            files[group].append(written(rec))
            continue
        if spread:
            files[n_groups + 1].append(written(rec))                  # :289 the spread file gets the record as it is
            rec = set_sr(rec)                                         # :290
        files[group].append(written(rec))                             # :292
    return files


def split_bytes(bam_bytes, group_of_ref, n_groups, single_end=False, rejected=()):
    """-> the files as BAM record streams"""
    return [b"".join(f) for f in split_files(bam_bytes, group_of_ref, n_groups, single_end, rejected)]


def split_lines(bam_bytes, group_of_ref, n_groups, names, single_end=False, rejected=()):
    """-> the files as SAM text (tests/samref.py's lines of the files' records)"""
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    return [b"".join(samref.line(r, names) for r in f) for f in split_files(bam_bytes, group_of_ref, n_groups, single_end, rejected)]
