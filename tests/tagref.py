"""The optional-field options of `elprep filter` restated in plain Python on BAM record bytes (test infrastructure: no device code,
nothing of elprep_amd).  Written from the Go sources, statement by statement where a statement decides a byte:

    parse_fields         parseBamAlignment's tag loop          sam/bam-files.go:138-221, 373-396
    normalize            formatBamTag's integer rule           sam/bam-files.go:492-525
    apply_tag_filter     RemoveOptionalFields                  filters/simple-filters.go:235-257
                         KeepOptionalFields                    filters/simple-filters.go:261-288
                         in filters2's order: remove, keep     cmd/filter.go:878-902
                         SmallMap.DeleteIf                     utils/small-map.go:89-99
    replace_read_group   AddOrReplaceReadGroup, aln.SetRG      filters/simple-filters.go:156-162
                         SmallMap.Set                          utils/small-map.go:59-67
    strict_keep          RemoveNonExactMappingReadsStrict      filters/simple-filters.go:115-134
                         SmallMap.Get                          utils/small-map.go:45-52

A record is its bytes with the block_size field in front; a field is (key: 2 bytes, type: 1 byte, value bytes) - for type B the value
holds the element type, the count and the elements, for Z / H the NUL.  Functions that change a record return new bytes with block_size
rewritten."""
import struct

_INT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
_ELEM = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def records(bam_bytes):
    """the records of a stream of BAM alignment records"""
    bam_bytes = bytes(bam_bytes)
    out, p = [], 0
    while p < len(bam_bytes):
        bs = struct.unpack_from("<I", bam_bytes, p)[0]
        out.append(bam_bytes[p:p + 4 + bs])
        p += 4 + bs
    assert p == len(bam_bytes)
    return out


def tags_at(rec):
    """offset of the first optional field inside a record (block_size field included)"""
    l_name = rec[12]
    n_cig = struct.unpack_from("<H", rec, 16)[0]
    l_seq = struct.unpack_from("<I", rec, 20)[0]
    return 4 + 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq


def parse_fields(rec):
    out, p = [], tags_at(rec)
    while p < len(rec):
        key, ty = rec[p:p + 2], rec[p + 2:p + 3]
        p += 3
        if ty in _SIZE:
            n = _SIZE[ty]
        elif ty in (b"Z", b"H"):
            n = rec.index(b"\0", p) - p + 1
        elif ty == b"B":
            n = 5 + _ELEM[rec[p:p + 1]] * struct.unpack_from("<I", rec, p + 1)[0]
        else:
            raise ValueError("field type %r" % ty)
        out.append((key, ty, rec[p:p + n]))
        p += n
    assert p == len(rec)
    return out


def with_fields(rec, fields):
    """the record with these optional fields in place of its own"""
    body = rec[4:tags_at(rec)] + b"".join(k + t + v for k, t, v in fields)
    return struct.pack("<I", len(body)) + body


def int_field(key, ty, value):
    """an integer field in a type of the caller's choice (what other writers produce)"""
    return (key, ty, struct.pack(_INT[ty], value))


def int_value(ty, val):
    """the int64 parseBamAlignment makes of an integer field; None for every other type"""
    return struct.unpack(_INT[ty], val)[0] if ty in _INT else None


def normalize(fields):
    """the fields as formatBamTag writes them: integers in the smallest type that holds them, unsigned if >= 0; the rest as it came"""
    out = []
    for key, ty, val in fields:
        v = int_value(ty, val)
        if v is not None:
            if v < 0:
                ty = b"c" if v >= -128 else (b"s" if v >= -32768 else b"i")
            else:
                ty = b"C" if v <= 255 else (b"S" if v <= 65535 else b"I")
            val = struct.pack(_INT[ty], v)
        out.append((key, ty, val))
    return out


def append_fields(bam_bytes, per_record_fields):
    """every record of the stream with extra fields behind its own: per_record_fields[k] = the fields of the k-th record"""
    recs = records(bam_bytes)
    assert len(recs) == len(per_record_fields)
    return b"".join(with_fields(r, parse_fields(r) + list(extra)) for r, extra in zip(recs, per_record_fields))


def _keys(lst):
    return [k.encode() if isinstance(k, str) else bytes(k) for k in lst]


def apply_tag_filter(rec, remove=None, keep=None):
    """remove: a list of keys, "all" or None (no such option); keep: a list of keys, "none" or None (no such option)"""
    fields = parse_fields(rec)
    # cmd/filter.go:878-889: --remove-optional-fields
    if remove is not None:
        if remove == "all":
            fields = []                                           # KeepOptionalFields(nil): aln.TAGS = nil
        else:
            optionals = _keys(remove)
            if len(optionals) != 0:                               # RemoveOptionalFields: len(tags) == 0 -> no filter
                fields = [f for f in fields if not any(tag == f[0] for tag in optionals)]  # DeleteIf: every entry that matches
    # cmd/filter.go:891-902: --keep-optional-fields
    if keep is not None:
        optionals = [] if keep == "none" else _keys(keep)
        if len(optionals) == 0:
            fields = []                                           # aln.TAGS = nil
        else:
            fields = [f for f in fields if any(tag == f[0] for tag in optionals)]
    return with_fields(rec, fields)


def replace_read_group(rec, rg_id):
    """aln.SetRG(id) = aln.TAGS.Set(RG, id): the first entry of the key takes the value (a string: type Z), else a new entry at the end"""
    rg_id = rg_id.encode() if isinstance(rg_id, str) else bytes(rg_id)
    fields = parse_fields(rec)
    for index in range(len(fields)):
        if fields[index][0] == b"RG":
            fields[index] = (b"RG", b"Z", rg_id + b"\0")
            return with_fields(rec, fields)
    fields.append((b"RG", b"Z", rg_id + b"\0"))
    return with_fields(rec, fields)


def strict_keep(rec):
    """"keep", "reject", or "panics" (x.(int64) on a value of another type)"""
    fields = parse_fields(rec)

    def get(key):                                                  # SmallMap.Get: the first entry of the key
        for k, ty, val in fields:
            if k == key:
                return (ty, val), True
        return None, False

    for key, want in ((b"X0", 1), (b"X1", 0), (b"XM", 0), (b"XO", 0), (b"XG", 0)):
        x, ok = get(key)
        if not ok:
            return "reject"
        v = int_value(*x)
        if v is None:
            return "panics"
        if v != want:
            return "reject"
    return "keep"
