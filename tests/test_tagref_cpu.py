"""Known answers for tests/tagref.py (-m "not gpu"), derived by hand from the Go sources it restates and written out as bytes: the
restatement is what the GPU tests of the optional-field options take their expected bytes from, so it is pinned here first."""
import struct

import pytest

from tests import tagref

# one unmapped record without CIGAR and bases, read name "r": 32 fixed bytes + "r\0"; the optional fields follow
HEAD = bytes.fromhex("ffffffff" "ffffffff" "02" "00" "4812" "0000" "0400" "00000000" "ffffffff" "ffffffff" "00000000") + b"r\0"


def _rec(tags: bytes) -> bytes:
    return struct.pack("<I", len(HEAD) + len(tags)) + HEAD + tags


def _tags(rec: bytes) -> bytes:
    assert struct.unpack_from("<I", rec)[0] == len(rec) - 4 and rec[4:4 + len(HEAD)] == HEAD
    return rec[4 + len(HEAD):]


NM5, RGAB, XTU, NM7 = b"NMC\x05", b"RGZab\0", b"XTAU", b"NMi\x07\0\0\0"
T = NM5 + RGAB + XTU + NM7  # two fields of key NM


def test_parse_and_rebuild():
    assert len(HEAD) == 34 and tagref.tags_at(_rec(T)) == 38
    assert tagref.parse_fields(_rec(T)) == [(b"NM", b"C", b"\x05"), (b"RG", b"Z", b"ab\0"), (b"XT", b"A", b"U"), (b"NM", b"i", b"\x07\0\0\0")]
    arr = b"XBBs\x02\0\0\0\x01\0\xff\xff"
    assert tagref.parse_fields(_rec(arr + NM5)) == [(b"XB", b"B", b"s\x02\0\0\0\x01\0\xff\xff"), (b"NM", b"C", b"\x05")]
    assert tagref.parse_fields(_rec(b"")) == []
    two = _rec(NM5) + _rec(b"")
    assert tagref.records(two) == [_rec(NM5), _rec(b"")]
    got = tagref.append_fields(two, [[tagref.int_field(b"X0", b"s", 1)], [(b"XT", b"A", b"U")]])
    assert got == _rec(NM5 + b"X0s\x01\0") + _rec(XTU)  # block_size rewritten: 34 + 9 and 34 + 4
    assert got[:4] == b"\x2b\0\0\0"


def test_normalize_is_format_bam_tags_integer_rule():
    f = tagref.parse_fields(_rec(b"NMi\x07\0\0\0" b"ASs\xfd\xff" b"XLI\x70\x11\x01\0" b"XNi\xc0\x63\xff\xff" b"XSi\x2c\x01\0\0" b"XCc\x7f" b"XTAU" b"XDs\x00\x80"))
    assert tagref.with_fields(_rec(b""), tagref.normalize(f)) == \
        _rec(b"NMC\x07" b"ASc\xfd" b"XLI\x70\x11\x01\0" b"XNi\xc0\x63\xff\xff" b"XSS\x2c\x01" b"XCC\x7f" b"XTAU" b"XDs\x00\x80")


def test_remove_and_keep_lists():
    r = _rec(T)
    assert _tags(tagref.apply_tag_filter(r)) == T
    assert _tags(tagref.apply_tag_filter(r, remove=["XT"], keep=["NM", "XT"])) == NM5 + NM7  # remove first, then keep
    assert _tags(tagref.apply_tag_filter(r, remove=["NM"])) == RGAB + XTU                      # duplicate keys: both go
    assert _tags(tagref.apply_tag_filter(r, keep=["NM"])) == NM5 + NM7                         # ... or both stay, in their order
    assert _tags(tagref.apply_tag_filter(r, remove=["RG"])) == NM5 + XTU + NM7                 # a list that names RG
    assert _tags(tagref.apply_tag_filter(r, keep=[b"RG"])) == RGAB
    assert _tags(tagref.apply_tag_filter(r, remove="all")) == b""
    assert _tags(tagref.apply_tag_filter(r, keep="none")) == b""
    assert _tags(tagref.apply_tag_filter(r, remove="all", keep=["NM"])) == b""
    assert _tags(tagref.apply_tag_filter(r, remove=[])) == T                                   # RemoveOptionalFields: an empty list is no filter
    assert _tags(tagref.apply_tag_filter(r, keep=[])) == b""                                   # KeepOptionalFields: an empty list is `none`
    assert _tags(tagref.apply_tag_filter(r, remove=["Nm", "nM", "NN", "N"])) == T              # one byte off, or not two bytes: no match
    assert _tags(tagref.apply_tag_filter(r, keep=["NMX"])) == b""                              # a keep list that can match nothing
    assert _tags(tagref.apply_tag_filter(r, remove=["NM", "RG", "XT"])) == b""
    assert tagref.apply_tag_filter(_rec(b""), remove=["NM"], keep=["RG"]) == _rec(b"")          # a record without any field


X_OK = b"X1C\0XMC\0XOC\0XGC\0"


def test_strict_keep():
    assert tagref.strict_keep(_rec(b"X0C\x01" + X_OK)) == "keep"
    assert tagref.strict_keep(_rec(b"X0s\x01\0" + X_OK)) == "keep"
    assert tagref.strict_keep(_rec(NM5 + b"X0I\x01\0\0\0" + XTU + X_OK)) == "keep"
    assert tagref.strict_keep(_rec(X_OK)) == "reject"                                          # X0 missing
    assert tagref.strict_keep(_rec(b"")) == "reject"
    assert tagref.strict_keep(_rec(b"X0C\x01X1C\0XMC\0XOC\0")) == "reject"                      # XG missing
    assert tagref.strict_keep(_rec(b"X0C\x01X1C\0XMC\0XOC\0XGc\xff")) == "reject"               # XG = -1
    assert tagref.strict_keep(_rec(b"X0C\x01X1C\0XMA0XOC\0XGC\0")) == "panics"                  # XM:A: x.(int64) on a byte
    assert tagref.strict_keep(_rec(b"X0C\x02X1C\0XMA0XOC\0XGC\0")) == "reject"                  # ... never reached: X0 = 2 fails first
    assert tagref.strict_keep(_rec(b"X0C\x01X1C\x03XMA0XOC\0XGC\0")) == "reject"
    assert tagref.strict_keep(_rec(b"X0Z1\0" + X_OK)) == "panics"
    assert tagref.strict_keep(_rec(b"X0C\x01X0C\x02" + X_OK)) == "keep"                         # Get: the first field of a key
    assert tagref.strict_keep(_rec(b"X0C\x02X0C\x01" + X_OK)) == "reject"
    assert tagref.strict_keep(_rec(b"XGC\0XOC\0XMC\0X1C\0X0C\x01")) == "keep"                   # the fields' own order does not matter


def test_replace_read_group():
    assert _tags(tagref.replace_read_group(_rec(RGAB + NM5 + b"RGZcd\0"), "new")) == b"RGZnew\0" + NM5 + b"RGZcd\0"  # Set: the first of two
    assert _tags(tagref.replace_read_group(_rec(NM5 + b"RGAx" + XTU), "new")) == NM5 + b"RGZnew\0" + XTU             # type A becomes Z, in place
    assert _tags(tagref.replace_read_group(_rec(NM5 + XTU), b"new")) == NM5 + XTU + b"RGZnew\0"                      # none: appended last
    assert tagref.replace_read_group(_rec(b""), "g") == _rec(b"RGZg\0")                                              # a record without any field
    assert _tags(tagref.replace_read_group(_rec(b"RGZa\0"), "longer-id")) == b"RGZlonger-id\0"
    # the tag filter acts on the result
    assert _tags(tagref.apply_tag_filter(tagref.replace_read_group(_rec(NM5), "new"), remove=["RG"])) == NM5
    assert _tags(tagref.apply_tag_filter(tagref.replace_read_group(_rec(NM5), "new"), keep=["RG"])) == b"RGZnew\0"


def test_malformed_type_is_an_error():
    with pytest.raises(ValueError):
        tagref.parse_fields(_rec(b"NMq\x05"))
