"""elp_stage_bgzf on DEFLATE as other writers frame it (tests/deflate_forms.py): every valid form of the catalogue must inflate to what
zlib's inflate gives (tests/test_deflate_forms_cpu.py pins that), every invalid one must be refused.  The records behind or inside the
forms are compared with the same records through elp_stage_bam."""
import zlib

import numpy as np
import pytest

import oracle as orc
from elprep_amd.engine import ElpError, Engine
from tests import deflate_forms as df
from tests.test_gpu_round4 import _bam_case, _bgzf
from tests.test_gpu_round6 import _records_with_payload_tags

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case():
    """the records (about 600 pairs with payload tags of every kind) and what elp_stage_bam makes of them: computed once, left unchanged"""
    if "case" not in _CACHE:
        b, h, raw0, off0 = _bam_case(600, seed=41)
        raw, rec_off = _records_with_payload_tags(raw0, off0, 3)
        e = Engine(h)
        e.set_read_group_ids(h.rg_ids)
        e.stage_bam(raw, rec_off=rec_off)
        assert e.n == b.n
        flags = e.mark_duplicates(True)
        e.sort_coordinate()
        want = e.emit_sorted_bam().tobytes()
        e.close()
        assert np.array_equal(flags, orc.mark_duplicates(b, h))
        _CACHE["case"] = (b, h, raw.tobytes(), [int(x) for x in rec_off], flags, want)
    return _CACHE["case"]


def _forms():
    if "forms" not in _CACHE:
        _CACHE["forms"] = df.valid_forms()
    return _CACHE["forms"]


def _own_members():
    """the forms with content of their own, each encoded once: [(form, member, intended bytes)]"""
    if "own" not in _CACHE:
        _CACHE["own"] = [(f, e.member, e.data) for f, e in ((f, f.encode()) for f in _forms() if f.own)]
    return _CACHE["own"]


def _staged(h, bz, first_record=0, tuning=None):
    """(n, flags, sorted BAM bytes) of a BGZF file through elp_stage_bgzf"""
    e = Engine(h, tuning=tuning)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bgzf(np.frombuffer(bz, dtype=np.uint8), first_record=first_record)
        n = e.n
        flags = e.mark_duplicates(True) if n else None
        if n:
            e.sort_coordinate()
        return n, flags, e.emit_sorted_bam().tobytes() if n else b""
    finally:
        e.close()


def _through_forms(group, stream):
    """the stream cut into members, member k in form k of the group (cycling), each of the size its form is about.  A part that no
    writer could frame in the form - 65536 bytes of noise do not fit a member - is written plainly in two halves, and the form takes the
    bytes behind it.  Returns the file, the forms applied, the member sizes, the group's forms and how often a part was written plainly."""
    key = ("file", group)
    if key not in _CACHE:
        forms = [f for f in _forms() if f.group == group and not f.own]
        members, applied, sizes, fallbacks, k, i = [], [], [], 0, 0, 0
        while k < len(stream):
            f = forms[i % len(forms)]
            size = f.size
            part = stream[k:k + size]
            e = f.encode(part) if len(part) == size else None
            if e is not None and len(e.cdata) <= df.MAX_CDATA:
                assert zlib.decompress(e.member, wbits=31) == part, f.name  # (zlib is the reference for these very bytes too)
                members.append(e.member)
                applied.append(f.name)
                sizes.append(len(part))
                i += 1
            else:
                members += [df.plain_member(part[:len(part) // 2]), df.plain_member(part[len(part) // 2:])] if len(part) > 1 else [df.plain_member(part)]
                fallbacks += 1
            k += len(part)
        _CACHE[key] = (b"".join(members) + df.EOF_MEMBER, applied, sizes, [f.name for f in forms], fallbacks)
    return _CACHE[key]


@pytest.mark.parametrize("group", df.DATA_GROUPS)
def test_records_through_every_form(group):
    b, h, stream, rec_off, flags, want = _case()
    bz, applied, sizes, names, fallbacks = _through_forms(group, stream)
    assert set(applied) == set(names), sorted(set(names) - set(applied))  # every form of the group took a part of the stream
    # a part is written plainly only in the record of 70000 noise bytes (65536 of them fit no member: twice at the most) and at the
    # stream's end (once)
    assert fallbacks <= 3, fallbacks
    assert 65536 in sizes  # records straddle the seams of 65536-byte members
    n, got_flags, got = _staged(h, bz)
    assert n == b.n
    assert np.array_equal(got_flags, flags)
    assert got == want


def _record_members(stream):
    if "records" not in _CACHE:
        _CACHE["records"] = _bgzf(stream, 6)
    return _CACHE["records"]


@pytest.mark.parametrize("where", ["member_start", "mid_member", "no_records", "scan_pieces_in_the_prefix", "scan_pieces_no_records"])
def test_crafted_members_in_the_prefix(where):
    """the forms that generate their content as members in front of the records, first_record behind them: staging succeeds only if the
    device's CRC-32 over what it inflated is the CRC-32 of the intended bytes, for every member.  first_record at a member's first byte
    (the byte behind the last prefix member), in mid-member, and at the end of the inflated data (no records).  With "bgzf_piece" below
    the prefix's size whole scan pieces lie in front of first_record: they stage nothing."""
    b, h, stream, rec_off, flags, want = _case()
    own = _own_members()
    prefix = b"".join(m for _, m, _ in own)
    n_prefix = sum(len(d) for _, _, d in own)
    assert n_prefix > 6 * 65536 and len(own) >= 140
    tuning = {"bgzf_piece": 70_000} if where.startswith("scan_pieces") else None
    if where.endswith("no_records"):
        n, _, _ = _staged(h, prefix + df.EOF_MEMBER, n_prefix, tuning)
        assert n == 0
        return
    if where == "mid_member":  # the last prefix bytes and the first records share a member
        junk = bytes(range(256)) * 3
        bz = prefix + df.plain_member(junk + stream[:1000]) + _bgzf(stream[1000:], 6)
        n_prefix += len(junk)
    else:
        bz = prefix + _record_members(stream)
    n, got_flags, got = _staged(h, bz, n_prefix, tuning)
    assert n == b.n
    assert np.array_equal(got_flags, flags)
    assert got == want


@pytest.mark.parametrize("tuning", [None, {"bgzf_piece": 70_000}], ids=["one_piece", "scan_pieces_in_the_prefix"])
def test_a_prefix_members_crc_is_checked(tuning):
    """the control of the test above: one bit of the CRC-32 of one PREFIX member flipped - the file is refused, also where the member
    lies in a scan piece that stages nothing"""
    b, h, stream, rec_off, flags, want = _case()
    own = _own_members()
    n_prefix = sum(len(d) for _, _, d in own)
    members = [m for _, m, _ in own]
    k = len(members) // 2
    bad = bytearray(members[k])
    bad[-8] ^= 0x10
    members[k] = bytes(bad)
    with pytest.raises(ElpError, match="invalid CRC-32"):
        _staged(h, b"".join(members) + _record_members(stream), n_prefix, tuning)
    with pytest.raises(ElpError, match="invalid CRC-32"):
        _staged(h, b"".join(members) + df.EOF_MEMBER, n_prefix, tuning)  # (and where no scan piece holds a record)


def _few_records(stream, rec_off):
    """the first records of the stream as three small members, and their number"""
    n = 5
    part = stream[:rec_off[n]]
    assert len(part) < 8000
    return _bgzf(part, 6, cut=len(part) // 3 + 1), n


def test_each_form_alone():
    """every valid form as a one-member file of its own in front of a few record members, on one context with elp_reset between them:
    a form the decoder refuses or inflates to other bytes is named"""
    b, h, stream, rec_off, flags, want = _case()
    tail, n_rec = _few_records(stream, rec_off)
    at = rec_off[12]  # (the forms that take the caller's bytes get record bytes from here on: behind the records of 70000 bytes)
    failures = []
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        for f, own in [(f, None) for f in _forms() if not f.own] + [(f, (m, d)) for f, m, d in _own_members()]:
            if own is None:
                enc = f.encode(stream[at:at + f.size])
                own = (enc.member, enc.data)
                assert zlib.decompress(enc.member, wbits=31) == stream[at:at + f.size], f.name
                assert enc.info.get("n_dynamic", 300) >= 300, f.name  # (many_blocks is many blocks on these bytes too)
            e.reset()
            try:
                e.stage_bgzf(np.frombuffer(own[0] + tail, dtype=np.uint8), first_record=len(own[1]))
                if e.n != n_rec:
                    failures.append("%s: %d records" % (f.name, e.n))
            except ElpError as err:
                failures.append("%s: %s" % (f.name, err))
    finally:
        e.close()
    assert not failures, failures


def test_invalid_forms_are_refused():
    """every invalid form, as a member between a good prefix member and the records, is refused by the DECODER (its message, which the
    call reports before a CRC mismatch); the call returns, and after elp_reset the same context stages the good file.  Where a decoder
    that lacked the form's check would leave definite bytes the member carries their CRC-32, so that the CRC compare cannot refuse it
    either.  The controls: a valid stream framed the same way is accepted, and with a wrong CRC-32 it is refused with the CRC's message,
    not the decoder's."""
    b, h, stream, rec_off, flags, want = _case()
    tail, n_rec = _few_records(stream, rec_off)
    head = bytes(range(256)) * 2
    good = df.plain_member(head) + tail
    valid = df.Deflater()
    valid.dynamic(df.lz_parse(df._INVALID_TEXT), final=True)
    wrong = []
    e = Engine(h)
    try:
        e.set_read_group_ids(h.rg_ids)
        e.stage_bgzf(np.frombuffer(df.plain_member(head) + df.frame(valid.getvalue(), bytes(valid.out)) + tail, dtype=np.uint8), first_record=len(head) + len(valid.out))
        assert e.n == n_rec
        e.reset()
        with pytest.raises(ElpError, match="invalid CRC-32"):
            e.stage_bgzf(np.frombuffer(df.plain_member(head) + df.frame(valid.getvalue(), crc=0, isize=len(valid.out)) + tail, dtype=np.uint8),
                         first_record=len(head) + len(valid.out))
        for name, cdata, isize in df.invalid_forms():
            assert df.rejected(cdata, isize), name
            lax = df.lax_output(name, isize, head)
            bad = df.plain_member(head) + df.frame(cdata, crc=zlib.crc32(lax) if lax is not None else 0, isize=isize) + tail
            e.reset()
            try:
                e.stage_bgzf(np.frombuffer(bad, dtype=np.uint8), first_record=len(head) + isize)
                wrong.append("%s: accepted" % name)
            except ElpError as err:
                if "does not inflate" not in str(err):
                    wrong.append("%s: %s" % (name, err))
            e.reset()
            e.stage_bgzf(np.frombuffer(good, dtype=np.uint8), first_record=len(head))
            assert e.n == n_rec, name
    finally:
        e.close()
    assert not wrong, wrong
