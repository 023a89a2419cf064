"""CPU tests of the BGZF compressor's catalogue (tests/bgzf_payloads.py) on the host emulation (tests/deflate_host.cpp), and of the token
reader the device test reads the device's bytes with (tests/deflate_tokens.py).  What the catalogue claims about a payload's tokens must
hold on the emulation in every thread order before the device is held to it (tests/test_gpu_deflate_seams.py)."""
import zlib

import numpy as np
import pytest

from tests import bgzf_payloads as bp
from tests import deflate_forms as df
from tests import deflate_tokens as dt
from tests.test_deflate_cpu import _inflate

BTYPE_OF_KIND = {0: 1, 1: 0, 2: 2}  # the emulation's kind (0 fixed codes, 1 stored, 2 dynamic codes) -> BTYPE


# ---- the token reader
def test_token_reader_against_zlib_and_a_second_writer():
    """blocks of zlib (stored, fixed codes, dynamic codes) and of tests/deflate_forms.py's writer, which keeps the tokens it wrote: the
    reader gives zlib's bytes and the writer's matches, and its bit count ends in the data's last byte"""
    rng = np.random.default_rng(31)
    text = bytes(rng.choice(np.frombuffer(b"ACGTN#I", dtype=np.uint8), 3000)) + bytes(40) + b"ACGTTGCA" * 60
    for level, strategy, btype in ((0, 0, 0), (6, zlib.Z_FIXED, 1), (1, 0, 2), (9, 0, 2), (6, zlib.Z_HUFFMAN_ONLY, 2)):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        cdata = co.compress(text) + co.flush()
        blk = dt.read_block(cdata)
        assert blk.btype == btype and blk.data == text == _inflate(cdata), (level, strategy)
        assert (blk.bits + 7) // 8 == len(cdata)
        assert blk.n_literals + sum(l for _, l, _ in blk.matches) == len(text)
        if strategy == zlib.Z_HUFFMAN_ONLY:
            assert not blk.matches
    toks = df.lz_parse(text)
    for how in ("stored", "fixed", "dynamic"):
        d = df.Deflater()
        if how == "stored":
            d.stored(text, final=True)
        else:
            getattr(d, how)(toks, final=True)
        blk = dt.read_block(d.getvalue())
        assert blk.data == text and blk.bits == d.bitpos
        assert set(blk.matches) == d.placed and len(blk.matches) == d.nmatch
        if how == "dynamic":
            h = d.headers[-1]
            assert len(blk.ll_lens) == h["hlit"] + 257 and len(blk.d_lens) == h["hdist"] + 1
    # literals and a single distance code of one bit (the one incomplete code RFC 1951 allows), used and not used
    ll = [0] * 258
    ll[97], ll[256], ll[257] = 1, 2, 2
    for dl, toks in (([1], [97, 97, 97, (3, 1)]), ([1], [97, 97]), ([0], [97, 97])):
        d = df.Deflater()
        d.dynamic(toks, final=True, ll=ll, dl=dl, check=False)
        blk = dt.read_block(d.getvalue())
        assert blk.data == bytes(d.out) and blk.d_lens == dl


def test_token_reader_refuses_what_it_must():
    """every invalid form of tests/deflate_forms.py that is wrong in the block itself (not in the member's ISIZE); then, each on an
    otherwise valid block: a distance one more than the position, an over-subscribed and an incomplete code of each alphabet, a set bit
    behind the block's end, a byte behind it"""
    for name, cdata, isize in df.invalid_forms():
        if "isize" in name:
            continue
        with pytest.raises(dt.DeflateError):
            dt.read_block(cdata)
    c = df.canonical(df.FIXED_LL)
    cd = df.canonical(df.FIXED_D)

    def fixed_block(dist_sym):
        d = df.Deflater()
        d.bits(1, 1); d.bits(1, 2)
        d.bits(*c[97]); d.bits(*c[98]); d.bits(*c[257]); d.bits(*cd[dist_sym]); d.bits(*c[256])
        return d.getvalue()
    assert dt.read_block(fixed_block(1)).matches == [(2, 3, 2)]
    with pytest.raises(dt.DeflateError, match="reaches in front"):
        dt.read_block(fixed_block(2))
    text = b"abracadabra, abracadabra" * 9
    toks = df.lz_parse(text)
    ll, dl = df.Deflater().auto_lengths(toks)
    assert dt.kraft(ll) == dt.kraft(dl) == 1 << 15
    for what, ll2, dl2 in (("over-subscribed", [l - (l == max(ll)) for l in ll], dl), ("incomplete", [l + (l == max(ll)) for l in ll], dl),
                           ("over-subscribed", ll, [l - (l == max(dl)) for l in dl]), ("incomplete", ll, [l + (l == max(dl)) for l in dl])):
        d = df.Deflater()
        d.header(ll2, dl2, final=True, check=False)
        d.bits(0, 64)
        with pytest.raises(dt.DeflateError, match=what):
            dt.read_block(d.getvalue())
    d = df.Deflater()
    d.dynamic(toks, final=True)
    good = d.getvalue()
    assert dt.read_block(good).data == text
    spare = 8 * len(good) - d.bitpos
    if not spare:  # (a literal more moves the end off the byte's edge)
        d = df.Deflater()
        d.dynamic(df.lz_parse(text + b"!"), final=True)
        good, spare = d.getvalue(), 8 * len(d.getvalue()) - d.bitpos
    assert 0 < spare < 8
    with pytest.raises(dt.DeflateError, match="bits behind"):
        dt.read_block(good[:-1] + bytes([good[-1] | 0x80]))
    with pytest.raises(dt.DeflateError, match="ends at bit"):
        dt.read_block(good + b"\0")
    with pytest.raises(dt.DeflateError):
        dt.read_block(good[:-1])


# ---- the catalogue
def test_catalogue_is_what_it_says():
    P = bp.payloads()
    groups = {}
    for name, data, facts in P:
        groups.setdefault(facts["group"], []).append(name)
    assert sorted(groups) == list("abcdefg")
    plants = [(pl, name) for name, _, facts in P if facts["group"] == "a" for pl in facts["plants"]]
    dists = {d for (_, _, d), _ in plants}
    assert {300, 511, 512, 513, 4096, 4097, 16384, 16385, 24576, 24577, 32767, 32768} <= dists and min(dists) == 6 and max(dists) == 32768
    # every (distance, length, phase) of the sweep but 300 bytes from 300 back
    assert len(plants) == len(bp.A_DISTS) * len(bp.A_LENGTHS) * len(bp.A_PHASES) - len(bp.A_PHASES)
    for d in bp.A_DISTS[1:]:
        assert {(l, p % 256) for (p, l, dd), _ in plants if dd == d} >= {(l, ph) for l in bp.A_LENGTHS for ph in bp.A_PHASES if d >= l + 2}, d
    assert {(l, p % 256) for (p, l, dd), _ in plants if dd == max(l + 2, p % 256 + 1)} >= {(l, ph) for l in bp.A_LENGTHS for ph in bp.A_PHASES}
    for (p, l, d), name in plants:  # the source lies in an earlier strip
        assert (p - d) // 256 < p // 256, name
    beyond = {name for name, _, facts in P if facts["group"] == "b"}
    assert len(beyond) >= 8
    for name, data, facts in P:
        for p, l, d in facts.get("plants", ()):
            assert data[p:p + l] == data[p - d:p - d + l] and data[p - 1] == 202 and data[p - d - 1] == 201 and data[p - d + l] == 203, name
            assert p + l == len(data) or data[p + l] == 204, name
        for lo, hi in facts.get("no_match", ()):
            assert data[lo - 1] == 202 and 0 not in data[lo:hi], name
    ends = {len(data) - p - l for name, data, facts in P if facts["group"] == "c" for p, l, _ in facts.get("plants", ())}
    assert ends == {0, 1, 2, 3}
    assert {len(data) for _, data, facts in P if facts["group"] == "c"} >= {bp.PAYLOAD, bp.N_SHORT}


@pytest.mark.parametrize("order", [0, 1, 16, 17])
def test_every_payload_on_the_emulation(order):
    """zlib inflates the emulation's block to the payload; the token reader reads the same bytes to the same length and the same block
    type, within len + 5 bytes; the payload's facts hold for its tokens"""
    for name, data, facts in bp.payloads():
        cdata, kind, ntok, _ = bp.emulate(data, order)
        assert _inflate(cdata) == data, name
        assert len(cdata) <= len(data) + 5, name
        blk = dt.read_block(cdata)
        assert blk.btype == BTYPE_OF_KIND[kind], name
        assert len(blk.data) == len(data) and (blk.bits + 7) // 8 == len(cdata), name
        if kind != 1:
            assert blk.n_literals + len(blk.matches) == ntok, name
        bp.check_tokens(blk, data, facts, name)
        want = facts.get("kind_fixed" if order >= 16 else "kind")
        if want is not None:
            assert kind == want, (name, kind)
        if "size" in facts and order < 16:
            assert len(cdata) == facts["size"], (name, len(cdata))


def test_match_free_payloads_do_not_depend_on_the_order():
    n = 0
    for name, data, facts in bp.payloads():
        if facts.get("match_free"):
            assert bp.emulate(data, 0)[0] == bp.emulate(data, 1)[0] and bp.emulate(data, 16)[0] == bp.emulate(data, 17)[0], name
            n += 1
    assert n >= 10


def test_the_orders_difference_is_the_documented_one():
    """DELTA and GROUP_DELTA of tests/bgzf_payloads.py are what the emulation gives; the band of 4 * the group's value around a choice of
    form exempts at most one payload in ten from the device test's comparison of block types"""
    P = bp.payloads()
    delta, group = {0: 0, 16: 0}, {}
    for name, data, facts in P:
        for o in (0, 16):
            d = abs(len(bp.emulate(data, o)[0]) - len(bp.emulate(data, o + 1)[0]))
            delta[o] = max(delta[o], d)
            if o == 0:
                group[facts["group"]] = max(group.get(facts["group"], 0), d)
    print("largest difference between the orders: %d bytes, with fixed codes only %d; by group %s" % (delta[0], delta[16], group))
    assert (delta[0], delta[16]) == (bp.DELTA, bp.DELTA_FIXED) and group == bp.GROUP_DELTA
    for fixed_only in (False, True):
        exempt = [name for name, data, facts in P if bp.exempt(data, facts, fixed_only)]
        print("exempt (fixed codes only: %s): %s" % (fixed_only, exempt))
        assert 10 * len(exempt) <= len(P)
