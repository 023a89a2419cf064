"""tests/deflate_forms.py's catalogue against zlib's inflate: every valid form inflates to its intended bytes, has the property it is named
for, and every invalid form is rejected.  What the device's decoder is then held to (tests/test_gpu_inflate_forms.py) is zlib's verdict."""
import zlib

import numpy as np
import pytest

from tests import deflate_forms as df


def sample(n, seed=5):
    """bytes that look like alignment records to a compressor: names that count, short alphabets, runs, a little noise"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    k = 0
    while len(out) < n:
        out += b"\x9c\x00\x00\x00\x01\x00\x00\x00" + int(k * 37).to_bytes(4, "little") + b"read:%d:%d\x00" % (k % 7, k)
        out += bytes(rng.choice(np.frombuffer(b"\x11\x12\x24\x48\x81\x88", dtype=np.uint8), 50))
        out += bytes(rng.choice(np.frombuffer(b"#,:FFFFF", dtype=np.uint8), 100))
        if k % 9 == 0:
            out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(3, 600))
        if k % 13 == 0:
            out += rng.integers(0, 256, int(rng.integers(1, 60)), dtype=np.uint8).tobytes()
        k += 1
    return bytes(out[:n])


@pytest.fixture(scope="module")
def encoded():
    """every valid form encoded once: [(form, Enc)]"""
    return [(f, f.encode(None if f.own else sample(f.size or 5000, seed=len(f.name)))) for f in df.valid_forms()]


def test_every_valid_form_inflates_to_its_intended_bytes(encoded):
    names = [f.name for f, _ in encoded]
    assert len(set(names)) == len(names)
    for f, e in encoded:
        o = zlib.decompressobj(-15)
        got = o.decompress(e.cdata)
        assert o.eof and o.unused_data == b"" and o.unconsumed_tail == b"", f.name
        assert got == e.data and 0 < len(e.data) <= 65536, f.name
        if not f.own:
            assert e.data == sample(f.size or 5000, seed=len(f.name)), f.name
        m = e.member
        assert len(m) <= 65536 and zlib.decompress(m, wbits=31) == e.data, f.name
        assert len(m) == int.from_bytes(m[16:18], "little") + 1, f.name


def test_the_forms_have_the_properties_they_are_named_for(encoded):
    by = {f.name: (f, e) for f, e in encoded}
    phases = {"dynamic": set(), "fixed": set()}
    for f, e in encoded:
        b = e.d.blocks
        if f.props.get("go_close"):  # a non-final block, then BFINAL=1 stored LEN=0
            assert b[-1]["type"] == 0 and b[-1]["len"] == 0 and b[-1]["final"] and len(b) >= 2 and not any(x["final"] for x in b[:-1]), f.name
            assert e.cdata[-4:] == b"\x00\x00\xff\xff", f.name
        if "phase" in f.props and f.group == "go_close":
            assert e.info["phase"] == f.props["phase"], f.name
            assert b[-1]["start"] == e.info["eob_end"], f.name
            if b[-2]["type"]:
                phases["dynamic" if b[-2]["type"] == 2 else "fixed"].add(e.info["phase"])
        if f.name.startswith("stored_after_compressed"):
            assert e.info["phase"] == f.props["phase"] and b[-1]["type"] == 0 and b[-2]["type"] == 2, f.name
        if "isize" in f.props:
            assert len(e.data) == f.props["isize"], f.name
        if "ntok" in f.props:
            assert e.d.ntok == f.props["ntok"] == 21846 and e.d.nmatch == 21845 and e.d.nmatch < 21888, f.name
        if "header_bit" in f.props:
            assert b[1]["type"] == 2 and b[1]["start"] == f.props["header_bit"] == e.info["header_bit"], f.name
        if "stored_end" in f.props:
            assert b[0]["type"] == 0 and b[0]["data_end"] == f.props["stored_end"] and b[1]["type"] == 2, f.name
    assert phases["dynamic"] == set(range(8)) and phases["fixed"] == set(range(8))
    assert sum(1 for f, _ in encoded if f.props.get("isize") == 65536) >= 9
    assert sorted(f.props["header_bit"] for f, _ in encoded if "header_bit" in f.props) == list(range(505 * 8, 520 * 8))
    assert sorted(f.props["stored_end"] for f, _ in encoded if "stored_end" in f.props) == df.SEAMS
    # several data blocks in front of Go's final block; an unused / absent distance code
    assert len(by["go_close_dynamic_cut_phase1"][1].d.blocks) >= 4
    h = by["go_literals_only"][1].d.headers[0]
    assert h["hdist"] == 0 and df.expand_spelling(h["items"])[-1] == 1 and by["go_literals_only"][1].d.nmatch == 0
    h = by["no_dist_codes"][1].d.headers[0]
    assert h["hdist"] == 0 and df.expand_spelling(h["items"])[-1] == 0 and by["no_dist_codes"][1].d.nmatch == 0
    for sym in (0, 29):
        d = by["one_dist_code_symbol_%d" % sym][1].d
        lens = df.expand_spelling(d.headers[0]["items"])[d.headers[0]["hlit"] + 257:]
        assert d.headers[0]["hdist"] == sym and lens == [0] * sym + [1] and d.nmatch >= 300 and d.d_used == {1}
    assert max(by["one_dist_code_symbol_29"][1].d.dists) > 32000
    # blocks
    b = by["flush_blocks"][1].d.blocks
    empty = [x["type"] if x["end"] - x["start"] == (10 if x["type"] == 1 else -1) or (x["type"] == 0 and x["len"] == 0) else None for x in b]
    assert "".join("f" if t == 1 else "s" if t == 0 else "." for t in empty).count("f" * 200) == 1 and empty.count(0) >= 3 and not b[empty.index(0)]["final"]
    assert by["many_blocks"][1].info["n_dynamic"] >= 300 and sum(1 for x in by["many_blocks"][1].d.blocks if x["type"] == 2) >= 300
    assert by["largest_stored_block"][1].cdata.__len__() == df.MAX_CDATA and len(by["largest_stored_block"][1].member) == 65536
    # codes: every code length 1..15 of both alphabets is used by an emitted symbol; the deep codes sit on the frequent symbols
    ll_used, d_used = set(), set()
    for f, e in encoded:
        ll_used |= e.d.ll_used
        d_used |= e.d.d_used
    assert ll_used == set(range(1, 16)) and d_used == set(range(1, 16))
    for f, e in encoded:
        if f.group == "deep_codes":
            assert max(e.d.ll_used) >= 10 and len(e.cdata) * 8 > 9 * e.d.ntok, f.name  # (more than 9 bits a token: the long codes are the common ones)
    d = by["longest_match_symbol"][1].d
    assert d.ll_used == set(range(1, 16)) and d.d_used == set(range(1, 16)) and (284, 258) in d.lens
    d = by["all_lengths_all_dists"][1].d
    assert {n for _, n in d.lens} == set(range(3, 259)) and {(284, 258), (285, 258)} <= d.lens
    assert all(df.DIST_BASE[s] in d.dists and df.DIST_BASE[s] + (1 << df.DIST_EXTRA[s]) - 1 in d.dists for s in range(30)) and 32768 in d.dists
    # header spellings
    hs = {k[7:]: v[1].info["header"] for k, v in by.items() if k.startswith("header_") and not k.startswith("header_at")}
    assert hs["hlit_0"]["hlit"] == 0 and hs["hlit_29"]["hlit"] == 29 and hs["hdist_29"]["hdist"] == 29 and hs["hclen_15"]["hclen"] == 15
    assert hs["hclen_smallest"]["hclen"] == 1 and max(hs["cl_7_bits"]["cl"]) == 7
    it = hs["16_across_boundary"]["items"]
    k = next(k for k, (s, _) in enumerate(it) if s == 16)
    assert len(df.expand_spelling(it[:k])) == 257 and hs["16_across_boundary"]["hlit"] == 0
    assert any(a[0] == 18 and b[0] == 16 for a, b in zip(hs["16_after_18"]["items"], hs["16_after_18"]["items"][1:]))
    assert any(a[0] == 17 and b[0] == 16 for a, b in zip(hs["16_after_17"]["items"], hs["16_after_17"]["items"][1:]))
    assert hs["17_ends_at_the_end"]["items"][-1][0] == 17 and (18, 127) in hs["18_of_138"]["items"]
    assert all(s < 16 for s, _ in hs["no_run_codes"]["items"])
    # matches
    assert by["matches_deep_chain"][1].d.nmatch >= 20000 and by["matches_deep_chain_far"][1].d.nmatch >= 10000
    assert {(258, k) for k in (1, 2, 3, 7, 257)} <= by["matches_self_overlap"][1].d.pairs
    d = by["matches_dist_near_length"][1].d
    assert {(n, n + k) for n in (3, 4, 10, 64, 200, 258) for k in (-1, 0, 1)} <= d.pairs
    d = by["matches_dist_is_position"][1].d  # (position, length, distance): the copies start at byte 0
    assert {(5, 5, 5), (10, 258, 10), (268, 100, 268), (32768, 258, 32768)} <= d.placed
    d = by["matches_into_stored_block"][1].d  # the dynamic block's first match copies the stored block's 700 bytes from byte 0 on
    assert [x["type"] for x in d.blocks] == [0, 2, 0, 1] and d.blocks[0]["len"] == 700 and (700, 258, 700) in d.placed
    assert (1271, 4, 1) in d.placed and (1275, 200, 1215) in d.placed and d.blocks[2]["len"] == 1  # (the fixed block: into the one stored byte, into the first block)
    d = by["matches_into_previous_blocks_match"][1].d  # bytes 30..130 are a match of block 1; block 2 starts with a copy of them
    assert [x["type"] for x in d.blocks] == [2, 2, 1, 2] and {(30, 100, 30), (130, 100, 100), (230, 258, 65), (488, 258, 258)} <= d.placed
    # the 65536-byte members' edges
    d = by["isize_65536_runs_258"][1].d
    assert d.pairs == {(258, 1), (3, 1)} and d.nmatch == 255 and d.ntok == 256
    assert (65536 - 258, 258, 8232) in by["isize_65536_match_ends_at_65535"][1].d.placed
    assert (65533, 3, 32765) in by["isize_65536_match_starts_at_65533"][1].d.placed
    assert {(32768, 258, 32768), (65516, 17, 32768), (65533, 3, 32768)} <= by["isize_65536_dist_32768"][1].d.placed
    d = by["isize_65536_stored_noise_then_compressed"][1].d
    assert [x["type"] for x in d.blocks] == [0, 2] and d.blocks[0]["len"] == 30000 and d.nmatch > 0
    assert by["isize_65536_most_tokens"][1].d.pairs == {(3, 1)}


_WHY = {
    "btype_3": "invalid block type", "stored_len_not_nlen": "invalid stored block lengths", "stored_past_cdata": "not at the end",
    "hlit_30": "too many length or distance symbols", "hlit_31": "too many length or distance symbols",
    "hdist_30": "too many length or distance symbols", "hdist_31": "too many length or distance symbols",
    "cl_code_oversubscribed": "invalid code lengths set", "cl_code_incomplete": "invalid code lengths set",
    "first_length_is_16": "invalid bit length repeat", "run_past_the_lengths": "invalid bit length repeat",
    "no_end_of_block_code": "invalid code -- missing end-of-block",
    "literal_code_oversubscribed": "invalid literal/lengths set", "literal_code_incomplete": "invalid literal/lengths set",
    "distance_code_oversubscribed": "invalid distances set", "distance_code_incomplete": "invalid distances set",
    "unused_pattern_of_the_single_distance_code": "invalid distance code", "match_without_distance_codes": "invalid distance code",
    "fixed_symbol_286": "invalid literal/length code", "fixed_symbol_287": "invalid literal/length code",
    "fixed_distance_30": "invalid distance code", "fixed_distance_31": "invalid distance code",
    "distance_one_more_than_the_position": "invalid distance too far back", "distance_into_the_previous_member": "invalid distance too far back",
    "output_longer_than_isize": "+1 bytes", "output_much_longer_than_isize": "+200 bytes", "output_shorter_than_isize": "-1 bytes",
    "output_much_shorter_than_isize": "-40000 bytes", "stored_longer_than_isize": "+1 bytes",
    "ends_mid_symbol": "not at the end", "ends_in_the_header": "not at the end", "no_final_block": "not at the end",
    "no_final_block_stored": "not at the end",
}


def test_every_invalid_form_is_rejected():
    forms = df.invalid_forms()
    names = [n for n, _, _ in forms]
    assert len(set(names)) == len(names) >= 30
    for name, cdata, isize in forms:
        assert isize > 0 and len(cdata) <= df.MAX_CDATA, name
        assert df.rejected(cdata, isize), name
        # ... and for the reason it is named for: zlib's message, or how far it came without one
        o = zlib.decompressobj(-15)
        try:
            got = o.decompress(cdata)
            why = "not at the end" if not o.eof else "%+d bytes" % (len(got) - isize)
        except zlib.error as err:
            why = str(err).split(": ")[-1]
        assert why == _WHY[name], (name, why)
        # what a decoder without the form's check would leave, where that is defined, is ISIZE bytes: framed with their CRC-32 the
        # member can only be refused by the decoder
        lax = df.lax_output(name, isize, b"previous")
        assert lax is None or len(lax) == isize, name
    assert sum(1 for name, _, isize in forms if df.lax_output(name, isize, b"p") is not None) == 7
    # the check itself: a valid form is not "rejected", and is with another ISIZE
    d = df.Deflater()
    d.dynamic(df.lz_parse(b"abcabcabcabc"), final=True)
    assert not df.rejected(d.getvalue(), 12) and df.rejected(d.getvalue(), 11)


def test_random_codes_are_complete_and_at_most_15_bits_deep():
    for seed in range(20):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(2, 287))
        syms = [int(s) for s in rng.choice(286, n, replace=False)]
        freq = {s: int(rng.integers(0, 1000)) for s in syms}
        code = df.random_complete_code(syms, freq, np.random.default_rng(seed))
        assert df.kraft(code.values()) == 1 and max(code.values()) <= 15 and sorted(code) == sorted(syms)
        assert code == df.random_complete_code(syms, freq, np.random.default_rng(seed))
        order = sorted(syms, key=lambda s: (-freq[s], s))
        assert all(code[a] >= code[b] for a, b in zip(order, order[1:]))  # the frequent symbols have the long codes
        if n >= 64:
            assert max(code.values()) >= 10
    for limit, n in ((15, 286), (7, 19), (15, 30)):
        freq = {s: 1 + (1 << min(s, 40)) for s in range(n)}  # counts that want a deeper tree than the limit
        h = df.huff_lengths(freq, limit)
        assert df.kraft(h.values()) == 1 and max(h.values()) == limit


def test_everything_is_deterministic():
    a, b = df.valid_forms(), df.valid_forms()
    for f, g in list(zip(a, b))[::7]:
        data = None if f.own else sample(f.size or 5000)
        assert f.encode(data).cdata == g.encode(data).cdata, f.name
    assert df.invalid_forms() == df.invalid_forms()
