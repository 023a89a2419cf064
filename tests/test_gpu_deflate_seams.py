"""GPU tests (-m gpu) of the BGZF compressor on the device (k_bgzf_deflate and k_bgzf_frame, elprep_amd/csrc/bgzf_out.hip; algorithm:
deflate_core.hpp) at its match, window, part and block seams.  The host emulation the CPU tests run is compiled from the same header,
but under the device compiler the header swaps in other forms of load4, match_len, find_match, table_insert and bit_reverse, and the
phases, the scans and the LDS that the hash table, the codes and the DEFLATE data share exist in the kernel alone.  The payloads of
tests/bgzf_payloads.py go through the device as the blocks of BAM records' optional fields (records_for), in the three forms of the
writer (default, "bgzf_fixed", "bgzf_stored"); every member is parsed by hand, inflated by zlib, and its tokens are read with
tests/deflate_tokens.py and held to the facts of its payload, which tests/test_bgzf_payloads_cpu.py pins on the emulation."""
import struct
import zlib

import numpy as np
import pytest

from elprep_amd.engine import Engine
from tests import bgzf_payloads as bp
from tests import deflate_tokens as dt

pytestmark = pytest.mark.gpu

PAYLOAD = bp.PAYLOAD
FORMS = {"default": None, "fixed": "bgzf_fixed", "stored": "bgzf_stored"}
BTYPE_OF_KIND = {0: 1, 1: 0, 2: 2}
GZ_HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
_RUNS = {}


class _Writer:
    """one context in one form of the writer; the tuning keys go back to 0 when it closes"""

    def __init__(self, form):
        self.form = form
        self.e = Engine(bp.header())

    def __enter__(self):
        if FORMS[self.form]:
            self.e.set_tuning(FORMS[self.form], 1)
        return self

    def __exit__(self, *exc):
        try:
            self.e.set_tuning("bgzf_fixed", 0)
            self.e.set_tuning("bgzf_stored", 0)
        finally:
            self.e.close()

    def emit(self, blocks):
        """-> (the sorted record stream, its BGZF members as the device wrote them, where each payload's block lies)"""
        raw, rec_off, where = bp.records_for(blocks)
        e = self.e
        e.reset()
        e.set_read_group_ids([bp.RG_ID])
        e.stage_bam(raw, rec_off=rec_off)
        e.sort_coordinate()
        want = e.emit_sorted_bam().tobytes()
        assert len(want) == raw.size
        assert bp.record_names(want) == bp.record_names(raw.tobytes())  # (the records kept their order: the short block is the last)
        return want, e.emit_sorted_bgzf().tobytes(), where


def _members(bz, want, form):
    """the members of a BGZF stream parsed by hand -> [(DEFLATE data, payload)], every member checked against its slice of `want`"""
    out, p, k = [], 0, 0
    n_blocks = (len(want) + PAYLOAD - 1) // PAYLOAD
    while p < len(bz):
        assert bz[p:p + 16] == GZ_HEAD, k
        bsize = struct.unpack_from("<H", bz, p + 16)[0] + 1
        assert 26 <= bsize <= 65536 and p + bsize <= len(bz), k
        cdata = bz[p + 18:p + bsize - 8]
        crc, isize = struct.unpack_from("<II", bz, p + bsize - 8)
        d = zlib.decompressobj(-15)
        data = d.decompress(cdata) + d.flush()
        assert d.eof and not d.unused_data, k
        assert data == want[PAYLOAD * k:PAYLOAD * (k + 1)], k
        assert isize == len(data) and crc == zlib.crc32(data), k
        assert len(data) == PAYLOAD or (k == n_blocks - 1 and 0 < len(data) < PAYLOAD), k
        assert len(cdata) <= len(data) + 5, k  # (the kernel's own rule: a block that would be longer is stored)
        if form == "stored":
            plain = GZ_HEAD + struct.pack("<H", len(data) + 5 + 25) + b"\x01" + struct.pack("<HH", len(data), ~len(data) & 0xFFFF) + data + \
                struct.pack("<II", zlib.crc32(data), len(data))
            assert bz[p:p + bsize] == plain, k
        out.append((cdata, data))
        p += bsize
        k += 1
    assert p == len(bz) and k == n_blocks
    return out


def _catalogue_run(form, mode):
    """the whole catalogue through the device in one form, once per context mode: the full blocks (and one short one behind them) in one
    emit, every other short payload as the last block of an emit of its own.  -> {name: (DEFLATE data, payload, facts)} + the first
    emit's stream and members"""
    key = (form, mode)
    if key not in _RUNS:
        full, short = bp.full_blocks(), bp.short_blocks()
        got = {}
        with _Writer(form) as w:
            first = None
            for group in [full + short[:1]] + [[s] for s in short[1:]]:
                want, bz, where = w.emit([data for _, data, _ in group])
                mem = _members(bz, want, form)
                for (name, data, facts), k in zip(group, where):
                    assert mem[k][1] == data, name  # (the payload is what landed in the block)
                    got[name] = (mem[k][0], data, facts)
                if first is None:
                    first = (want, bz, [m for k, m in enumerate(mem) if k not in where])
        _RUNS[key] = (got, first)
    return _RUNS[key]


@pytest.mark.parametrize("form", list(FORMS))
def test_every_member_inflates_to_its_block(form, engine_mode):
    """every payload of the catalogue as a block of its own: the member's BC field, BSIZE, CRC-32 and ISIZE, its DEFLATE data inflated by
    zlib to exactly its 65280-byte slice of the record stream, no longer than the stored form; with "bgzf_stored" every member is the
    stored framing byte for byte (_members)"""
    got, (want, bz, heads) = _catalogue_run(form, engine_mode)
    assert len(got) == len(bp.payloads())
    assert len(bz) < len(want) or form == "stored"
    if form == "stored":
        assert all(cdata[0] == 1 for cdata, _, _ in got.values())


@pytest.mark.parametrize("form", ["default", "fixed"])
def test_tokens_of_the_devices_own_bytes(form, engine_mode):
    """the device's DEFLATE data read token by token: the planted copies go out by the rule (groups a and c), nothing touches a copy
    whose source lies beyond the window (b), the match-free payloads have no match (d), the run of the first strip alone has one
    distance code (e); everywhere a match is at most 258 long and reaches at most to the block's first byte and 32768 back"""
    got, (want, bz, heads) = _catalogue_run(form, engine_mode)
    n_plants = 0
    for name, (cdata, data, facts) in got.items():
        blk = dt.read_block(cdata)
        assert blk.btype in ((0, 1, 2) if form == "default" else (0, 1)), name
        bp.check_tokens(blk, data, facts, name)
        n_plants += len(facts.get("plants", ()))
    for k, (cdata, data) in enumerate(heads):  # (the records' first blocks: the fixed fields and a run of zeros)
        bp.check_tokens(dt.read_block(cdata), data, {}, "head %d" % k)
    assert n_plants > 2600


@pytest.mark.parametrize("form", ["default", "fixed"])
def test_match_free_blocks_are_the_emulations_bytes(form, engine_mode):
    """where no match exists the tokens cannot depend on the schedule: the device's DEFLATE data is the emulation's, byte for byte - the
    Huffman build, the header's spelling and the bit writer of the device held to the CPU-tested ones"""
    got, _ = _catalogue_run(form, engine_mode)
    n = 0
    for name, (cdata, data, facts) in got.items():
        if facts.get("match_free"):
            assert cdata == bp.emulate(data, 0 if form == "default" else 16)[0], name
            n += 1
    assert n >= 10


@pytest.mark.parametrize("form", ["default", "fixed"])
def test_block_types_are_the_emulations(form, engine_mode):
    """BTYPE on the device is the emulation's choice wherever both thread orders of the emulation make the same one by more than the
    band of tests/bgzf_payloads.py (exempt()); noise is stored, noise with 256 zeros behind it is not"""
    got, _ = _catalogue_run(form, engine_mode)
    exempt = []
    for name, (cdata, data, facts) in got.items():
        btype = (cdata[0] >> 1) & 3
        if bp.exempt(data, facts, form == "fixed"):
            exempt.append(name)
            continue
        kind, by = bp.margin(data, form == "fixed")
        assert btype == BTYPE_OF_KIND[kind], (name, btype, kind, by)
    print("%s form: block type not compared for %d of %d payloads: %s" % (form, len(exempt), len(got), exempt))
    assert 10 * len(exempt) <= len(got)
    assert (got["f noise"][0][0] >> 1) & 3 == 0
    if form == "default":
        assert (got["f noise, 256 zeros"][0][0] >> 1) & 3 == 2


TAILS = [1, 2, 3, 4, 5, 15, 16, 17, 254, 255, 256, 257, 509, 510, 511, 4095, 4096, 4097, 65279]


@pytest.mark.parametrize("form", list(FORMS))
def test_last_block_of_every_length(form, engine_mode):
    """streams of exactly 65280 + t bytes, of 65280 and of 2 * 65280 on one context with elp_reset between them, the tail in turn zeros,
    a de Bruijn prefix and noise: the CRC's fold over a short last part and the 16-byte loads of both kernels at every part and vector
    seam (_members checks CRC-32, ISIZE and what the member inflates to)"""
    db = bp.de_bruijn()
    noise = np.random.default_rng(105).integers(0, 256, PAYLOAD, dtype=np.uint8).tobytes()
    with _Writer(form) as w:
        for k, t in enumerate(TAILS):
            tail = (bytes(t), db[:t], noise[:t])[k % 3]
            want, bz, where = w.emit([tail])
            assert len(want) == PAYLOAD + t
            mem = _members(bz, want, form)
            assert len(mem) == 2 and mem[1][1] == tail, t
            if form != "stored":
                for cdata, data in mem:
                    bp.check_tokens(dt.read_block(cdata), data, {}, "tail %d" % t)
        for blocks in ([], [noise], [db[:PAYLOAD]]):  # (no short block)
            want, bz, where = w.emit(blocks)
            assert len(want) == PAYLOAD * (1 + len(blocks))
            assert len(_members(bz, want, form)) == 1 + len(blocks)


@pytest.mark.parametrize("form", ["default", "fixed"])
def test_a_workgroups_second_block(form, engine_mode):
    """one emit of 2 * CUs + 37 blocks: the kernel's grid is two workgroups per CU, so the workgroup of block b also compresses block
    b + 2 * CUs, with the same LDS (the codes where the hash table was, the DEFLATE data where the payload was) and the same scratch for
    its match notes.  Block b and its successor differ in kind: zeros then noise, noise then a de Bruijn block, planted copies then one
    distance code, a block with dynamic codes then one without any distance code; the last block is short.  Every member and its
    tokens as in the tests above."""
    import torch
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    P = {name: (data, facts) for name, data, facts in bp.payloads()}
    plants = [name for name, data, facts in bp.payloads() if facts["group"] == "a"]
    first = ["g zeros", "f noise", None, "g text"]  # (None: a block of plants)
    second = ["f noise", "d de Bruijn", "e one strip of one value, then de Bruijn", "d de Bruijn in 144..159"]
    names, b = [], 0
    while b < grid + 37:
        if b % (bp.PER_RECORD + 1) == 0:  # (a record's first block)
            b += 1
            continue
        q = b % grid
        pair = q < 37 and (q < 14 or q > 32)
        if b == grid + 36:
            name = "d de Bruijn, 257 bytes"
        elif pair and b < grid:
            name = first[q % 4] or plants[q]
        elif pair:
            name = second[q % 4]
        else:
            name = plants[b % len(plants)]
        names.append(name)
        b += 1
    with _Writer(form) as w:
        want, bz, where = w.emit([P[name][0] for name in names])
    assert len(want) == PAYLOAD * (grid + 36) + 257
    mem = _members(bz, want, form)
    assert len(mem) == grid + 37
    at = dict(zip(where, names))
    pairs = [(at[q], at[q + grid]) for q in range(36) if q in at and q + grid in at]
    for k in range(4):  # the pairs are there: each kind of them three times or more
        assert sum(1 for a, b in pairs if b == second[k] and (a == first[k] or (first[k] is None and a in plants))) >= 3, k
    for k, (cdata, data) in enumerate(mem):
        name = at.get(k)
        if name is not None:
            assert data == P[name][0], (k, name)
        facts = P[name][1] if name is not None else {}
        blk = dt.read_block(cdata)
        bp.check_tokens(blk, data, facts, (k, name))
        if facts.get("match_free"):
            assert cdata == bp.emulate(data, 0 if form == "default" else 16)[0], (k, name)


def test_round_trip_through_the_decoder(engine_mode):
    """the catalogue's members as the device compressed them go back in through elp_stage_bgzf on another context: the same records"""
    got, (want, bz, heads) = _catalogue_run("default", engine_mode)
    e = Engine(bp.header())
    try:
        e.set_read_group_ids([bp.RG_ID])
        e.stage_bgzf(np.frombuffer(bz, dtype=np.uint8))
        e.sort_coordinate()
        assert e.emit_sorted_bam().tobytes() == want
    finally:
        e.close()
