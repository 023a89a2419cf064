"""A DEFLATE token reader written from RFC 1951, for the tests of the device's BGZF writer: where zlib's inflate only says what a
block inflates to, this reader says HOW it was coded - the block type, every match with its place, the number of literals, the code
lengths of both alphabets and the number of bits the block takes - so that a test can hold the compressor to claims about its parse
(tests/bgzf_payloads.py has the claims).  It reads ONE block, which must be the final one, and is strict where a writer can be wrong
without zlib noticing or where zlib's own rules are the ones to hold: see read_block."""
from collections import namedtuple

Block = namedtuple("Block", "btype matches n_literals ll_lens d_lens bits data")
Block.__doc__ = """btype: 0 stored, 1 fixed codes, 2 dynamic codes; matches: [(output position, length, distance)]; n_literals;
ll_lens / d_lens: the code lengths of the literal / length and the distance alphabet ([] in a stored block); bits: the bits read, the
block header's three included; data: what the block inflates to"""


class DeflateError(ValueError):
    """the bytes are not one valid final DEFLATE block"""


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def kraft(lens, maxbits=15):
    """the code's Kraft sum in units of 2^-maxbits: 1 << maxbits for a complete code, more for an over-subscribed one"""
    return sum(1 << (maxbits - l) for l in lens if l)


def check_code(lens, maxbits, what, one_bit_code_allowed=False):
    """RFC 1951 3.2.2 / 3.2.7: a code must be complete; the one incomplete form allowed is a distance alphabet with a single code of one
    bit (and the one without any code, for a block of literals only)"""
    if any(l > maxbits for l in lens):
        raise DeflateError("%s: a code longer than %d bits" % (what, maxbits))
    k, full = kraft(lens, maxbits), 1 << maxbits
    if k > full:
        raise DeflateError("%s: over-subscribed code" % what)
    if k < full:
        used = [l for l in lens if l]
        if not (one_bit_code_allowed and used in ([], [1])):
            raise DeflateError("%s: incomplete code" % what)


def _table(lens):
    """decoding table of a canonical code (RFC 1951 3.2.2): entry [the next maxlen bits of the stream, LSB first] = symbol << 4 | length,
    0 where no code begins so"""
    maxlen = max(lens) if any(lens) else 1
    table = [0] * (1 << maxlen)
    code = 0
    for length in range(1, maxlen + 1):
        for sym, l in enumerate(lens):
            if l == length:
                rev = int(format(code, "0%db" % length)[::-1], 2)  # Huffman codes enter the stream MSB first
                n = 1 << (maxlen - length)
                table[rev::1 << length] = [sym << 4 | length] * n
                code += 1
        code <<= 1
    return table, (1 << maxlen) - 1


def read_block(cdata, max_out=1 << 20):
    """cdata: one final DEFLATE block and nothing else -> Block.  DeflateError if BFINAL is not set, the type is 11, a stored block's
    NLEN is not ~LEN, a code is over-subscribed or incomplete (check_code), a run-length symbol of the header repeats nothing or runs
    over the alphabets' end, the end-of-block symbol has no code, a symbol without a code or beyond the alphabets (286, 287; 30, 31) is
    read, a distance reaches in front of the block's first byte (there is no history: a BGZF member stands alone), the block ends
    behind the data's end or before its last byte, or a bit behind the block's end in its last byte is set."""
    cdata = bytes(cdata)
    total = 8 * len(cdata)
    buf = cdata + bytes(8)
    pos = [0]

    def take(k):
        v = (int.from_bytes(buf[pos[0] >> 3:(pos[0] >> 3) + 8], "little") >> (pos[0] & 7)) & ((1 << k) - 1)
        pos[0] += k
        if pos[0] > total:
            raise DeflateError("the block runs over the data's end")
        return v

    if take(1) != 1:
        raise DeflateError("BFINAL is not set")
    btype = take(2)
    if btype == 3:
        raise DeflateError("BTYPE 11")
    if btype == 0:
        pos[0] = (pos[0] + 7) & ~7
        n, nn = take(16), take(16)
        if n ^ nn != 0xFFFF:
            raise DeflateError("stored block: NLEN is not the complement of LEN")
        at = pos[0] >> 3
        if at + n != len(cdata):
            raise DeflateError("stored block: %d bytes behind the header, LEN says %d" % (len(cdata) - at, n))
        return Block(0, [], n, [], [], 8 * (at + n), cdata[at:at + n])
    if btype == 1:
        ll_lens, d_lens = list(FIXED_LL), list(FIXED_D)
    else:
        hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
        if hlit > 286 or hdist > 30:
            raise DeflateError("HLIT %d / HDIST %d" % (hlit, hdist))
        cl = [0] * 19
        for k in range(hclen):
            cl[_CL_ORDER[k]] = take(3)
        check_code(cl, 7, "code of the code lengths")
        tab, mask = _table(cl)
        lens = []
        while len(lens) < hlit + hdist:
            e = tab[(int.from_bytes(buf[pos[0] >> 3:(pos[0] >> 3) + 8], "little") >> (pos[0] & 7)) & mask]
            if not e:
                raise DeflateError("header: no code of the code lengths begins so")
            take(e & 15)
            s = e >> 4
            if s < 16:
                lens.append(s)
            elif s == 16:
                if not lens:
                    raise DeflateError("header: symbol 16 with nothing to repeat")
                lens += [lens[-1]] * (3 + take(2))
            elif s == 17:
                lens += [0] * (3 + take(3))
            else:
                lens += [0] * (11 + take(7))
        if len(lens) != hlit + hdist:
            raise DeflateError("header: a run passes the alphabets' end")
        ll_lens, d_lens = lens[:hlit], lens[hlit:]
        if not ll_lens[256]:
            raise DeflateError("the end-of-block symbol has no code")
        check_code(ll_lens, 15, "literal / length code")
        check_code(d_lens, 15, "distance code", one_bit_code_allowed=True)
    ll_tab, ll_mask = _table(ll_lens)
    d_tab, d_mask = _table(d_lens)
    out = bytearray()
    matches, n_lit, p = [], 0, pos[0]
    frm = int.from_bytes
    while True:
        if p > total:
            raise DeflateError("the block runs over the data's end")
        v = frm(buf[p >> 3:(p >> 3) + 8], "little") >> (p & 7)  # (57 bits or more: a match takes 15 + 5 + 15 + 13 at the most)
        e = ll_tab[v & ll_mask]
        if not e:
            raise DeflateError("no literal / length code begins so at bit %d" % p)
        p += e & 15
        v >>= e & 15
        s = e >> 4
        if s < 256:
            out.append(s)
            n_lit += 1
            continue
        if s == 256:
            break
        if s > 285:
            raise DeflateError("literal / length symbol %d" % s)
        xb = _LEN_EXTRA[s - 257]
        length = _LEN_BASE[s - 257] + (v & ((1 << xb) - 1))
        p += xb
        v >>= xb
        e = d_tab[v & d_mask]
        if not e:
            raise DeflateError("no distance code begins so at bit %d" % p)
        p += e & 15
        v >>= e & 15
        ds = e >> 4
        if ds > 29:
            raise DeflateError("distance symbol %d" % ds)
        xb = _DIST_EXTRA[ds]
        dist = _DIST_BASE[ds] + (v & ((1 << xb) - 1))
        p += xb
        if dist > len(out):
            raise DeflateError("a distance of %d at output position %d reaches in front of the block" % (dist, len(out)))
        matches.append((len(out), length, dist))
        if dist >= length:
            out += out[len(out) - dist:len(out) - dist + length]
        else:
            out += (bytes(out[-dist:]) * (length // dist + 1))[:length]
        if len(out) > max_out:
            raise DeflateError("more than %d bytes" % max_out)
    if p > total:
        raise DeflateError("the block runs over the data's end")
    if (p + 7) >> 3 != len(cdata):
        raise DeflateError("the block ends at bit %d, the data has %d bytes" % (p, len(cdata)))
    if p & 7 and cdata[-1] >> (p & 7):
        raise DeflateError("bits behind the block's end are set in its last byte")
    return Block(btype, matches, n_lit, ll_lens, d_lens, p, bytes(out))


def used_distance_symbols(block):
    """the distance symbols (RFC 1951 3.2.5) of the block's matches"""
    used = set()
    for _, _, dist in block.matches:
        ds = 29
        while _DIST_BASE[ds] > dist:
            ds -= 1
        used.add(ds)
    return used
