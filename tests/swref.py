"""A plain Python restatement of the HaplotypeCaller's Smith-Waterman, `runSmithWaterman` and `lastIndex` (filters/sw.go:96-316), with
the full score and backtrack matrices as the reference keeps them.  This is the readable one: it follows the Go source line by line and
shares nothing with elprep_amd/csrc/sw_core.hpp.  tests/swref_c.c is the same again in C (the fast one); tests/test_swref_cpu.py pins
both on hand-derived cases and against each other.

A CIGAR is a list of (length, op) with op one of "MIDS"; `encode` gives BAM's `len << 4 | op` words."""

SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 0, 1, 2, 3  # sw.go:31-36
MIN_INT32 = -(1 << 31)
MATRIX_MIN_CUTOFF = -100000000   # sw.go:132
LOW_INIT_VALUE = MIN_INT32 // 2  # sw.go:133
OPS = "MIDNSHP=X"

P1 = (10, -15, -30, -5)      # realignment of reads, filters/realign.go:310
P2 = (25, -50, -110, -6)     # dangling ends, filters/assemble-reads.go:1042,1152
P3 = (200, -150, -260, -11)  # haplotype CIGARs, filters/sw.go:401

_TO_N = b"RYMKWSBDHV"


def to_upper_and_n(base: int) -> int:
    """fasta.ToUpperAndN (fasta/fasta-files.go:126-151): acgtn and ACGTN become ACGTN, the other IUPAC letters in either case N, all
    other bytes stay"""
    up = base & ~0x20 if 0x61 <= base <= 0x7A else base
    if up in b"ACGTN":
        return up
    if up in _TO_N:
        return 0x4E
    return base


def last_index(ref: bytes, seq: bytes) -> int:
    """sw.go:96-108: the LAST offset at which seq stands in the normalised reference; seq is compared raw"""
    ql = len(seq)
    r = len(ref) - ql
    while r >= 0:
        q = 0
        while q < ql and to_upper_and_n(ref[r + q]) == seq[q]:
            q += 1
        if q == ql:
            return r
        r -= 1
    return -1


def run_smith_waterman(reference: bytes, alternate: bytes, params, strategy: int):
    """sw.go:110-316.  Returns (cigar, alignment offset)."""
    match_value, mismatch_penalty, gap_open, gap_extend = params
    if strategy in (SOFTCLIP, IGNORE):
        off = last_index(reference, alternate)
        if off >= 0:
            return [(len(alternate), "M")], off

    ref_length, alt_length = len(reference), len(alternate)
    nrow, ncol = ref_length + 1, alt_length + 1
    sw = [[0] * ncol for _ in range(nrow)]
    backtrack = [[0] * ncol for _ in range(nrow)]
    best_gap_v = [LOW_INIT_VALUE] * (ncol + 1)
    gap_size_v = [0] * (ncol + 1)
    best_gap_h = [LOW_INIT_VALUE] * (nrow + 1)
    gap_size_h = [0] * (nrow + 1)

    if strategy in (INDEL, LEADING_INDEL):  # :141-156; these cells are not clamped
        top = sw[0]
        if ncol > 1:
            top[1] = gap_open
        cur = gap_open
        for i in range(2, ncol):
            cur += gap_extend
            top[i] = cur
        if nrow > 1:
            sw[1][0] = gap_open
        cur = gap_open
        for i in range(2, nrow):
            cur += gap_extend
            sw[i][0] = cur

    cur_row = sw[0]
    for i in range(1, nrow):  # :160-210
        a_base = reference[i - 1]
        last_row = cur_row
        cur_row = sw[i]
        bt_row = backtrack[i]
        for j in range(1, ncol):
            b_base = alternate[j - 1]
            step_diag = last_row[j - 1] + (match_value if a_base == b_base else mismatch_penalty)

            prev_gap = last_row[j] + gap_open
            best_gap_v[j] += gap_extend
            if prev_gap > best_gap_v[j]:
                best_gap_v[j] = prev_gap
                gap_size_v[j] = 1
            else:
                gap_size_v[j] += 1
            step_down, kd = best_gap_v[j], gap_size_v[j]

            prev_gap = cur_row[j - 1] + gap_open
            best_gap_h[i] += gap_extend
            if prev_gap > best_gap_h[i]:
                best_gap_h[i] = prev_gap
                gap_size_h[i] = 1
            else:
                gap_size_h[i] += 1
            step_right, ki = best_gap_h[i], gap_size_h[i]

            if step_diag >= step_down and step_diag >= step_right:
                cur_row[j] = max(MATRIX_MIN_CUTOFF, step_diag)
                bt_row[j] = 0
            elif step_right >= step_down:
                cur_row[j] = max(MATRIX_MIN_CUTOFF, step_right)
                bt_row[j] = -ki
            else:
                cur_row[j] = max(MATRIX_MIN_CUTOFF, step_down)
                bt_row[j] = kd

    max_score = MIN_INT32  # :212-238
    segment_length = 0
    p1 = 0
    p2 = alt_length
    if strategy == INDEL:
        p1 = ref_length
    else:
        for i in range(1, nrow):
            cur_score = sw[i][alt_length]
            if cur_score >= max_score:
                p1 = i
                max_score = cur_score
        if strategy != LEADING_INDEL:
            bottom = sw[ref_length]
            for j in range(1, ncol):
                cur_score = bottom[j]
                if cur_score > max_score or (cur_score == max_score and abs(ref_length - j) < abs(p1 - p2)):
                    p1 = ref_length
                    p2 = j
                    max_score = cur_score
                    segment_length = alt_length - j

    lce = []  # :240-275
    if segment_length > 0 and strategy == SOFTCLIP:
        lce.append([segment_length, "S"])
        segment_length = 0
    state = "M"
    while True:
        step_length = 1
        btr = backtrack[p1][p2]
        if btr > 0:
            new_state = "D"
            step_length = btr
            p1 -= btr
        elif btr < 0:
            new_state = "I"
            step_length = -btr
            p2 += btr
        else:
            new_state = "M"
            p1 -= 1
            p2 -= 1
        if new_state == state:
            segment_length += step_length
        else:
            lce.append([segment_length, state])
            segment_length = step_length
            state = new_state
        if p1 <= 0 or p2 <= 0:
            break

    if strategy == SOFTCLIP:  # :277-297
        lce.append([segment_length, state])
        if p2 > 0:
            lce.append([p2, "S"])
        offset = p1
    elif strategy == IGNORE:
        lce.append([segment_length + p2, state])
        offset = p1 - p2
    else:
        lce.append([segment_length, state])
        if p1 > 0:
            lce.append([p1, "D"])
        elif p2 > 0:
            lce.append([p2, "I"])
        offset = 0

    lce.reverse()  # :299-315
    i = 1
    while i < len(lce):
        if lce[i - 1][0] == 0:
            del lce[i - 1]
        elif lce[i - 1][1] == lce[i][1]:
            lce[i - 1][0] += lce[i][0]
            del lce[i]
        else:
            i += 1
    if lce[-1][0] == 0:
        lce.pop()
    return [(n, op) for n, op in lce], offset


def cigar_string(cigar) -> str:
    return "".join("%d%s" % (n, op) for n, op in cigar)


def encode(cigar):
    return [(n << 4) | OPS.index(op) for n, op in cigar]


def decode(words):
    return [(int(w) >> 4, OPS[int(w) & 15]) for w in words]
