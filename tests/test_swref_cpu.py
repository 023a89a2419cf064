"""The two restatements of runSmithWaterman (filters/sw.go:96-316) that the Smith-Waterman tests measure against - tests/swref.py, plain
Python with the full matrices, and tests/swref_c.c, the same in C - pinned on cases worked out by hand from the Go lines, held against
each other on random problems, and checked for the properties the C ABI states (the operation bound, no zero length, no equal
neighbours).  No Go toolchain exists here: like every other operator's oracle they are pinned by derivation, not by reference output."""
import numpy as np
import pytest

from tests import sw_cases, swref
from tests.swref import IGNORE, INDEL, LEADING_INDEL, P1, P2, P3, SOFTCLIP

ALL = (SOFTCLIP, INDEL, LEADING_INDEL, IGNORE)


def both(ref, alt, params, strategy):
    py = swref.run_smith_waterman(ref, alt, params, strategy)
    c = sw_cases.run_c(ref, alt, params, strategy)
    assert py == c, (py, c)
    return swref.cigar_string(py[0]), py[1]


def test_to_upper_and_n_and_last_index():
    """fasta-files.go:126-151: the table has acgtn / ACGTN -> ACGTN and RYMKWSBDHV in either case -> N; '*', '-', 'U', 'x' are not in it.
    lastIndex (:96-108) walks r from len(ref) - len(seq) DOWN and returns the first fit: the last occurrence; -1 if seq is longer."""
    assert bytes(swref.to_upper_and_n(c) for c in b"acgtnACGTN") == b"ACGTNACGTN"
    assert bytes(swref.to_upper_and_n(c) for c in b"RYMKWSBDHVrymkwsbdhv") == b"N" * 20
    assert bytes(swref.to_upper_and_n(c) for c in b"*-UxuX=") == b"*-UxuX="
    L = sw_cases.swref_c()
    for ref, seq, want in ((b"ACGTACGT", b"ACGT", 4), (b"ACGTTTTT", b"ACGT", 0), (b"acgt", b"ACGT", 0), (b"acgt", b"acgt", -1), (b"ARGT", b"ANGT", 0),
                           (b"ARGT", b"ARGT", -1), (b"ACG", b"ACGT", -1), (b"AAAA", b"AA", 2), (b"A", b"A", 0)):
        assert swref.last_index(ref, seq) == want and L.swref_last_index(ref, len(ref), seq, len(seq)) == want, (ref, seq)


def test_shortcut_cases():
    """ACGTACGT / ACGT: ACGT stands at 0 and at 4, lastIndex starts at r = 4: 4M, offset 4.
    acgt / ACGT: the reference byte is upper-cased, the alternate is raw: a fit at 0.  acgt / acgt: 'A' != 'a' everywhere, no fit; the DP
    compares raw bytes (:169), four matches on the diagonal: 10, 20, 30, 40; the last column's best is row 4 (40), the bottom row's
    best is the same cell (not strictly closer): p1 = p2 = 4, four diagonal steps, 4M, offset p1 = 0.
    ARGT / ANGT: R -> N fits the raw N.  ARGT / ARGT: N != 'R', no fit, the DP again matches raw R with raw R: 4M, 0."""
    assert both(b"ACGTACGT", b"ACGT", P1, SOFTCLIP) == ("4M", 4)
    assert both(b"acgt", b"ACGT", P1, SOFTCLIP) == ("4M", 0)
    assert both(b"acgt", b"acgt", P1, SOFTCLIP) == ("4M", 0)
    assert both(b"ARGT", b"ANGT", P1, SOFTCLIP) == ("4M", 0)
    assert both(b"ARGT", b"ARGT", P1, SOFTCLIP) == ("4M", 0)
    assert both(b"ACGTACGT", b"ACGT", P1, IGNORE) == ("4M", 4)
    assert both(b"ACGTACGT", b"ACGT", P1, INDEL) == ("4D4M", 0)  # no shortcut: from the corner, the diagonal to (4, 0), then p1 = 4 > 0: 4D


def test_one_mismatch_stays_on_the_diagonal():
    """ACGTACGTAC / ACGTTCGTAC, P1: the diagonal scores 10, 20, 30, 40, 25 (-15), 35, .., 75 at (10, 10).  A gap instead of the mismatch
    costs -30 - 5 twice over (a deletion and an insertion, to stay on the diagonal): far below -15.  End search: 75 at the corner is the
    last column's maximum and the bottom row's: 10M, offset 0."""
    assert both(b"ACGTACGTAC", b"ACGTTCGTAC", P1, SOFTCLIP) == ("10M", 0)


def test_leading_insertion_before_the_match():
    """AAAACCCCGGGG / TTTTCCCCGGGG, P1 softclip.  CCCCGGGG against CCCCGGGG: the diagonal through (5, 5) .. (12, 12) collects 80 on top of
    cell (4, 4).  Row 4 / column 4 hold nothing better than 0 (softclip's first row and column are 0, T never matches A or C), and the
    cheapest way into (5, 5) is the diagonal from (4, 4) = max(cutoff, ..) - the mismatches TTTT/AAAA at -15 each lose against the gap
    chain that the zero first column feeds: cell (4, 4) is reached by `right` from (4, 0) = 0 with -30 - 3 * 5 = -45 (ki = 4) against the
    diagonal's -60.  The traceback from (12, 12): eight diagonal steps to (4, 4), backtrack -4: I of 4, p2 = 0, stop.  Tail: p2 = 0, no S;
    offset p1 = 4.  Reversed: 4I 8M."""
    assert both(b"AAAACCCCGGGG", b"TTTTCCCCGGGG", P1, SOFTCLIP) == ("4I8M", 4)


REF_D, ALT_D = b"ACGTACGTTTGACCAGTACA", b"ACGTACGTACCAGTACA"  # ACGTACGT + TTG + ACCAGTACA against ACGTACGT + ACCAGTACA


def test_a_deletion_of_three():
    """P2 (25, -50, -110, -6): 8 matches = 200 at (8, 8); the deletion of TTG costs -110 - 2 * 6 = -122 (kd = 3 at row 11), nine more
    matches: 200 - 122 + 225 = 303 at (20, 17).  Without the gap the alternate's ACCAGTACA would meet TTGACCAGT: at most 2 matches in 9, far
    below.  leadingIndel: the last column's maximum is row 20; the traceback walks 9 diagonal cells to (11, 8), reads kd = 3: D, p1 = 8, 8
    diagonal cells to (0, 0).  8M 3D 9M, offset 0 by definition.  ignore: no exact occurrence (17 bytes never stand in the reference), same
    path, p2 = 0 is folded in: 8M 3D 9M, offset p1 - p2 = 0.  P3 (200, -150, -260, -11), softclip: 1600 - 282 + 1800: the same path.
    Swapped, the gap is an insertion (-ki = -3 in row 8): 8M 3I 9M under leadingIndel and indel."""
    assert both(REF_D, ALT_D, P2, LEADING_INDEL) == ("8M3D9M", 0)
    assert both(REF_D, ALT_D, P2, IGNORE) == ("8M3D9M", 0)
    assert both(REF_D, ALT_D, P3, SOFTCLIP) == ("8M3D9M", 0)
    assert both(ALT_D, REF_D, P2, LEADING_INDEL) == ("8M3I9M", 0)
    assert both(ALT_D, REF_D, P2, INDEL) == ("8M3I9M", 0)


def test_overhang_on_both_sides():
    """ACG / TACGT, P1.  softclip: ACG matches columns 2..4 on the diagonal from (0, 1) = 0: 10, 20, 30 at (3, 4).  Cell (3, 5): `right`
    from (3, 4) gives 30 - 30 = 0 with ki = 1; the diagonal comes from (2, 4) = -10 (itself `right` of (2, 3) = 20) and gives -25: the
    cell is 0, backtrack -1.  The last column's other rows hold less than 0, so it gives p1 = 3 with 0.  The bottom row then finds 30
    at j = 4 > 0: p1 = 3, p2 = 4, segmentLength = 5 - 4 = 1 -> a leading 1S.  Three diagonal steps to (0, 1): stop.  Tail: 3M pushed,
    p2 = 1 > 0: 1S; offset p1 = 0.  Reversed: 1S 3M 1S.
    leadingIndel: first row and column are -30, -35, ..; the diagonal from (0, 1) = -30 gives -20, -10, 0 at (3, 4) and (3, 5) = -30 by
    `right`, the last column's best; the bottom row is not searched.  The traceback reads -1 at (3, 5): I, then three diagonal steps
    to (0, 1), tail p1 = 0, p2 = 1: 1I.  Reversed: 1I 3M 1I, offset 0."""
    assert both(b"ACG", b"TACGT", P1, SOFTCLIP) == ("1S3M1S", 0)
    assert both(b"ACG", b"TACGT", P1, LEADING_INDEL) == ("1I3M1I", 0)


@pytest.mark.parametrize("params", [P1, P2, P3, (0, 0, 0, 0), (1, -1, 5, 5)])
def test_one_by_one(params):
    """A / C: one cell.  The shortcut misses.  Whatever wins the cell, the traceback makes one step from (1, 1): diagonal -> state M,
    length 1, (0, 0): 1M; a gap is only taken if strictly better than the diagonal AND then p1 or p2 stays 1 ... with the three parameter
    sets the mismatch (-15, -50, -150) beats open (-30, -110, -260): 1M, offset 0 under every strategy.  (0, 0, 0, 0): all equal, the
    diagonal wins.  (1, -1, 5, 5): a gap wins the cell - stated here so that the table's "any" is not read as "every": -1 < 0 + 5; right
    >= down: I of 1, p2 = 0; softclip's tail: 1I and offset p1 = 1."""
    if params == (1, -1, 5, 5):
        assert both(b"A", b"C", params, SOFTCLIP) == ("1I", 1)
        return
    for s in ALL:
        assert both(b"A", b"C", params, s) == ("1M", 0)


def test_the_clean_up_does_not_look_back_after_a_removal():
    """:302-311 on [3M 0D 2M]: i = 1: 3M is not empty, M != D: i = 2; lce[1] = 0D is empty: removed, i stays 2 = len: the loop ends with
    3M 2M unmerged.  Reached through the public function by a traceback that leaves a zero-length segment between two equal ones is
    rare; the random comparison below holds both restatements and the device's one-pass form (sw_core.hpp: sw_clean) to the loop as
    written, and this case pins the Python loop itself."""
    lce = [[3, "M"], [0, "D"], [2, "M"]]
    i = 1
    while i < len(lce):
        if lce[i - 1][0] == 0:
            del lce[i - 1]
        elif lce[i - 1][1] == lce[i][1]:
            lce[i - 1][0] += lce[i][0]
            del lce[i]
        else:
            i += 1
    assert lce == [[3, "M"], [2, "M"]]


def test_the_two_agree_on_random_problems_and_keep_the_stated_properties():
    """24 000 problems over two letters, lengths 1..14, the four strategies, the three parameter sets and three random ones each: equal
    CIGARs and offsets; at most len(ref) + len(alt) + 2 operations; no operation of length 0; only M, I, D, S; no two neighbours with the
    same operation (the loop's blind spot above needs a zero-length segment between two equal ones; the traceback only ever makes a
    zero-length M, next to a gap and an S)."""
    n = 0
    for case in sw_cases.small_random(24000, seed=123):
        cigar_off, cigar, offset = sw_cases.expected(case)
        for k in range(len(case.ref_of)):
            ref, alt = case.refs[k], case.alts[k]
            py, off = swref.run_smith_waterman(ref, alt, case.params, case.strategy)
            words = cigar[int(cigar_off[k]):int(cigar_off[k + 1])]
            assert swref.encode(py) == [int(w) for w in words] and off == int(offset[k]), (case.name, ref, alt)
            assert len(py) <= len(ref) + len(alt) + 2
            assert all(ln > 0 and op in "MIDS" for ln, op in py), (case.name, ref, alt, py)
            assert not any(py[i][1] == py[i + 1][1] for i in range(len(py) - 1)), (case.name, ref, alt, py)
            n += 1
    assert n >= 20000
