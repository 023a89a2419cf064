"""The orders of a run that does not sort, restated in numpy (test infrastructure: no device code).

    keep_order      elp_order_keep: Sam.AddNodes' StrictOrd(Slice) - input order - of the records that are output
                    (sam/filter-pipeline.go:110-112), the records that are not output behind them; by_split: split file after split file
    concat_stream   elp_emit_concat_bam's stream: MergeUnsortedFilesSplitPerChromosome (sam/split-merge.go:581-619)

state = the record-state column as the device holds it: 0 output, 1 sr-tagged copy, 2 rejected by a filter."""
import numpy as np

# sizes the GPU tests place their seams at (tests/test_keep_order_cpu.py checks them against the sources that state them)
KEEP_W = 512          # records per workgroup of the two partition kernels, csrc/keep.hip
SCAN_TILE = 2048      # counts per workgroup of exclusive_scan_u32, csrc/radix.hip (256 threads * SCAN_ITEMS)
MERGE_CHECK_W = 256   # entries per workgroup of the merge's order check, csrc/split_merge.hip


def keep_order(state, split=None, by_split=False):
    """-> (perm uint32 [n], number of output records)"""
    state = np.asarray(state)
    n_out = int((state == 0).sum())
    if not by_split:
        perm = np.concatenate([np.flatnonzero(state == 0), np.flatnonzero(state != 0)])
    else:
        key = (state != 0).astype(np.int64) * 65536 + np.asarray(split, dtype=np.int64)
        perm = np.argsort(key, kind="stable")
    return perm.astype(np.uint32), n_out


def concat_stream(g_state, g_split, s_state):
    """the source of every record of the concat stream: ("g", staging index in the groups context) or ("s", index in the spread
    context) - the groups' split 0 (the unmapped file), all of the spread, the groups' splits 1, 2, ... in id order; each part in
    staging order, output records only"""
    g_state, g_split, s_state = np.asarray(g_state), np.asarray(g_split), np.asarray(s_state)
    perm, n_out = keep_order(g_state, g_split, by_split=True)
    perm = perm[:n_out]
    first = [("g", int(i)) for i in perm if g_split[i] == 0]
    rest = [("g", int(i)) for i in perm if g_split[i] != 0]
    return first + [("s", int(j)) for j in np.flatnonzero(s_state == 0)] + rest
