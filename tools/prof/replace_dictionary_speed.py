"""elp_replace_reference_dictionary on N reads of the c3 read set: the kernel's time from profile() (HIP events), next to
clear_duplicate_flag's on the same records in the same run (the comparable one-column pass).  usage: replace_dictionary_speed.py [reads]
Three maps, each on freshly staged records, one timed launch each behind an untimed first one: reversed (every mapped record's two refids rewritten), one contig dropped
(refids, RNEXT of the mates and the states of its records rewritten), identity (nothing written)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from elprep_amd.engine import Engine  # noqa: E402
from tools import synth  # noqa: E402

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 16_000_000
cfg = synth.config("c3")
h = cfg.header()
b = synth.generate(cfg, 0, reads // 2)
n_ref = h.n_ref
print(f"{b.n} reads, {n_ref} contigs")
e = Engine(h, 0)
ident = np.arange(n_ref, dtype=np.int32)
dropped = np.where(ident == 1, -1, ident - (ident > 1)).astype(np.int32)
maps = [("reversed", ident[::-1].copy(), h.ref_len[::-1].copy()), ("one contig dropped", dropped, np.delete(h.ref_len, 1)),
        ("identity", ident, h.ref_len)]
e.stage(b)  # both kernels once, untimed: a kernel's first launch carries the load of its code
e.clear_duplicate_flag()
e.replace_reference_dictionary(ident, h.ref_len)
for label, m, ln in maps:
    e.reset()
    e.stage(b)
    e.sync()
    e.profile_enable(True)
    e.profile_reset()
    e.clear_duplicate_flag()
    n_rej = e.replace_reference_dictionary(m, ln)
    e.sync()
    p = e.profile()
    e.profile_enable(False)
    t_r, t_c = p["replace_dictionary"][1], p["clear_duplicate_flag"][1]
    written = 4 * int((b.refid >= 0).sum() + (b.next_refid >= 0).sum()) if label == "reversed" else (
        4 * int((b.refid >= 1).sum() + (b.next_refid >= 1).sum()) + int(n_rej) if label != "identity" else 0)
    moved = 9 * b.n + written
    print(f"{label}: replace_dictionary {t_r:.3f} ms ({n_rej} rejected), {moved / b.n:.1f} B/record moved = {moved / t_r / 1e9 * 1e3:.0f} GB/s = "
          f"{moved / t_r / 1e9 * 1e3 / 8000:.3f} of 8 TB/s; clear_duplicate_flag {t_c:.3f} ms, 4 B/record = {4 * b.n / t_c / 1e9 * 1e3:.0f} GB/s")
e.close()
