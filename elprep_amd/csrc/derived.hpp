// derived.hpp — which of a context's derived data is still valid for its staged records, and the one table that says what a change
// to the staged data spoils.  Plain C++17, nothing of HIP: tests/derived_host.cpp builds it with the host compiler.
#pragma once

#include <cstdint>

namespace elp {

// What every derived item is computed from.  This table is the specification; the events below follow from it.
//
//   item                                             computed from
//   ------------------------------------------------ ------------------------------------------------------------------------------
//   keys: key, upos, key_bits                        POS, REFID, FLAG (strand, unmapped), CIGAR, has_sr; n_ref, max_pos
//   scores: score, qbounds, and of the score kernel  QUAL, FLAG (who is a candidate), rgid and the header's covariates (apply_recs),
//     of the same adapt stage its error word           the one-length fact, tuning "score_kernel"
//     (adapt_pending, adapt_bad_qual), its quality
//     sample (adapt_sampled) and ApplyBQSR's
//     records (apply_recs_valid)
//   permutation: perm (sorted; sorted_qname = it is  coordinate: keys, then QNAME, FLAG, MAPQ, RNEXT, PNEXT, TLEN
//     in queryname order; sorted_keep = it is in     queryname: QNAME, has_sr
//     input order, sorted_keep_by_split = ... split  keep (elp_order_keep): has_sr; with by_split also the split ids
//     file after split file)
//   presort: the sort's key passes made ahead        the key column (keys)
//   marks: FLAG's duplicate bit, mate, pair_win      keys (upos), scores, REFID, FLAG, rgid -> library, split ids, QNAME
//   quality hint: qual_present                       QUAL (a sample, or the score kernel's), tuning "qual_hint", "qual_hint_drop"
//   snapshot: snap_flag, snap_qual                   a copy of FLAG and QUAL of the n records staged when it was taken, under the
//                                                    dictionary (REFID, RNEXT numbering, n_ref) in force at that time
//   tile index: tile_first                           the QUAL offsets (n, qual_bytes)
//   one-length fact: uniform_len                     the QUAL and SEQ offsets, l_seq (n, qual_bytes)
//
// The sub-items of the scores are read only while `scores` holds; an event that spoils the scores clears them with it.
//
// Deliberate exceptions - sites that clear less than the table suggests, kept as they are:
//   * elp_mark_duplicates rewrites FLAG's duplicate bit and raises no event: an existing coordinate permutation stays valid although
//     the comparator reads FLAG (a host that wants the reference's order sorts behind mark duplicates; the bench's sort-ahead makes
//     only the key passes early, the tie-break runs behind the final FLAGs).  Keys and scores do not read that bit.
//     elp_clear_duplicate_flag, which takes the bit away in front of duplicate marking, does raise one (duplicate_bit_cleared: the marks
//     and any permutation go - the comparator's modFlag tie-break read the bit; keys, the key passes made ahead and scores stay).
//   * qual_changed() (elp_bqsr_apply) keeps the marks although they were decided with the scores of the old qualities: the marks are
//     the result the reference computes BEFORE it recalibrates, not a cache of the current QUAL column.
//   * header_changed() (elp_set_header) clears apply_recs only, although the keys hold n_ref and the marks the libraries: a header is
//     set before records are staged (elp_stage refuses without one), and staging clears everything.
//   * No event clears the snapshot but records_changed() and dictionary_replaced(): it is a copy to return to, not a function of the
//     current columns.  dictionary_replaced() (elp_replace_reference_dictionary) rewrites REFID / RNEXT, the record states and n_ref: what
//     fixed_fields_changed() and header_changed() spoil goes (the keys with the key passes made ahead of them, scores, permutation,
//     marks, ApplyBQSR's records), and the snapshot too - a rollback restores FLAG and QUAL, not the refids they were decided under.
//   * duplicate_bit_cleared() and flag_qual_restored() drop a keep permutation too although it reads neither FLAG nor QUAL: one rule for
//     every kind of permutation (conservative; elp_order_keep is cheap to repeat).
//   * Tuning "score_kernel" clears the scores only (with one `adapted` flag it took the keys along, which do not depend on it).
struct Derived {
  bool keys = false;
  bool scores = false;
  bool adapt_pending = false;      // the score kernel's error word (adapt_err) has not been read yet ...
  bool adapt_bad_qual = false;     // ... it has, and the kernel met a quality > 93 in a duplicate-marking candidate
  bool adapt_sampled = false;      // the score kernel sampled the quality values (adapt_qmask once the words have been read)
  bool apply_recs_valid = false;   // the score kernel wrote ApplyBQSR's per-read records (apply_rec.hpp)
  bool presorted = false;          // the coordinate sort's key passes were made ahead from the key column as it is (sort_presort)
  bool sorted = false;
  bool sorted_qname = false;       // the permutation is in queryname order (elp_sort_queryname), not coordinate order
  bool sorted_keep = false;        // the permutation is in input order (elp_order_keep): no sort made it ...
  bool sorted_keep_by_split = false;  // ... with the records of one split id behind those of the smaller ids (by_split != 0)
  bool marked = false;
  bool have_qual_present = false;
  bool have_snapshot = false;
  uint64_t flat_index_n = 0, flat_index_bytes = 0;         // the record set the tile index was made for (valid: equal to n, qual_bytes)
  uint64_t uniform_n = ~0ull, uniform_bytes = ~0ull;       // ... the one-length fact was established for

  bool adapted() const { return keys && scores; }
  bool has_flat_index(uint64_t n, uint64_t qual_bytes) const { return flat_index_n == n && flat_index_bytes == qual_bytes && n; }
  bool has_uniform(uint64_t n, uint64_t qual_bytes) const { return uniform_n == n && uniform_bytes == qual_bytes && n; }

  // ---- items becoming valid where a flag alone would allow an inconsistent pair
  void set_sorted(bool by_qname) { sorted = true; sorted_qname = by_qname; sorted_keep = sorted_keep_by_split = false; }
  void set_sorted_keep(bool by_split) { sorted = sorted_keep = true; sorted_keep_by_split = by_split; sorted_qname = false; }
  void adapt_word_read(bool bad_qual) { adapt_pending = false; if (bad_qual) adapt_bad_qual = true; }  // adapt_note

  // ---- items dropped by the stage that is about to recompute them (and by the events)
  void drop_scores() { scores = adapt_pending = adapt_bad_qual = adapt_sampled = apply_recs_valid = false; }
  void drop_sorted() { sorted = sorted_qname = sorted_keep = sorted_keep_by_split = false; }
  void drop_marked() { marked = false; }
  void drop_qual_hint() { have_qual_present = false; }
  void drop_presort() { presorted = false; }
  void drop_keys() { keys = false; drop_presort(); }
  // the adapt stage starts: key column and scores are about to be rewritten (sorted words made from the old column are stale)
  void adapt_begins() { drop_keys(); drop_scores(); }

  // ---- events: one per kind of change to the staged data
  void records_changed() {  // count or any column: elp_reset, elp_stage, the BAM / BGZF staging calls, the exchange's receiving side
    fixed_fields_changed();
    drop_qual_hint();
    have_snapshot = false;
    flat_index_n = 0;
    uniform_n = ~0ull;
  }
  void fixed_fields_changed() { drop_keys(); drop_scores(); drop_sorted(); drop_marked(); }  // MAPQ / CIGAR / has_sr: elp_clean_sam, elp_filter_records
  void qual_changed() { drop_scores(); drop_qual_hint(); }                                    // elp_bqsr_apply.  NOT the keys
  void flag_qual_restored() { fixed_fields_changed(); drop_qual_hint(); }                     // elp_rollback
  void split_changed() { drop_marked(); if (sorted_keep_by_split) drop_sorted(); }            // elp_split_classify (a keep permutation by split was made from the ids)
  void duplicate_bit_cleared() { drop_sorted(); drop_marked(); }                              // elp_clear_duplicate_flag.  NOT keys / scores
  void dictionary_replaced() { fixed_fields_changed(); header_changed(); have_snapshot = false; }  // elp_replace_reference_dictionary: REFID, RNEXT, has_sr, n_ref
  void radix_timed_out() { drop_sorted(); drop_marked(); }                                    // fetch_err: whichever sort it was, its result is wrong
  void qual_hint_refuted() { drop_qual_hint(); }                                              // the gather's retry path
  void header_changed() { apply_recs_valid = false; }                                         // elp_set_header
  void score_tuning_changed() { drop_scores(); }                                              // elp_set_tuning "score_kernel"
  void hint_tuning_changed() { drop_qual_hint(); }                                            // elp_set_tuning "qual_hint", "qual_hint_drop"
};

}  // namespace elp
