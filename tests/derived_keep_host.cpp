// derived_keep_host.cpp — the permutation items of elprep_amd/csrc/derived.hpp behind one C function, for tests/test_keep_order_cpu.py:
// from "everything valid" with a permutation of the given kind, raise one event and report which permutation items are still set.
#include <string_view>

#include "../elprep_amd/csrc/derived.hpp"

enum : unsigned { SORTED = 1, SORTED_QNAME = 2, SORTED_KEEP = 4, SORTED_KEEP_BY_SPLIT = 8, MARKED = 16, KEYS = 32 };

// start: "coordinate", "queryname", "keep", "keep_by_split".  -> the mask of the items above that hold after `event` ("" = no event), or
// ~0u for an unknown start or event
extern "C" unsigned derived_keep_after(const char *start, const char *event) {
  elp::Derived d;
  d.keys = d.scores = d.adapt_sampled = d.apply_recs_valid = d.presorted = d.marked = d.have_qual_present = d.have_snapshot = true;
  const std::string_view s(start), e(event);
  if (s == "coordinate") d.set_sorted(false);
  else if (s == "queryname") d.set_sorted(true);
  else if (s == "keep") d.set_sorted_keep(false);
  else if (s == "keep_by_split") d.set_sorted_keep(true);
  else return ~0u;
  if (e == "") {}
  else if (e == "records_changed") d.records_changed();
  else if (e == "fixed_fields_changed") d.fixed_fields_changed();
  else if (e == "qual_changed") d.qual_changed();
  else if (e == "flag_qual_restored") d.flag_qual_restored();
  else if (e == "split_changed") d.split_changed();
  else if (e == "duplicate_bit_cleared") d.duplicate_bit_cleared();
  else if (e == "dictionary_replaced") d.dictionary_replaced();
  else if (e == "radix_timed_out") d.radix_timed_out();
  else if (e == "qual_hint_refuted") d.qual_hint_refuted();
  else if (e == "header_changed") d.header_changed();
  else if (e == "score_tuning_changed") d.score_tuning_changed();
  else if (e == "hint_tuning_changed") d.hint_tuning_changed();
  else if (e == "adapt_begins") d.adapt_begins();
  else if (e == "drop_sorted") d.drop_sorted();
  else if (e == "set_sorted_coordinate") d.set_sorted(false);
  else if (e == "set_sorted_queryname") d.set_sorted(true);
  else if (e == "set_sorted_keep") d.set_sorted_keep(false);
  else if (e == "set_sorted_keep_by_split") d.set_sorted_keep(true);
  else return ~0u;
  return (d.sorted ? SORTED : 0) | (d.sorted_qname ? SORTED_QNAME : 0) | (d.sorted_keep ? SORTED_KEEP : 0) |
         (d.sorted_keep_by_split ? SORTED_KEEP_BY_SPLIT : 0) | (d.marked ? MARKED : 0) | (d.keys ? KEYS : 0);
}
