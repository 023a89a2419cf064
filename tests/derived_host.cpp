// derived_host.cpp — elprep_amd/csrc/derived.hpp behind one C function, for tests/test_derived_cpu.py: from "everything valid" for a
// record set of 100 records / 1000 QUAL bytes, raise one event and report what is still valid.
#include <string_view>

#include "../elprep_amd/csrc/derived.hpp"

enum : unsigned {
  KEYS = 1, SCORES = 2, SAMPLE = 4, APPLY_RECS = 8, SORTED = 16, SORTED_QNAME = 32, PRESORT = 64, MARKED = 128, QUAL_HINT = 256, SNAPSHOT = 512,
  TILE_INDEX = 1024, ONE_LENGTH = 2048
};

static unsigned mask(const elp::Derived &d, uint64_t n, uint64_t qb) {
  return (d.keys ? KEYS : 0) | (d.scores ? SCORES : 0) | (d.scores && d.adapt_sampled ? SAMPLE : 0) | (d.scores && d.apply_recs_valid ? APPLY_RECS : 0) |
         (d.sorted ? SORTED : 0) | (d.sorted_qname ? SORTED_QNAME : 0) | (d.presorted ? PRESORT : 0) | (d.marked ? MARKED : 0) |
         (d.have_qual_present ? QUAL_HINT : 0) | (d.have_snapshot ? SNAPSHOT : 0) | (d.has_flat_index(n, qb) ? TILE_INDEX : 0) |
         (d.has_uniform(n, qb) ? ONE_LENGTH : 0);
}

// -> the mask of the items still valid, or ~0u for an unknown event ("" = no event: the starting point itself)
extern "C" unsigned derived_valid_after(const char *event) {
  const uint64_t n = 100, qb = 1000;
  elp::Derived d;
  d.keys = d.scores = d.adapt_sampled = d.apply_recs_valid = d.presorted = d.marked = d.have_qual_present = d.have_snapshot = true;
  d.set_sorted(true);
  d.flat_index_n = d.uniform_n = n;
  d.flat_index_bytes = d.uniform_bytes = qb;
  const std::string_view e(event);
  if (e == "") {}
  else if (e == "records_changed") d.records_changed();
  else if (e == "fixed_fields_changed") d.fixed_fields_changed();
  else if (e == "qual_changed") d.qual_changed();
  else if (e == "flag_qual_restored") d.flag_qual_restored();
  else if (e == "split_changed") d.split_changed();
  else if (e == "radix_timed_out") d.radix_timed_out();
  else if (e == "qual_hint_refuted") d.qual_hint_refuted();
  else if (e == "header_changed") d.header_changed();
  else if (e == "score_tuning_changed") d.score_tuning_changed();
  else if (e == "hint_tuning_changed") d.hint_tuning_changed();
  else if (e == "adapt_begins") d.adapt_begins();
  else if (e == "drop_sorted") d.drop_sorted();
  else if (e == "drop_marked") d.drop_marked();
  else if (e == "drop_presort") d.drop_presort();
  else if (e == "set_sorted_coordinate") d.set_sorted(false);
  else return ~0u;
  return mask(d, n, qb);
}
