// derived_events_host.cpp — the events of elprep_amd/csrc/derived.hpp that tests/derived_host.cpp does not know, behind the same kind of C
// function, for tests/test_derived_events_cpu.py: from "everything valid" for 100 records / 1000 QUAL bytes, raise one event and report
// what is still valid (same bit order as derived_host.cpp).
#include <string_view>

#include "../elprep_amd/csrc/derived.hpp"

static unsigned mask(const elp::Derived &d, uint64_t n, uint64_t qb) {
  const bool items[12] = {d.keys, d.scores, d.scores && d.adapt_sampled, d.scores && d.apply_recs_valid, d.sorted, d.sorted_qname, d.presorted, d.marked,
                          d.have_qual_present, d.have_snapshot, d.has_flat_index(n, qb), d.has_uniform(n, qb)};
  unsigned m = 0;
  for (int k = 0; k < 12; k++) m |= items[k] ? 1u << k : 0u;
  return m;
}

extern "C" unsigned derived_events_valid_after(const char *event) {
  const uint64_t n = 100, qb = 1000;
  elp::Derived d;
  d.keys = d.scores = d.adapt_sampled = d.apply_recs_valid = d.presorted = d.marked = d.have_qual_present = d.have_snapshot = true;
  d.set_sorted(true);
  d.flat_index_n = d.uniform_n = n;
  d.flat_index_bytes = d.uniform_bytes = qb;
  const std::string_view e(event);
  if (e == "") {}
  else if (e == "dictionary_replaced") d.dictionary_replaced();
  else if (e == "duplicate_bit_cleared") d.duplicate_bit_cleared();
  else return ~0u;
  return mask(d, n, qb);
}
