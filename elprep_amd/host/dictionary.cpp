// dictionary.cpp — the host half of --replace-reference-sequences: from the @SQ names of the old and the new dictionary, the index map
// elp_replace_reference_dictionary takes and the verdict on @HD SO.  Reference: filters/simple-filters.go:32-60
// (ReplaceReferenceSequenceDictionary), :208-231 (AddREFID).
#include <cstdint>
#include <string_view>
#include <unordered_map>

#include "../../include/elprep_host.h"

namespace {
std::string_view name_at(const uint8_t *names, const uint32_t *off, int32_t k) {
  return std::string_view(reinterpret_cast<const char *>(names) + off[k], off[k + 1] - off[k]);
}
}  // namespace

extern "C" int elp_host_dictionary_map(const uint8_t *old_names, const uint32_t *old_off, int32_t n_old, const uint8_t *new_names, const uint32_t *new_off,
                                       int32_t n_new, int32_t *new_of_old, int *order_kept_out) {
  if (n_old < 0 || n_new < 0 || (n_old && (!old_off || !new_of_old)) || (n_new && !new_off)) return -1;
  for (int32_t k = 0; k < n_old; k++)
    if (old_off[k + 1] < old_off[k] || (old_off[k + 1] > old_off[k] && !old_names)) return -1;
  for (int32_t k = 0; k < n_new; k++)
    if (new_off[k + 1] < new_off[k] || (new_off[k + 1] > new_off[k] && !new_names)) return -1;
  // AddREFID's dictTable (:209-213): later entries of a name overwrite earlier ones - the LAST index wins
  std::unordered_map<std::string_view, int32_t> last_new;
  last_new.reserve((size_t)n_new * 2);
  for (int32_t k = 0; k < n_new; k++) last_new[name_at(new_names, new_off, k)] = k;
  for (int32_t r = 0; r < n_old; r++) {
    const auto it = last_new.find(name_at(old_names, old_off, r));
    new_of_old[r] = it == last_new.end() ? -1 : it->second;
  }
  if (order_kept_out) {
    // :36-51: utils.Find gives the FIRST old entry of the name; the walk ends at the first found position that does not ascend
    std::unordered_map<std::string_view, int32_t> first_old;
    first_old.reserve((size_t)n_old * 2);
    for (int32_t r = n_old - 1; r >= 0; r--) first_old[name_at(old_names, old_off, r)] = r;
    int kept = 1;
    int32_t previous = -1;
    for (int32_t k = 0; k < n_new; k++) {
      const auto it = first_old.find(name_at(new_names, new_off, k));
      if (it == first_old.end()) continue;
      if (it->second > previous) previous = it->second;
      else { kept = 0; break; }
    }
    *order_kept_out = kept;
  }
  return 0;
}
