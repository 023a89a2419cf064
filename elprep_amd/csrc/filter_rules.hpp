// filter_rules.hpp — the per-record rules of the filters next to the hot path and of the split / merge bookkeeping, and the scratch
// layouts and grids of their entry points, as host-and-device code in the manner of optical_name.hpp / samparse.hpp: the kernels of
// filter.hip, clean_sam.hip, dictionary.hip, split_merge.hip and split.hip and the host build the CPU tests compile
// (tests/filter_rules_host.cpp) run the same functions.  How a record's columns and bytes are fetched stays with the caller.  Nothing
// here touches the device or needs common.hpp; the header compiles with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bamtag_read.hpp"

#if defined(__HIPCC__)
#define ELP_RULES_HD __host__ __device__ __forceinline__
#else
#define ELP_RULES_HD inline
#endif

namespace elp {

// the FLAG bits and CIGAR operators the rules read, under names of their own (common.hpp's F_* / OP_* and op_consumes_* need HIP; the
// .hip files assert that the numbers agree)
constexpr uint16_t RULE_UNMAPPED = 0x4, RULE_DUPLICATE = 0x400;
constexpr uint32_t RULE_OP_M = 0, RULE_OP_I = 1, RULE_OP_D = 2, RULE_OP_N = 3, RULE_OP_S = 4, RULE_OP_EQ = 7, RULE_OP_X = 8;
ELP_RULES_HD bool rule_consumes_read(uint32_t op) { return op == RULE_OP_M || op == RULE_OP_I || op == RULE_OP_S || op == RULE_OP_EQ || op == RULE_OP_X; }
ELP_RULES_HD bool rule_consumes_ref(uint32_t op) { return op == RULE_OP_M || op == RULE_OP_D || op == RULE_OP_N || op == RULE_OP_EQ || op == RULE_OP_X; }

// ---------------- the fused predicates (filters/simple-filters.go)

// intervals.Overlap, intervals/intervals.go:146-160 (binary search, same comparisons); iv = [n][2] Start, End sorted by Start
ELP_RULES_HD bool overlap(const int32_t *iv, int64_t n, int32_t start, int32_t end) {
  int64_t left = 0, right = n - 1;
  while (left <= right) {
    const int64_t mid = (left + right) / 2;
    const int32_t is = iv[2 * mid], ie = iv[2 * mid + 1];
    if (is > end - 1) right = mid - 1;
    else if (ie <= start - 1) left = mid + 1;
    else return true;
  }
  return false;
}

// what the rules ask of a CIGAR: reference and read bases consumed, and whether every operator is M or S (the others - I D N H P X = -
// are nonExactMappingOperator's, :90-99)
struct CigarFacts {
  int32_t ref_len, read_len;
  bool exact;
};
ELP_RULES_HD CigarFacts cigar_facts(const uint32_t *ops, uint64_t nop) {
  CigarFacts c{0, 0, true};
  for (uint64_t k = 0; k < nop; k++) {
    const uint32_t op = ops[k] & 0xF;
    const int32_t ln = (int32_t)(ops[k] >> 4);
    if (op != RULE_OP_M && op != RULE_OP_S) c.exact = false;
    if (rule_consumes_ref(op)) c.ref_len += ln;
    if (rule_consumes_read(op)) c.read_len += ln;
  }
  return c;
}

// Whether the selected predicates reject a record: RemoveUnmappedReads :73-75, RemoveUnmappedReadsStrict :79-83,
// RemoveMappingQualityLessThan :332-347 (a bound over 255 rejects everything), RemoveDuplicateReads :136-138,
// RemoveNonExactMappingReads :90-99, RemoveNonOverlappingReads :310-328 - the region test only on records the others kept.
// p: the six switches of elp_predicates (any struct that has them).  mapq() -> the record's MAPQ and cigar() -> its CigarFacts are
// called only where a selected predicate reads them.  regions[r] / n_regions[r]: the intervals of refid r, r < n_ref.
template <class P, class Mapq, class Cigar>
ELP_RULES_HD bool record_rejected(const P &p, uint16_t f, int32_t r, int32_t ps, Mapq mapq, Cigar cigar, int32_t n_ref,
                                  int32_t *const *regions, const int64_t *n_regions) {
  bool drop = false;
  if (p.remove_unmapped && (f & RULE_UNMAPPED)) drop = true;
  if (p.remove_unmapped_strict && ((f & RULE_UNMAPPED) || ps == 0 || r < 0)) drop = true;
  if (p.min_mapq > 0 && (p.min_mapq > 255 || (int)mapq() < p.min_mapq)) drop = true;
  if (p.remove_duplicates && (f & RULE_DUPLICATE)) drop = true;
  if (!drop && (p.remove_non_exact || p.use_regions)) {
    const CigarFacts c = cigar();
    if (p.remove_non_exact && !c.exact) drop = true;
    if (!drop && p.use_regions) {
      int32_t a_end = ps;  // :318-324
      if (!(f & RULE_UNMAPPED) && c.read_len > 0) a_end = ps + c.ref_len - 1;
      drop = !(r >= 0 && r < n_ref && overlap(regions[r], n_regions[r], ps, a_end));
    }
  }
  return drop;
}

// ---------------- RemoveNonExactMappingReadsStrict (:115-134): keep iff the FIRST field of key X0 exists and is 1, then likewise X1, XM,
// XO, XG exist and are 0 - tested in this order, stopping at the first test that fails (TAGS.Get returns the first entry of a key,
// utils/small-map.go:45-52).  A tested field that is no integer makes the reference panic on x.(int64).
struct StrictBits {
  uint32_t found, not_int, wrong;  // bit w: the first field of key w (X0 X1 XM XO XG) exists / is no integer / has another value
};
// the first optional field of a BAM record (rec: behind its block_size field)
ELP_RULES_HD const uint8_t *bam_fields_at(const uint8_t *rec) {
  const uint32_t l_name = rec[8], n_cig = ld_u16(rec + 12), l_seq = ld_u32(rec + 16);
  return rec + (32ull + l_name + 4ull * n_cig + ((l_seq + 1) >> 1) + l_seq);
}
// the walk over a record's optional fields [t, end); it stops at a field that does not fit (staging has checked every record's fields,
// so on staged records it ends at `end`)
ELP_RULES_HD StrictBits strict_walk(const uint8_t *t, const uint8_t *end) {
  StrictBits b{0, 0, 0};
  while (t + 3 <= end) {
    const uint8_t k0 = t[0], k1 = t[1], ty = t[2];
    const uint8_t *v = t + 3;
    const uint32_t sz = tag_value_size(ty, v, end);
    if (!sz || sz > (uint64_t)(end - v)) break;  // (a value of fixed size that the record cuts short is not read)
    if (k0 == 'X') {
      const int w = k1 == '0' ? 0 : (k1 == '1' ? 1 : (k1 == 'M' ? 2 : (k1 == 'O' ? 3 : (k1 == 'G' ? 4 : -1))));
      if (w >= 0 && !((b.found >> w) & 1u)) {
        b.found |= 1u << w;
        if (!tag_is_int(ty)) b.not_int |= 1u << w;
        else if (tag_int_value(ty, v) != (w == 0 ? 1 : 0)) b.wrong |= 1u << w;
      }
    }
    t = v + sz;
  }
  return b;
}
enum : int { STRICT_KEEP = 0, STRICT_REJECT = 1, STRICT_PANICS = 2 };
// the ordered five-key decision: the first key that is missing or wrong-valued rejects, one that is no integer in front of it panics
ELP_RULES_HD int strict_decide(StrictBits b) {
  int rule = STRICT_KEEP;
  for (int w = 0; w < 5 && rule == STRICT_KEEP; w++) {
    if (!((b.found >> w) & 1u)) rule = STRICT_REJECT;
    else if ((b.not_int >> w) & 1u) rule = STRICT_PANICS;
    else if ((b.wrong >> w) & 1u) rule = STRICT_REJECT;
  }
  return rule;
}

// ---------------- CleanSam (:292-306): an alignment that ends behind its reference sequence is soft-clipped there by softClipEndOfRead
// (filters/utils.go:102-119) - restated with its arithmetic as it stands: the running position accumulates (`pos += endPos`, :116) and
// the clip's length is ReadLengthFromCigar + clipFrom (:112); a drop-in must write what the reference writes.

// referenceSequenceTable[aln.RNAME] (simple-filters.go:300): a Go map - RNAME '*' or a name the header does not have gives length 0, so a
// read with the mapped flag and no reference (End() > 0) is soft-clipped from its first base on
ELP_RULES_HD int32_t clean_length(const int32_t *ref_len, int32_t n_ref, int32_t r) { return (r >= 0 && r < n_ref) ? ref_len[r] : 0; }

// the new CIGAR of a record (out may be null: count only); returns the number of operations, -1: the reference panics, -2: a length the
// 28-bit BAM field cannot hold; *changed = the record is rewritten.  length: clean_length of the record's refid
ELP_RULES_HD int clean_cigar(const uint32_t *ops, int nop, uint16_t f, int32_t rec_pos, int32_t length, uint32_t *out, bool *changed) {
  *changed = false;
  bool clip = false;
  int32_t clip_from = 0, read_len = 0;
  if (!(f & RULE_UNMAPPED)) {
    const CigarFacts c = cigar_facts(ops, (uint64_t)nop);
    read_len = c.read_len;
    const int32_t end = rec_pos + c.ref_len - 1;  // Alignment.End, sam/sam-types.go:769-775
    if (end > length) { clip = true; clip_from = length - rec_pos + 1; }
  }
  if (!clip) {
    if (out) for (int k = 0; k < nop; k++) out[k] = ops[k];
    return nop;
  }
  *changed = true;
  int32_t pos = 0;
  clip_from--;
  int n_new = 0;
  for (int k = 0; k < nop; k++) {
    const uint32_t op = ops[k], o = op & 15u;
    const int32_t end_pos = pos + (rule_consumes_read(o) ? (int32_t)(op >> 4) : 0);
    if (end_pos < clip_from) {
      if (out) out[n_new] = op;
      n_new++;
    } else {
      int32_t clipped = read_len + clip_from;
      const int32_t rel = clip_from - pos;
      if (rule_consumes_read(o)) {
        if (rule_consumes_ref(o)) {
          if (rel > 0) {
            if (rel >= (1 << 28)) return -2;
            if (out) out[n_new] = ((uint32_t)rel << 4) | o;
            n_new++;
          }
        } else {
          clipped += rel;
        }
      } else if (rel != 0) {
        return -1;  // "Unexpected non-0 relative clipping position in CleanSam." (filters/utils.go:93)
      }
      if (clipped < 0 || clipped >= (1 << 28)) return -2;
      if (out) out[n_new] = ((uint32_t)clipped << 4) | RULE_OP_S;
      n_new++;
      break;
    }
    pos += end_pos;
  }
  return n_new;
}

// ---------------- `elprep split` / `elprep merge` (sam/split-merge.go)

// SplitFilePerChromosome's routing rule (:280-293) for a record with these refids: *g = its split file - 0 for RNAME "*"
// (contigToGroup["*"] = "unmapped", :254), else group_of_ref[refid] -; returns whether it also goes to the spread file (:286: RNEXT != "=",
// which in BAM is next_refid != refid (sam/bam-files.go:344-346), RNAME != "*", and the mate's group differs - so a mapped record with RNEXT
// "*" is spread).  elp_split_classify (split_merge.hip) and the split emitters' list (split.hip) route by it.
ELP_RULES_HD bool split_route(int32_t r, int32_t nr, const int32_t *__restrict__ group_of_ref, int32_t n_ref, int32_t *g) {
  *g = (r >= 0 && r < n_ref) ? group_of_ref[r] : 0;
  const int32_t gn = (nr >= 0 && nr < n_ref) ? group_of_ref[nr] : 0;
  return nr != r && r >= 0 && gn != *g;
}

// (refid, POS) as the merge loop compares them (:417-434): refid -1 (the high word 0xFFFFFFFF) sorts behind every contig
ELP_RULES_HD uint64_t merge_key(int32_t refid, int32_t pos) { return ((uint64_t)(uint32_t)refid << 32) | (uint64_t)(uint32_t)pos; }
// the first of the ng sorted group keys that is greater than `key`: a spread read goes behind every group read with key <= its own
ELP_RULES_HD uint64_t merge_upper_bound(const uint64_t *__restrict__ kg, uint64_t ng, uint64_t key) {
  uint64_t lo = 0, hi = ng;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (kg[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---------------- scratch slot 5 of the entry points: byte offsets of every part and the bytes to ask for (16-byte steps keep the 8-byte
// parts aligned), and the grids that are not one workgroup per 256 records

inline size_t rule_align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline unsigned rule_blocks(uint64_t n, unsigned per_block) { return (unsigned)((n + per_block - 1) / per_block); }
inline unsigned rule_grid(unsigned blocks, unsigned cap) {  // max(1, min(blocks, cap))
  const unsigned g = blocks < cap ? blocks : cap;
  return g ? g : 1u;
}

// elp_filter_records with regions: the interval pool ([total][2] int32) | per refid a pointer into it | per refid its interval count
struct RegionLayout {
  size_t pool, ptr, cnt, bytes;
  RegionLayout(size_t total_intervals, int32_t n_ref)
      : pool(0), ptr(rule_align16(total_intervals * 8)), cnt(ptr + (size_t)n_ref * sizeof(int32_t *)), bytes(total_intervals * 8 + (size_t)n_ref * 16 + 64) {}
};
// elp_split_classify: group_of_ref (int32 per contig) | counts (n_groups + 2 of 64 bits: unmapped, groups, spread) | split (uint16 per
// record, + 8) | spread (a byte per record)
struct ClassifyLayout {
  size_t n_counts, gof, counts, split, spread, bytes;
  ClassifyLayout(uint64_t n, int32_t n_ref, int32_t n_groups)
      : n_counts((size_t)n_groups + 2), gof(0), counts(rule_align16((size_t)n_ref * 4)), split(counts + n_counts * 8), spread(split + ((size_t)n + 8) * 2),
        bytes((size_t)n_ref * 4 + n_counts * 8 + (size_t)n * 3 + 64) {}
  static unsigned grid(uint64_t n) { const unsigned b = rule_blocks(n, 256); return b < 2048u ? b : 2048u; }  // (not called for n = 0)
};
// elp_replace_reference_dictionary: two 64-bit counters (rejected, rejected tagged copies) | the map (int32 per old contig)
struct DictionaryLayout {
  size_t counters, map, bytes;
  explicit DictionaryLayout(int32_t n_old) : counters(0), map(16), bytes((size_t)n_old * 4 + 64) {}
  static unsigned grid(uint64_t n, int n_cu) { return rule_grid(rule_blocks(n, 256), (unsigned)n_cu * 16); }  // a few workgroups per CU stride over the records
};
// elp_clear_duplicate_flag: eight flags per thread and round
inline unsigned clear_flag_grid(uint64_t n, int n_cu) { return rule_grid(rule_blocks((n + 7) / 8, 256), (unsigned)n_cu * 8); }

}  // namespace elp
