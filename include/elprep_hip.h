/*
 * elprep_hip.h — C ABI of libelprep_hip.so: the MI355X (gfx950) implementation of elPrep's
 * coordinate-sort -> mark-duplicates -> optical-duplicate metrics -> BQSR gather -> BQSR apply hot path.
 *
 * This is the drop-in boundary a host program (elPrep's Go code through cgo; the C++
 * host layer in elprep_amd/host; the Python test/bench harness through ctypes) binds to.  Plain C types
 * only.  Every entry point cites the reference interface it replaces (paths relative to
 * ExaScience/elprep v5.1.3).
 *
 * Conventions
 *  - Every function returns 0 on success and a negative elp_status on error; elp_last_error(ctx) holds a
 *    message.  The reference reports all errors by log.Panic (internal/misc.go:31-43); a Go adapter turns a
 *    non-zero status into log.Panic(elp_last_error(ctx)).
 *  - One elp_ctx per GPU.  A ctx owns one HIP stream, the staged column store in HBM and all scratch.
 *    Calls on one ctx must not overlap in time, except elp_stage, which may be called from many host
 *    threads (it serialises internally; it mirrors the reference's LimitedPar batch nodes,
 *    sam/filter-pipeline.go:290-292).
 *  - Records are identified by their staging index (order of arrival = input order), 0-based.
 *  - Records that carry the sr:i tag (has_sr; the copies `elprep split` leaves in a contig-group file, sam/split-merge.go:286-293)
 *    take part in duplicate marking and are then dropped by filters.RemoveOptionalReads (filters/simple-filters.go:146-152, appended
 *    behind the mark-duplicates filter, cmd/filter.go:773,803): they never reach Sam.Alignments.  Here they stay staged, but the sort
 *    puts them behind every other record (elp_num_sorted() records are output), and the duplication metrics and BQSR ignore them.
 *  - Limits (ELP_ERR_UNSUPPORTED): 2^32-16 records per context, 4194303 bases per read, QNAMEs of at most 1000 bytes.
 *  - There is NO CPU fallback: if no gfx950 device is usable, elp_create fails.
 *  - Environment (read once per process): ELP_SYNC_SPIN=0 makes the library wait for its stream with hipStreamSynchronize instead of
 *    polling it (the default: the path waits ~15 times per pass for a few words that size the next launches, and an interrupt wake-up
 *    costs 100-200 us on a busy host; a host that runs many contexts per core may prefer to give the core up).  The host library
 *    (elprep_host.h) takes ELP_HOST_THREADS=<n>: worker threads of its table path per process (default: the hardware's, at most 16).
 */
#ifndef ELPREP_HIP_H
#define ELPREP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELP_NIL16 0xFFFFu /* "no value" for 16-bit dictionary ids (Go nil interface{} LIBID / missing RG tag) */

typedef enum elp_status {
  ELP_OK = 0,
  ELP_ERR_ARG = -1,       /* invalid argument / call order */
  ELP_ERR_HIP = -2,       /* HIP runtime error */
  ELP_ERR_NOMEM = -3,     /* out of device memory */
  ELP_ERR_DATA = -4,      /* input the reference would panic on (invalid QUAL, cycle > max_cycle, read without RG in ApplyBQSR ...) */
  ELP_ERR_UNSUPPORTED = -5 /* valid for the reference but outside this implementation's stated limits */
} elp_status;

typedef struct elp_ctx elp_ctx;

/* ---------------------------------------------------------------------------------------------------
 * Record batches: the SoA restaging of sam.Alignment (sam/sam-types.go:289-331) produced where the
 * reference batches records (InputFile.RunPipeline, sam/filter-pipeline.go:282-296; BytesToAlignment :92).
 * Fixed fields are exactly BAM's (sam/bam-files.go:299-312) after AddREFID (filters/simple-filters.go:208-231).
 * --------------------------------------------------------------------------------------------------- */
typedef struct elp_batch {
  uint64_t n;                 /* records in this batch */
  const int32_t *refid;       /* REFID temp: index of RNAME in @SQ, -1 for '*' / unknown */
  const int32_t *pos;         /* POS, 1-based */
  const int32_t *next_refid;  /* NextREFID temp ('=' already resolved) */
  const int32_t *pnext;       /* PNEXT, 1-based */
  const int32_t *tlen;        /* TLEN */
  const uint16_t *flag;       /* FLAG */
  const uint8_t *mapq;        /* MAPQ */
  const uint16_t *rgid;       /* dense id of the RG:Z tag string (index into elp_header.rg_*), ELP_NIL16 = no RG tag */
  const uint8_t *has_sr;      /* 1 = record carries the sr:i tag written by `elprep split` (sam/split-merge.go:291); may be NULL */
  const uint32_t *l_seq;      /* SEQ length in bases */
  const uint64_t *qname_off;  /* n+1 byte offsets into qname */
  const uint8_t *qname;       /* QNAME bytes, no terminator */
  const uint64_t *cigar_off;  /* n+1 offsets (in ops) into cigar */
  const uint32_t *cigar;      /* BAM-encoded ops: len<<4 | op, op indexes "MIDNSHP=X" (sam/bam-files.go:289) */
  const uint64_t *seq_off;    /* n+1 byte offsets into seq4 */
  const uint8_t *seq4;        /* BAM 4-bit bases, high nibble first, "=ACMGRSVTWYHKDBN" (utils/nibbles, sam/sam-types.go:228) */
  const uint64_t *qual_off;   /* n+1 byte offsets into qual */
  const uint8_t *qual;        /* raw phred, no +33 (sam/sam-files.go:400-402) */
  const uint16_t *split;      /* optional (NULL = all 0): id of the `elprep split` file the record belongs to.  Records with different
                                 split ids are duplicate-marked as if by separate `elprep filter` runs (their fragment / mate / pair
                                 keys never match), so that one context can hold several contig-group splits of an `sfm` run
                                 (cmd/sfm.go:129-805 runs one filter process per split file) */
} elp_batch;

/* Header facts read by the filters: @SQ LN (alignmentAgreesWithHeader, filters/utils.go:130-139) and the @RG
 * dictionaries (lbTable, filters/mark-duplicates.go:413-423; readGroupCovariate, filters/bqsr.go:35-51). */
typedef struct elp_header {
  int32_t n_ref;
  const int32_t *ref_len;   /* @SQ LN per refid */
  int32_t n_rg;
  const uint16_t *rg_lib;   /* per rgid: dense id of the LB string, ELP_NIL16 if the RG has no LB / is not in the header */
  const uint16_t *rg_cov;   /* per rgid: dense id of the BQSR read-group covariate string (PU if present, else ID) */
  int32_t n_lib;
  int32_t n_cov;
} elp_header;

/* ---- context ---- */
int elp_create(int device_ordinal, elp_ctx **out);
void elp_destroy(elp_ctx *ctx);
const char *elp_last_error(const elp_ctx *ctx);
int elp_sync(elp_ctx *ctx);                 /* wait for the ctx stream */
void *elp_stream(elp_ctx *ctx);             /* the hipStream_t all kernels of this ctx are launched on */

/* ---- staging (replaces Sam.AddNodes' Slice(&alns) collection, sam/filter-pipeline.go:108-124) ---- */
int elp_set_header(elp_ctx *ctx, const elp_header *hdr);
int elp_reserve(elp_ctx *ctx, uint64_t n_records, uint64_t qname_bytes, uint64_t cigar_ops, uint64_t seq_bytes, uint64_t qual_bytes);
int elp_stage(elp_ctx *ctx, const elp_batch *batch); /* appends; host buffers may be reused when the call returns */
int elp_reset(elp_ctx *ctx);                         /* drops all staged records and results */
/* The same two calls with every array as an argument of its own - the forms a cgo binding uses with plain Go slices.  cgo's pointer
 * rules ("Passing pointers", cmd/cgo) let Go code pass a Go pointer to C only if the memory it points to contains no Go pointers: an
 * elp_header / elp_batch that lives in Go memory and points at Go slices breaks that rule (run-time panic "cgo argument has Go pointer
 * to Go pointer"), a call that passes &slice[0] of every slice does not (filters/pedantic.go:28-41 is the reference's own precedent
 * for a cgo call with scalar / single-pointer arguments).  A host that keeps its column buffers in C memory (elp_pinned_alloc: page-
 * locked, read in place by the DMA engine - the fast route over PCIe) may use either form.  has_sr and split may be NULL. */
int elp_set_header_columns(elp_ctx *ctx, int32_t n_ref, const int32_t *ref_len, int32_t n_rg, const uint16_t *rg_lib, const uint16_t *rg_cov,
                           int32_t n_lib, int32_t n_cov);
int elp_stage_columns(elp_ctx *ctx, uint64_t n, const int32_t *refid, const int32_t *pos, const int32_t *next_refid, const int32_t *pnext,
                      const int32_t *tlen, const uint16_t *flag, const uint8_t *mapq, const uint16_t *rgid, const uint8_t *has_sr,
                      const uint32_t *l_seq, const uint64_t *qname_off, const uint8_t *qname, const uint64_t *cigar_off, const uint32_t *cigar,
                      const uint64_t *seq_off, const uint8_t *seq4, const uint64_t *qual_off, const uint8_t *qual, const uint16_t *split);
uint64_t elp_num_records(const elp_ctx *ctx);
uint64_t elp_num_qual_bytes(const elp_ctx *ctx);     /* size of the staged QUAL column (elp_get_qual) */

/* ---- staging straight from BAM, and BAM out: the data formats either side of the path (sam/bam-files.go) ----
 * elp_set_read_group_ids: the @RG ID strings in the order of elp_header.rg_* (RG:Z tags are looked up in them).
 * elp_stage_bam: `bytes` = inflated BGZF payload holding whole alignment records (block_size, fixed fields, read name, CIGAR, bases,
 *   qualities, optional fields; SAMv1 4.2) as bamReader hands them to parseBamAlignment (:299-400).  The records cross PCIe as
 *   they are and are cut into the columns on the device; all of them get `split_id`.  Appends like elp_stage and may be mixed with
 *   it only in separate contexts.  rec_off (optional): byte offset of every record's block_size field, rec_off[n_records] = n_bytes -
 *   a BAM reader knows them; without them the call walks the block_size chain on the host (one dependent load per record).
 *   Fast path: `bytes` in page-locked memory (elp_pinned_alloc) - the DMA engine reads it in place;
 *   pageable memory goes through a pinned double buffer.  Returns when `bytes` may be reused.
 * elp_emit_sorted_bam: formatBamAlignment (:635-737) of the elp_num_sorted() records of the context's permutation - made by
 *   elp_sort_coordinate, elp_sort_queryname or elp_order_keep, whichever ran last - in that order, into
 *   `out` (host memory, `cap` bytes; NULL = just compute *n_bytes_out): FLAG and QUAL as the path left them, bin() recomputed
 *   (:443-468), optional fields re-encoded as formatBamTag does (:481-632).  BGZF deflate stays with the host. */
int elp_set_read_group_ids(elp_ctx *ctx, const char *const *ids);
/* cgo form (no array of pointers): the ids behind each other, id_off[g] .. id_off[g + 1] = the bytes of read group g (n_rg + 1 offsets) */
int elp_set_read_group_ids_flat(elp_ctx *ctx, const uint8_t *ids, const uint32_t *id_off);
void *elp_pinned_alloc(size_t bytes);
void elp_pinned_free(void *p);
int elp_stage_bam(elp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_off /* n_records + 1, may be NULL */,
                  uint64_t n_records, uint16_t split_id);
int elp_emit_sorted_bam(elp_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);
/* BGZF on the device (utils/bgzf/bgzf-files.go).
 * elp_stage_bgzf = the reader (:95-221) + elp_stage_bam: `bgzf` holds whole BGZF blocks of a BAM file (the file, or a part of it that
 * starts at a block and ends with a complete alignment record; an end-of-file block is skipped).  The compressed bytes are copied to the
 * device (in chunks, while the decoder works on the chunks in front), every block is inflated (RFC 1951: stored, fixed and dynamic Huffman
 * blocks; round 6, csrc/bgzf_inflate.hip: a wavefront turns the block's bit stream into literals in place and match tokens - 64 candidate symbols
 * per step -, a workgroup resolves the matches by pointer jumping in LDS), its CRC-32 is checked
 * ("invalid CRC-32 value for a data block in a BGZF file"), the starts of the alignment records are found on the device (every block
 * guesses its first record start, walks its records, and the guesses are proven by checking that every block's chain ends where the
 * next one's begins; wrong guesses are repaired in order), and the records are staged as elp_stage_bam stages them.  first_record = the
 * offset of the first alignment record in the inflated stream (behind magic, header text and reference dictionary, which the host
 * parses from the first block(s) itself); 0 for a part that starts with a record.
 * elp_emit_sorted_bgzf = elp_emit_sorted_bam + the writer (:324-383): the sorted records as BGZF blocks of <= 65280 payload bytes, each
 * COMPRESSED on the device (DEFLATE over a parallel LZ77 parse with the block's own Huffman codes - round 6; fixed codes where those are
 * not longer -, csrc/deflate_core.hpp; a block that would not shrink is stored), CRC-32 and ISIZE computed on the device.  Inflating the blocks gives elp_emit_sorted_bam's bytes (parity
 * of a BAM file is defined on the inflated stream: the reference's own bytes are whatever Go's compress/flate emits); a BAM file = the
 * host's header block(s) + these blocks + the 28-byte end-of-file block (:53-62).  A size query (out = NULL) returns an UPPER BOUND - the
 * size of the stored form, which is also the room `out` must offer; *n_bytes_out of the real call is the actual size. */
int elp_stage_bgzf(elp_ctx *ctx, const uint8_t *bgzf, uint64_t n_bytes, uint64_t first_record, uint16_t split_id);
int elp_emit_sorted_bgzf(elp_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);
/* ---- SAM text in (sam/sam-files.go:186-410, sam/string-scanner.go, ScanCigarString sam/sam-types.go:680-740; csrc/samin.hip) ----
 * The reference reads SAM text whenever it is fed from an aligner's pipe (sam.Open picks the reader by content, sam/aln-files.go:144-174).
 * elp_stage_sam replaces the host's parseSamAlignment per line + elp_stage: `text` = whole alignment lines of a SAM file - the host reads
 * and strips the header lines, as it writes them for the emitters.  The device turns every line into the BAM record
 * formatBamAlignment(parseSamAlignment(line)) writes behind AddREFID (filters/simple-filters.go:208-231) and stages it as elp_stage_bam
 * stages records: columns, sr state, RG look-up and the staged bytes the emitters, the tag filter, elp_filter_exact_strict,
 * elp_copy_records and elp_exchange_records read.  A staging call with elp_stage_bam's rules: it appends and returns when `text` may be
 * reused; page-locked `text` is read in place, pageable text goes through the pinned double buffer; it may be mixed with elp_stage_bam /
 * elp_stage_bgzf on one context, not with elp_stage; every record gets `split_id`.  Needs a header, the read-group ids
 * (elp_set_read_group_ids*, unless elp_set_replace_read_group is in force) and the reference names (elp_set_reference_names_flat:
 * ELP_ERR_ARG without them; RNAME and RNEXT are looked up in a hash table over them in HBM, made by the first call behind the names and
 * dropped with them); refused behind elp_replace_reference_dictionary, as the other staging calls are.
 *   A line is the bytes up to '\n' with one trailing '\r' dropped (bufio.ScanLines); a last line without '\n' counts; an empty line and
 * a line of more than 1 MiB (maxTokenSize, sam/sam-files.go:614) are ELP_ERR_DATA.  Eleven mandatory fields (ten tabs, else
 * ELP_ERR_DATA): FLAG = ParseUint(.., 16), MAPQ = ParseUint(.., 8), POS / PNEXT / TLEN = ParseInt(.., 32) (a sign is read by ParseInt
 * only); BAM pos = POS - 1 with int32 wrap-around.  RNAME: "*" and "=" give -1 (AddREFID knows no contig "="), else the name's refid;
 * RNEXT: "*" -1, "=" RNAME's refid.  CIGAR: "*" or empty = no operation, else <decimal><op> with op in "MIDNSHP=X" in either case
 * (cigarOperationsTable), adjacent operations of one kind merged with their lengths added ("5M5M" is 10M).  SEQ: a nibble per byte from
 * "=ACMGRSVTWYHKDBN", every other byte 15 (lower case, and "*" = ONE base N); QUAL: every byte - 33 modulo 256 ("*" = one quality of 9).
 * Optional fields KK:T:value: A one byte; i = ParseInt(.., 64) stored in the smallest of c C s S i I that holds it (formatBamTag,
 * sam/bam-files.go:492-523); Z the bytes + NUL; B a subtype, ',' and at least one entry, entries ParseInt at 8 / 32 bits (c, i) or
 * ParseUint at 8 / 16 / 32 (C, S, I) - and B:s through ParseUint(.., 16) cast to int16 as the reference has it (:263-272): "-1" is
 * refused, "40000" stored as -25536; f and B:f = float32(ParseFloat(s, 32)): [+-]digits[.digits][(e|E)[+-]digits] with a digit in the
 * mantissa, [+-]inf / infinity, unsigned nan (0x7FC00000), the float32 NEAREST the decimal with ties to even, read directly and not via a
 * double; beyond the largest float32 ELP_ERR_DATA, underflow +-0.  A tab behind the last field ends the line, as in the reference.
 * strconv is restated from its documentation (csrc/samparse.hpp): no Go toolchain was at hand to run against.
 *   ELP_ERR_DATA: what the reference panics on - the above, an empty CIGAR length, an unknown operation, a length beyond int32, an
 * unknown field type, a field that is not KK:T:, "B:c" without comma or entry, a number that does not parse.  ELP_ERR_UNSUPPORTED: what
 * the reference reads and this call does not - an RNAME / RNEXT that is neither "*" / "=" nor in the dictionary (the reference's BAM
 * writer makes -1 of it, its SAM writer keeps the string, which the emitters here cannot print); a merged CIGAR length above 2^28 - 1,
 * more than 65535 operations; len(QUAL) != len(SEQ) (the reference writes a record whose l_seq and QUAL disagree); QNAME above 254 bytes
 * or with a NUL; two fields of one key in a line (SmallMap.Set would overwrite the first in place); an i value outside
 * [-2^31, 2^32 - 1]; a NUL in a Z value; H fields (as the emitters); hexadecimal floats, underscores in floats, float tokens above 64
 * bytes; more than 245 optional fields in a line; a tab as a key byte or as the value of an A field (the reference's scanner steps over
 * it; here the line is ELP_ERR_DATA).
 *   Errors: the first bad line of a piece decides; elp_last_error names its 0-based line number within the call and the reason.  Errors
 * are found in the size pass, before anything of the piece is committed: a text of up to 256 MiB is one piece and is staged whole or not
 * at all; of a longer text the pieces in front of the refused one stay staged, as elp_stage_bam leaves them (elp_num_records tells).
 * elp_set_tuning("sam_pass") caps the lines per write pass (tests).
 * Reads: the header, read-group ids, names.  Writes: what elp_stage_bam writes; invalidates what it invalidates. */
int elp_stage_sam(elp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, uint16_t split_id);
/* The merge of `elprep merge` / `sfm` phase 3 with payloads (MergeSortedFilesSplitPerChromosome, sam/split-merge.go:410-576): the sorted
 * outputs of a context that holds group splits and of the context that holds the spread split as ONE stream of BAM records in the merge's
 * order (elp_merge_spread's slots), gathered in HBM.  Both contexts staged with elp_stage_bam, on one device, each coordinate-sorted
 * (elp_sort_coordinate) or holding coordinate-sorted input in input order (elp_order_keep with by_split = 0; elp_merge_spread states the
 * rule and its check).
 * elp_emit_merged_bgzf: the same stream as BGZF members, as elp_emit_sorted_bgzf writes the sorted one (`sfm`'s final output): members of
 *   65280 payload bytes except the last, wherever the device passes fall (the bytes behind a pass's last full member are carried into the
 *   next pass); inflating the members gives elp_emit_merged_bam's bytes; a size query (out = NULL) returns the stored form's size, an
 *   upper bound and the room `out` must offer.  Same checks and errors as elp_emit_merged_bam. */
int elp_emit_merged_bam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);
int elp_emit_merged_bgzf(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);
/* The merge of UNSORTED splits: MergeUnsortedFilesSplitPerChromosome (sam/split-merge.go:581-619), which `elprep merge` takes for every
 * header that says neither SO:coordinate nor SO:queryname (cmd/merge.go:178-188).  The stream is (1) the output records of `groups` with
 * split id 0 - the unmapped file -, (2) all output records of `spread`, (3) the output records of `groups` with split ids 1, 2, ... in
 * id order - the group files; every part in staging order; records that are not output (sr-tagged copies, rejected records) appear
 * nowhere.  `groups` must hold a keep permutation made with by_split = 1 and `spread` one made with by_split = 0 (elp_order_keep), else
 * ELP_ERR_ARG; `spread` may be an empty context.  Otherwise the checks of elp_emit_merged_bam: one device, both staged with elp_stage_bam,
 * equal tag filters, equal replacing read groups, equal dictionary-replacement state (ELP_ERR_ARG), fewer than 2^31 output records
 * (ELP_ERR_UNSUPPORTED).  Ordering the stream across ranks is the host's: a rank's call covers the splits its context holds.
 * Reads: both permutations, the split-id column of `groups` (the end of the unmapped file among its output: one word made on the
 * device), and what elp_emit_sorted_bam reads.  Writes: `out` only.  elp_emit_concat_bgzf is the BGZF form, as elp_emit_merged_bgzf. */
int elp_emit_concat_bam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);
int elp_emit_concat_bgzf(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);

/* ---- the BAM index of a stream the device has written (SAM specification 5.2; csrc/bai.hip, csrc/bai_plan.hpp) ----
 * The reference writes no index: this is an extension.  elp_index_sorted_bgzf makes the .bai of the members elp_emit_sorted_bgzf has just
 * returned, elp_index_merged_bgzf that of elp_emit_merged_bgzf's, from the context's columns and the members' sizes - nothing is inflated,
 * no record comes back to the host.  `bgzf`, `n_bytes`: exactly what the emit call returned for the context(s) in their PRESENT state
 * (permutation, tag filter, replacing read group, CleanSam); base_coffset: the file offset at which the host writes these members, behind
 * its header block(s).  bai_out = NULL: a size query, exact.  The call invalidates nothing and writes only scratch and bai_out; a refused
 * call writes nothing.
 *   The host part (bai_plan.hpp) walks the members of the untrusted bytes - the 18-byte header 1f 8b 08 04 .. XLEN 6, 'B' 'C' 2 0,
 * BSIZE at byte 16, ISIZE in the last four bytes; every member but the last holds 65280 bytes, the last 1 .. 65280; no members at all is
 * valid - and gives coff[0 .. n_members], coff[n_members] = n_bytes.  ELP_ERR_DATA names the byte of a truncated member, a bad magic or
 * subfield, a BSIZE that runs past the end, a wrong ISIZE.  The ISIZE must add up to the stream length the device's size pass finds for
 * the context: else ELP_ERR_ARG "these bytes are not this context's stream".
 *   The index, canonical.  Stream position p has the virtual offset voff(p) = (base_coffset + coff[p / 65280]) << 16 | p % 65280.  Output
 * record k (the emitter's order and sizes): S = voff of its first byte, E = voff of the byte behind its last.  refid < 0: counted in
 * n_no_coor and nothing else.  Otherwise beg = max(POS - 1, 0), end = beg + span, span = the reference-consuming operations of the CIGAR
 * column as emitted, 1 if that is 0 or FLAG & 0x4; bin = reg2bin(beg, end - 1); windows beg >> 14 .. (end - 1) >> 14.
 *   Bytes, little-endian: "BAI\1", int32 n_ref (the dictionary in force); per contig int32 n_bin, the bins, int32 n_intv, uint64
 * ioffset[n_intv]; uint64 n_no_coor (always).  A contig without records: n_bin 0, n_intv 0.  With records: n_bin = distinct bins + 1, in
 * ascending bin number, each uint32 bin, int32 n_chunk, chunks uint64 beg, end: of a bin's records in output order one extends the
 * current chunk iff S >> 16 == chunk.end >> 16 (it starts in the member the chunk ends in), else opens one; chunk.end = E of its last
 * record.  Last the pseudo-bin 37450 with two chunks: (S of the contig's first record, E of its last), (n_mapped, n_unmapped by FLAG &
 * 0x4).  n_intv = the largest window a record of the contig touches + 1; ioffset[w] = the smallest S of the records that touch w, for a
 * window nobody touches the value of the next touched one to its right.
 *   Checks: the context holds a coordinate permutation (elp_sort_coordinate), or a plain keep permutation (elp_order_keep, by_split = 0)
 * whose (refid, POS) order passes elp_merge_spread's check - else ELP_ERR_DATA "records are not in coordinate order".  A queryname or
 * by-split permutation, none at all, records not staged with elp_stage_bam / _bgzf / _sam, cap below the size, base_coffset + n_bytes
 * beyond 2^48: ELP_ERR_ARG.  A record that ends beyond position 2^29 (a bin cannot hold it): ELP_ERR_UNSUPPORTED.  The merged form runs
 * elp_emit_merged_bam's checks.  Joining the indices of several ranks' parts of one file is host arithmetic on offsets, not done here. */
int elp_index_sorted_bgzf(elp_ctx *ctx, const uint8_t *bgzf, uint64_t n_bytes, uint64_t base_coffset, uint8_t *bai_out, uint64_t cap, uint64_t *n_bytes_out);
int elp_index_merged_bgzf(elp_ctx *groups, elp_ctx *spread, const uint8_t *bgzf, uint64_t n_bytes, uint64_t base_coffset, uint8_t *bai_out, uint64_t cap,
                          uint64_t *n_bytes_out);

/* ---- SAM text out (sam/sam-files.go:485-598; csrc/sam.hip) ----
 * The writer of the reference picks the format by the file's extension (sam/aln-files.go:134-135): these are the ".sam" forms of the
 * emitters above.  Each writes FormatAlignment(parseBamAlignment(record)) (:563-598, sam/bam-files.go:317-400) of every record its BAM
 * counterpart writes, in the same order, from the same permutation: eleven fields separated by tabs, every optional field behind a tab,
 * '\n'.  FLAG and MAPQ unsigned, POS / PNEXT (1-based) and TLEN signed decimal; RNAME = the name of refid, "*" below 0; RNEXT "*" for
 * next_refid < 0, "=" for next_refid == refid, else the name; CIGAR from the CIGAR column (behind elp_clean_sam), "*" for no operation;
 * SEQ one character per base of "=ACMGRSVTWYHKDBN" and EMPTY for l_seq 0 (the reference's loop writes nothing, not "*"); QUAL every byte
 * of the QUAL column as it is now + 33 modulo 256 (BAM's 0xFF "missing" bytes leave as spaces, as the reference writes them).  Optional
 * fields (formatSamTag :485-546) behind the tag filter and the read-group replacement, in the order the BAM emitters keep: A as :A:, c C
 * s S i I as :i: + decimal (the parser makes int64 of all), Z as :Z:, B as :B:<subtype> and ",<value>" per element, f and B:f values as
 * strconv.AppendFloat(float64(v), 'g', -1, 32) - the shortest decimal that reads back as the float32, exponent form "d.ddde+XX" for a
 * decimal exponent below -4 or from 6 up, NaN, +Inf, -Inf (csrc/samtext.hpp) -, a replaced or added read group as "\tRG:Z:<id>".
 * H fields: ELP_ERR_UNSUPPORTED, malformed fields: ELP_ERR_DATA, as in the BAM emitters.
 *   No header text goes out: the host writes @HD, @SQ, @RG and @PG and then these bytes.  out = NULL is a size query and returns the
 * EXACT size (text has no framing).  Checks, errors and concurrency rules are the BAM counterparts' (a permutation, records staged with
 * elp_stage_bam, the two-context rules of elp_emit_merged_bam / elp_emit_concat_bam), and: the reference names must be set
 * (ELP_ERR_ARG), in a stream of two contexts equal names in both (ELP_ERR_ARG - the rule of the tag filters); a staged next_refid that
 * the dictionary does not hold is ELP_ERR_DATA.  elp_set_tuning("emit_pass") caps these passes too.
 * Reads: what the BAM counterpart reads, and the names.  Writes: `out` only; the calls invalidate nothing.
 * elp_set_reference_names_flat: the @SQ SN strings of the context's CURRENT dictionary, behind each other: name_off[r] .. name_off[r + 1]
 *   = name of refid r (n_ref + 1 offsets).  Call after elp_set_header, for the dictionary the context holds now.  The names belong to
 *   that dictionary and are dropped wherever the reference table is replaced: elp_set_header, elp_replace_reference_dictionary (the host
 *   then sets the NEW names), an elp_reset that undoes a replacement; a plain elp_reset keeps them (the next file of the same header).
 *   ELP_ERR_ARG: no header, NULL arrays with n_ref > 0, offsets that decrease, an empty name, a name "*" or "=", two equal names -
 *   names are distinct, so the device decides "=" by comparing refids where the reference compares strings (bam-files.go:344-346).
 *   Writes: the names and an offsets table in HBM. */
int elp_set_reference_names_flat(elp_ctx *ctx, const uint8_t *names, const uint32_t *name_off);
int elp_emit_sorted_sam(elp_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);
int elp_emit_merged_sam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);
int elp_emit_concat_sam(elp_ctx *groups, elp_ctx *spread, uint8_t *out, uint64_t cap, uint64_t *n_bytes_out);

/* ---- the options that touch a record's optional fields (filters/simple-filters.go; cmd/filter.go:696-902) ----
 * The settings of elp_set_tag_filter and elp_set_replace_read_group belong to a run: elp_reset and elp_set_header clear both.
 *
 * elp_set_tag_filter: `--remove-optional-fields a,b` / `all` (RemoveOptionalFields :235-257, KeepOptionalFields(nil) :263-269,
 *   cmd/filter.go:878-889) and `--keep-optional-fields a,b` / `none` (KeepOptionalFields :261-288, cmd/filter.go:891-902) for the
 *   emitters.  remove_keys = n_remove two-byte keys behind each other; n_remove = -1: `all`; 0: no such filter.  keep_keys likewise;
 *   n_keep = -1: no keep filter; 0: `none` (also what a keep list without any two-byte entry amounts to).  A BAM tag key is two bytes,
 *   so a list entry of another length matches no field: the host drops it from the list.  More than 4096 keys in a list:
 *   ELP_ERR_UNSUPPORTED.  filters2 applies remove, then keep, each by SmallMap.DeleteIf, which deletes EVERY entry that matches
 *   (utils/small-map.go:89-99): a field goes out iff its key is not in the remove list (and remove is not `all`) and, with a keep
 *   filter, its key is in the keep list; fields of one key are all treated alike, the survivors keep their order and are re-encoded as
 *   before.  Call any time before the emit call (n_remove = 0, n_keep = -1 takes the filter away).  It acts on elp_emit_sorted_bam,
 *   elp_emit_sorted_bgzf, elp_emit_merged_bam / _bgzf and elp_emit_concat_bam / _bgzf - sizes, offsets, block_size, the size query, BGZF framing; the merged stream takes the
 *   filter of `groups` and the call returns ELP_ERR_ARG if `spread`'s differs.  Nothing else sees it (filters2 runs behind ApplyBQSR,
 *   cmd/filter.go:66-100): the staged rgid column and sr states, duplicate marking, BQSR, elp_copy_records and elp_exchange_records work
 *   on the unfiltered records; removing RG from the output changes no table.  Malformed fields and H fields are reported as without a
 *   filter, also in a field the filter drops (the reference parses before it filters).  Reads: the staged BAM bytes.  Writes: a table of
 *   65536 bits (one per key) in HBM, which the emitters' size and gather kernels look up per field in the walk they make anyway.
 * elp_set_replace_read_group: `--replace-read-group` (AddOrReplaceReadGroup :156-162).  Call after elp_set_header with a header of ONE
 *   read group (the new one: header.RG = []{readGroup}) and before staging (ELP_ERR_ARG with records staged or n_rg != 1); id_len <= 255,
 *   no NUL inside.  From then on elp_stage_bam / elp_stage_bgzf do not look RG fields up (elp_set_read_group_ids is not needed): every
 *   record, with or without an RG field, gets rgid 0 (aln.SetRG(id) runs on every alignment in front of AddREFID and MarkDuplicates:
 *   library and BQSR covariate are the new group's).  The emitters follow SmallMap.Set (utils/small-map.go:59-67): the first field
 *   with key RG, whatever its type, goes out as RG:Z:<id> in its place, later RG fields stay as they are, a record without one gets
 *   RG:Z:<id> behind its last field; the tag filter then acts on the result.  An output record can be 4 + id_len bytes longer than the
 *   staged one (the size query accounts for it).  The setting travels with nothing: elp_copy_records / elp_exchange_records between
 *   contexts whose settings differ return ELP_ERR_ARG, as does elp_emit_merged_bam.  Writes: the rgid column (at staging).
 * elp_filter_exact_strict: `--filter-non-exact-mapping-reads-strict` (RemoveNonExactMappingReadsStrict :115-134), one of the filters1
 *   predicates - call where elp_filter_records is called.  A record is kept iff its FIRST field of key X0 exists and is 1, then likewise
 *   X1, XM, XO, XG exist and are 0, in this order, stopping at the first test that fails; the value is the integer parseBamAlignment
 *   reads (types c C s S i I, sam/bam-files.go:138-173).  A tested field of another type makes the reference panic (x.(int64)): the call
 *   fails with ELP_ERR_DATA and changes nothing - but only if the tests in front of it passed for that record.  Rejected records get
 *   the state elp_filter_records gives (same effect on everything that follows; the counts of the calls add up).  Needs records staged
 *   with elp_stage_bam / elp_stage_bgzf (ELP_ERR_ARG otherwise: column-staged records have no optional fields).  Reads: the staged BAM
 *   bytes, the record-state column.  Writes: the record-state column.  n_rejected_out may be NULL.
 * elp_clear_duplicate_flag: `--clear-duplicate-flag` (ClearDuplicateFlag :350-355, cmd/filter.go:729-731): FLAG &^= 0x400 on every
 *   staged record whatever its state, behind the filters1 predicates and in front of elp_mark_duplicates.  Existing duplicate marks and
 *   any permutation become invalid (the comparator's modFlag tie-break reads the bit); sort keys and scores stay.  Reads and writes: the
 *   FLAG column. */
int elp_set_tag_filter(elp_ctx *ctx, const uint8_t *remove_keys, int n_remove, const uint8_t *keep_keys, int n_keep);
int elp_set_replace_read_group(elp_ctx *ctx, const uint8_t *id, int id_len);
int elp_filter_exact_strict(elp_ctx *ctx, uint64_t *n_rejected_out /* may be NULL */);
int elp_clear_duplicate_flag(elp_ctx *ctx);
/* elp_replace_reference_dictionary: `--replace-reference-sequences` (ReplaceReferenceSequenceDictionary, filters/simple-filters.go:32-60,
 *   appended to filters1 at cmd/filter.go:752-755, cmd/sfm.go:423-425) together with the renumbering that AddREFID makes behind it under
 *   the new header.SQ (:208-231, cmd/filter.go:762-766).  Staged records carry the OLD file's refids, in their bytes and in the REFID /
 *   RNEXT columns; the sort keys, the duplicate-marking keys, the BQSR reference look-ups, the contig order of the output and the refID /
 *   next_refID the BAM writer emits (sam/bam-files.go:642-647, 674-681) all follow the NEW dictionary.
 *   new_of_old[r] (r < the context's n_ref) = index in the new dictionary of old contig r's name, -1 if the new dictionary does not hold
 *   it (elp_host_dictionary_map, elprep_host.h, makes it from the names); ref_len_new[n_ref_new] = the new @SQ LN values.
 *   Records: one stays iff its refid < 0 (RNAME `*`: dictTable["*"], :53) or new_of_old[refid] >= 0 (:58); every other record gets the
 *   state elp_filter_records gives (same effect on everything that follows).  The counts of the calls add up as for
 *   elp_filter_exact_strict: a record that was live is counted in *n_rejected_out (and leaves elp_num_sorted()); an sr-tagged copy that
 *   is rejected was counted when it was staged; a record an earlier call rejected is not looked at again.
 *   Columns, for EVERY record whatever its state: refid = refid < 0 ? -1 : new_of_old[refid], next_refid likewise (a kept record whose
 *   mate's contig left the dictionary gets next_refid -1, as the writer emits for a name it does not hold; `=` needs no case of its own,
 *   the column holds it resolved; a value the old dictionary does not hold - possible in RNEXT of staged BAM bytes - names nothing: -1).
 *   A write that would change nothing is not made: the identity map with n_ref_new == n_ref leaves every column byte as it was.
 *   Header state: the context's reference table becomes the new one - elp_bqsr_set_reference / elp_bqsr_set_known_sites made BEFORE the
 *   call are dropped (their refids were the old ones'): the host sets them afterwards under the new refids.  Everything called afterwards
 *   sees the new dictionary.  The emitters take refID / next_refID from the columns, so the output records carry the new ones.
 *   Call order: where the reference's filter stands - behind elp_filter_records, elp_filter_exact_strict and elp_clean_sam, in front of
 *   elp_mark_duplicates (elp_clear_duplicate_flag, :729-731, may stand on either side: the two touch different columns).  CleanSam
 *   precedes it in filters1 (cmd/filter.go:747-749 against :752-755) and so
 *   clips against the OLD dictionary's LN: call elp_clean_sam first.  A second call on the same records is allowed; it maps from the
 *   dictionary as it then is.
 *   Errors: ELP_ERR_ARG without a header, for n_ref_new < 0, a NULL array that is needed, or a new_of_old[r] outside [-1, n_ref_new) -
 *   all checked on the host before anything is launched or changed (a call refused so changes nothing; after a HIP failure inside the
 *   call the context is good for elp_reset / elp_set_header only).
 *   Afterwards the staged bytes and the header no longer agree: elp_stage, elp_stage_columns, elp_stage_bam and elp_stage_bgzf return
 *   ELP_ERR_ARG until elp_reset or elp_set_header.  elp_reset returns to the dictionary elp_set_header gave (references and known sites
 *   set under the new refids are dropped with it, and elp_set_header behind a replacement drops them likewise), so a host that resets and stages the next file of the same header goes on as before.
 *   elp_copy_records, elp_exchange_records and elp_emit_merged_bam return ELP_ERR_ARG between two contexts of which one has replaced its
 *   dictionary and the other has not (the rule of elp_set_replace_read_group); two that both did, with equal results, pass.
 *   The sort keys (with key passes made ahead, elp_sort_ahead), scores, marks, any permutation and a snapshot (elp_rollback cannot
 *   restore refids) become invalid (csrc/derived.hpp: dictionary_replaced).  The @SQ lines and @HD SO of the output stay with the host.
 *   Reads: the REFID, RNEXT and record-state columns (9 bytes per record), the map (from LDS up to 256 old contigs, else from HBM).
 *   Writes: the same three columns where a value changes; the context's reference table.  n_rejected_out may be NULL. */
int elp_replace_reference_dictionary(elp_ctx *ctx, const int32_t *new_of_old /* [old n_ref] */, int32_t n_ref_new,
                                     const int32_t *ref_len_new /* [n_ref_new] */, uint64_t *n_rejected_out /* may be NULL */);

/* ---- fused per-record predicates: filters/simple-filters.go ----
 * The filters that stand in front of MarkDuplicates in filters1 (cmd/filter.go:696-803), evaluated in one pass over the staged
 * records: a rejected record takes part in nothing that follows (duplicate marking, sort output, metrics, BQSR tables) - it is
 * behind the elp_num_sorted() records of the permutation.  Call before the other operators; may be called again (predicates add up).
 *   remove_unmapped          RemoveUnmappedReads          :73-75    FLAG & 0x4
 *   remove_unmapped_strict   RemoveUnmappedReadsStrict    :79-83    ... or POS == 0 or RNAME == "*"
 *   min_mapq                 RemoveMappingQualityLessThan :332-347  keep MAPQ >= min_mapq (0 = off, > 255 rejects everything)
 *   remove_non_exact         RemoveNonExactMappingReads   :90-99    CIGAR may hold M and S only
 *   remove_duplicates        RemoveDuplicateReads         :136-138  FLAG & 0x400 as the column is now
 *   use_regions              RemoveNonOverlappingReads    :310-328  regions[refid] = [n_regions[refid]][2] {Start, End} as
 *                            intervals.FromBed makes them, sorted by Start and flattened; intervals.Overlap's comparisons */
typedef struct elp_predicates {
  int remove_unmapped, remove_unmapped_strict, min_mapq, remove_non_exact, remove_duplicates, use_regions;
  const int32_t *const *regions;
  const int64_t *n_regions;
} elp_predicates;
int elp_filter_records(elp_ctx *ctx, const elp_predicates *p, uint64_t *n_rejected_out /* may be NULL */);
/* cgo form (no pointers to pointers): the target regions of all contigs behind each other, region_off[r] .. region_off[r + 1] = the
 * {Start, End} rows of refid r (n_ref + 1 offsets, counted in intervals); regions NULL = no target-region test */
int elp_filter_records_flat(elp_ctx *ctx, int remove_unmapped, int remove_unmapped_strict, int min_mapq, int remove_non_exact, int remove_duplicates,
                            const int32_t *regions, const int64_t *region_off, uint64_t *n_rejected_out /* may be NULL */);

/* ---- `elprep split` / `merge` without touching payloads on the CPU: sam/split-merge.go ----
 * elp_split_classify: SplitFilePerChromosome's routing rule (:280-293) for every staged record: split_out[i] = 0 for RNAME "*",
 *   else group_of_ref[refid] (1..n_groups, computeContigGroups :178-213 on the host); spread_out[i] = 1 if the read also goes to the
 *   spread file (mate in another group); counts_out[n_groups + 2] = records per split (unmapped, groups, spread).  The split ids are
 *   also written to the context's split-id column (elp_batch.split), so that elp_copy_records / elp_exchange_records with new_split = -1
 *   deliver every record with the id of its split file.
 * elp_merge_spread: MergeSortedFilesSplitPerChromosome (:410-576) as ranks: slot_of_spread_out[j] = output slot of the j-th record of
 *   `spread`'s output among `groups`' output (behind every group read of its (refid, POS) and in front of the first greater one; group
 *   reads fill the remaining slots in order).  Each context holds a coordinate permutation (elp_sort_coordinate) or a plain keep
 *   permutation (elp_order_keep with by_split = 0); one of each is allowed, both are (refid, POS)-sorted streams.  A keep permutation is
 *   the sorted-input case: `sfm` on a header with SO:coordinate filters every split in input order (effectiveSortingOrder,
 *   sam/filter-pipeline.go:208-225) and interleaves the spread reads by (refid, POS).  By choosing this call the host vouches for
 *   SO:coordinate, as cmd/merge.go:157-174 chooses by header.HDSO(); a context that received its split files in file order holds them in
 *   the merge's order (the group files are read contig by contig in refid order, the groups hold consecutive contigs, `*` records are a
 *   sorted file's tail and are appended last, :557-576).  The merge's binary search needs (refid, POS) non-decreasing with refid -1 last:
 *   every keep-ordered side is checked (one pass over its keys, one word read back) and a violation returns ELP_ERR_DATA "records are
 *   not in coordinate order" with nothing emitted - a stated limit: the reference would write some order of its own.  A queryname
 *   permutation returns ELP_ERR_UNSUPPORTED, a keep permutation made with by_split != 0 ELP_ERR_ARG, no permutation ELP_ERR_ARG. */
int elp_split_classify(elp_ctx *ctx, const int32_t *group_of_ref, int32_t n_groups, uint16_t *split_out, uint8_t *spread_out, uint64_t *counts_out);
/* elp_copy_records: the write side of the same routing (:280-293 writes the record into the file of its split, and a copy tagged sr:i:1
 *   into the group file if the original goes to the spread file): appends the records idx[0 .. n) of `src` (staging indices, any order)
 *   to `dst` - two contexts of this process on one GPU or on two (device-to-device / peer copies of gathered column slices; nothing
 *   passes through the host).  new_split >= 0: the split id the copies get (else they keep theirs); tag_sr = 1: live records arrive as
 *   sr-tagged copies; tag_sr = 2: only the records whose index has bit 31 set do (the index is its low 31 bits: one call delivers a
 *   split file's records in input order, tagged copies among the others, as :280-293 writes them).  FLAG and QUAL travel as they are now; the inflated BAM records travel too if both contexts hold them
 *   (elp_stage_bam).  Large sets move in pieces inside the call; on an error the pieces already appended stay (elp_num_records tells). */
int elp_copy_records(elp_ctx *dst, elp_ctx *src, const uint32_t *idx, uint64_t n, int new_split, int tag_sr);
int elp_merge_spread(elp_ctx *groups, elp_ctx *spread, uint64_t *slot_of_spread_out);
/* elp_emit_split_bam / _bgzf / _sam: the FILES of `elprep split`, written on the device - SplitFilePerChromosome (:225-311) and
 *   SplitSingleEndFilePerChromosome (:664-724) with payloads.  One call writes all split files of the context's staged records behind each
 *   other into `out`: file_off_out[f] .. file_off_out[f + 1] are the bytes of file f (n_files + 1 offsets), *n_bytes_out their total.
 *   single_end == 0: n_files = n_groups + 2 - file 0 the unmapped file, files 1 .. n_groups the group files, file n_groups + 1 the spread
 *   file.  single_end != 0: n_files = n_groups + 1, no spread file, nothing tagged.  group_of_ref as elp_split_classify takes it (n_ref
 *   entries, each 0 .. n_groups); the routing is that call's rule (:280-293): a record goes to the file of its contig group, RNAME "*" to
 *   file 0; it is spread iff next_refid != refid, refid >= 0 and the mate's group differs (so a mapped record with RNEXT "*" is spread).
 *   Every file holds its records in staging order: a group file the untagged records and the tagged copies of the spread records among
 *   each other, each at its record's place; the spread file the untagged originals.  Records rejected by elp_filter_records and its kin
 *   (state 2) appear nowhere; records staged WITH an sr field (state 1: a split file that is split again) are routed and written as any
 *   other and keep their sr fields.
 *   A record's bytes are what the emitter of the same format writes for it (elp_emit_sorted_bam / _sam: CIGAR from the CIGAR column, FLAG
 *   and QUAL as they are now, integers re-encoded in their smallest type).  A tagged copy additionally gets aln.TAGS.Set(sr, int64(1))
 *   (:290; SmallMap.Set, utils/small-map.go:59-67): the FIRST field with key sr, whatever its type, goes out in its place as s r C 0x01
 *   (SAM: sr:i:1), later sr fields stay as they are, a record without one gets the field behind its last field (4 bytes, SAM: "\tsr:i:1").
 *   _bgzf: each file is framed on its own, as elp_emit_sorted_bgzf frames its stream - members of 65280 payload bytes except a file's last,
 *   nothing carried across a file boundary, an empty file is zero bytes; inflating file f's members gives _bam's bytes of file f.
 *   Header text or blocks - with the @sr co: line and the per-file @cs lines elprep split adds -, the BGZF end-of-file block and the file
 *   names are the host's.  out == NULL is the size query: _bam and _sam return the exact total and offsets, _bgzf the stored form's upper
 *   bound and bound offsets; the real call packs the files at their actual sizes.  elp_set_tuning "emit_pass" caps these passes too.
 *   The call reads the staged records only: it needs no elp_split_classify, reads and writes neither the split-id column nor a
 *   permutation, and invalidates nothing.
 *   Errors: ELP_ERR_ARG for NULL arguments, n_groups < 1 or > 65533, a group_of_ref entry outside 0 .. n_groups, records that were not
 *   staged with elp_stage_bam / _bgzf / _sam (no bytes to write), a tag filter or a replacing read group (`elprep split` has no such
 *   options: refused, not composed), _sam without reference names, an output buffer too small (*n_bytes_out = 0);
 *   ELP_ERR_UNSUPPORTED for more than 2^31-16 staged records (bit 31 of a list entry marks the tagged copy) and for H fields,
 *   ELP_ERR_DATA for malformed fields, as in the other emitters.
 *   Limits: the call is for READER contexts.  A context that received tagged copies through elp_copy_records / elp_exchange_records holds
 *   state 1 without the field in its bytes, and such records are written without it.  MergeInputs (several input files,
 *   sam/merge-inputs.go) stays the host's. */
int elp_emit_split_bam(elp_ctx *ctx, const int32_t *group_of_ref, int32_t n_groups, int single_end, uint8_t *out, uint64_t cap,
                       uint64_t *file_off_out /* n_files + 1 */, uint64_t *n_bytes_out);
int elp_emit_split_bgzf(elp_ctx *ctx, const int32_t *group_of_ref, int32_t n_groups, int single_end, uint8_t *out, uint64_t cap,
                        uint64_t *file_off_out /* n_files + 1 */, uint64_t *n_bytes_out);
int elp_emit_split_sam(elp_ctx *ctx, const int32_t *group_of_ref, int32_t n_groups, int single_end, uint8_t *out, uint64_t cap,
                       uint64_t *file_off_out /* n_files + 1 */, uint64_t *n_bytes_out);

/* ---- coordinate sort: By(CoordinateLess).ParallelStableSort (sam/sam-types.go:425-473, 639-641) ----
 * Builds the permutation on device: perm[k] = staging index of the record at sorted position k; records equal
 * under all nine keys of CoordinateLess keep staging order.  Payload permutation is the caller's (host) work.
 * The comparator's modFlag(FLAG) tie-break reads the FLAG column as it is at the time of the call.  In `elprep filter` the sort is
 * the Finalize step of the phase-1 pipeline (sam/filter-pipeline.go:116): it runs BEHIND the filters, so with --mark-duplicates it
 * sees the duplicate bits.  A drop-in host therefore calls elp_mark_duplicates first, then elp_sort_coordinate.
 * Concurrency (round 6): the sort runs on a SIDE LANE of the context - a stream, scratch pool and error words of its own; it reads the
 * key column and the comparator's columns and writes the permutation, nothing the BQSR calls touch.  Once elp_mark_duplicates has
 * returned, a host may therefore call elp_sort_coordinate from a thread of its own (a goroutine locked to its OS thread) WHILE another
 * thread calls elp_dup_metrics (side lane of its own, below) and a third drives elp_bqsr_gather(_device) -> finalize -> elp_bqsr_apply
 * on the same context: the three chains need nothing of each other (the reference runs them one after the other,
 * cmd/filter.go:162-196).  The call returns when the permutation is complete; calls that read it afterwards (elp_get_permutation,
 * elp_emit_*) are ordered behind it.  Calls that CHANGE staged records (staging, reset, rollback, filters, exchange) must not overlap
 * with any other call on the context.  What the sort's thread touches of the context: it READS the key column with its validity item
 * "keys" (csrc/derived.hpp - elp_mark_duplicates leaves it valid and no BQSR call clears it: elp_bqsr_apply spoils the scores and the
 * quality hint only, so the sort never enters the adapt stage nor the context's own stream), the comparator's columns (QNAME, FLAG,
 * MAPQ, RNEXT, PNEXT, TLEN) and the record-state column; it WRITES the permutation, its items "sorted" / "sorted_qname", and the
 * bookkeeping of key passes made ahead (elp_sort_ahead). */
int elp_sort_coordinate(elp_ctx *ctx);
/* on != 0: the host announces that elp_sort_coordinate will follow elp_mark_duplicates on this context (what `elprep filter
 * --mark-duplicates --sorting-order coordinate` does, sam/filter-pipeline.go:116).  The sort's key passes read the coordinate keys only -
 * not the duplicate bits, which only the comparator's tail (modFlag, sam/sam-types.go:447-452) looks at - so elp_mark_duplicates queues
 * them on the sort lane as soon as it has made the keys, and they run while it finishes; elp_sort_coordinate then breaks the ties on the
 * final FLAGs.  Same permutation either way; without a sort behind it the option costs the passes' time.  (Measured with bench.py's step,
 * where the gather follows mark duplicates at once: no gain - the GPU is busy either way, profiles/round6_sort_ahead_ab.txt; it is for a
 * host that has work of its own between the two calls.) */
int elp_sort_ahead(elp_ctx *ctx, int on);
/* the permutation the context holds - made by elp_sort_coordinate, elp_sort_queryname or elp_order_keep, whichever ran last;
 * ELP_ERR_ARG if none of them has run since the staged records last changed */
int elp_get_permutation(elp_ctx *ctx, uint32_t *perm_out /* n */);
/* ---- queryname sort: By(QNAMELess).ParallelStableSort (sam/filter-pipeline.go:118-122, sam/sam-types.go:475-481, :639-641) ----
 * The Finalize step of `elprep filter / sfm --sorting-order queryname` (cmd/filter.go:361,451), in place of elp_sort_coordinate.
 * perm[k] = staging index of the record at sorted position k (elp_get_permutation).  Order: QNAME bytes as Go compares strings -
 * unsigned bytes, lexicographic, a proper prefix first ("" < "a" < "a0" < "b"); records with equal QNAMEs keep staging order (mates and
 * secondary / supplementary records of a template stay in arrival order).  The first elp_num_sorted() entries are the output; the
 * records that are not output (sr-tagged copies, records rejected by elp_filter_records) follow behind them, ALSO in QNAME order with
 * ties in staging order.  Reads the QNAME column and the record-state column only (no sort keys, no scores: nothing of
 * elp_mark_duplicates is needed), so it may be called on its own or after elp_mark_duplicates, elp_filter_records or
 * elp_sort_coordinate or elp_order_keep, with the same result.  The context remembers which call made its permutation last: elp_get_permutation and
 * elp_emit_sorted_bam / elp_emit_sorted_bgzf give that order; elp_merge_spread and elp_emit_merged_bam return ELP_ERR_UNSUPPORTED
 * while either context holds a queryname permutation (the reference panics: "Merging of files sorted by queryname not yet
 * implemented.", cmd/merge.go:175-176).  Key passes queued ahead for a coordinate sort (elp_sort_ahead) are left as they are.
 * Concurrency: as elp_sort_coordinate - the sort runs on the same side lane of the context (a stream, scratch pool and error words of
 * its own) and writes the permutation only; once elp_mark_duplicates has returned, a host may call it from a thread of its own WHILE
 * other threads call elp_dup_metrics and drive elp_bqsr_gather(_device) -> finalize -> elp_bqsr_apply on the same context.  Calls that
 * CHANGE staged records must not overlap with it.  Its thread READS the QNAME and record-state columns and WRITES the permutation and its
 * validity items "sorted" / "sorted_qname" (csrc/derived.hpp), nothing else of the context.  Limits as for staging: 2^32-16 records,
 * QNAMEs of at most 1000 bytes. */
int elp_sort_queryname(elp_ctx *ctx);
/* ---- no sort: `--sorting-order keep` (the default, cmd/filter.go:451), `unknown`, `unsorted` ----
 * The permutation of a run that does not sort.  Sam.AddNodes collects the alignments with StrictOrd(Slice) - input order - for Keep and
 * Unknown (sam/filter-pipeline.go:110-112) and with Seq(Slice), of which input order is one legal result, for Unsorted (:123-124);
 * effectiveSortingOrder (:208-225) turns a requested `coordinate` into Keep whenever the input header already says SO:coordinate - the
 * production case of a BAM the aligner's pipeline has sorted, which the reference writes in the order it came (a file sorted by
 * (refid, POS) alone is NOT in CoordinateLess's nine-key order: elp_sort_coordinate would reorder records the reference leaves alone).
 * The host's choice after effectiveSortingOrder: Keep / Unknown / Unsorted -> elp_order_keep, Coordinate -> elp_sort_coordinate,
 * Queryname -> elp_sort_queryname.
 * perm[0 .. elp_num_sorted()) = the records that are output (state 0 in the record-state column), perm[elp_num_sorted() .. n) = the
 * records that are not (sr-tagged copies, records rejected by elp_filter_records, elp_filter_exact_strict or
 * elp_replace_reference_dictionary).  by_split == 0: both parts in staging order.  by_split != 0: both parts ordered by split id
 * ascending (the split column, ids 0 .. 65535) with staging order inside a split: a context that holds several `elprep split` files
 * delivers them file after file (elp_emit_concat_bam wants this form of its groups context).
 * Reads: the record-state column, and the split-id column if by_split.  Writes: the permutation and its validity items "sorted",
 * "sorted_keep", "sorted_keep_by_split" (csrc/derived.hpp).  Nothing else is needed - no keys, no scores, no marks: call it on its own
 * or after any operator; n == 0 succeeds.  It replaces whatever permutation the context held, and a later elp_sort_coordinate or
 * elp_sort_queryname replaces it in turn; elp_get_permutation, elp_emit_sorted_bam and elp_emit_sorted_bgzf take it as any other (sizes,
 * the size query, BGZF framing, the tag filter and elp_set_replace_read_group act as before).  Every change to the staged records that
 * invalidates a sort's permutation invalidates this one; elp_split_classify invalidates it only if it was made with by_split != 0 (it
 * rewrites the column that order was made from).
 * Concurrency: as elp_sort_coordinate - the call runs on the same side lane of the context (a stream, scratch pool and error words of
 * its own) and writes the permutation only; once elp_mark_duplicates has returned, a host may call it from a thread of its own WHILE
 * other threads call elp_dup_metrics and drive elp_bqsr_gather(_device) -> finalize -> elp_bqsr_apply on the same context.  Calls that
 * CHANGE staged records must not overlap with it.  Key passes queued ahead for a coordinate sort (elp_sort_ahead) are left as they are.
 * Cost: by_split == 0 is a two-pass partition, about 6 bytes per record (the state byte twice, the permutation once); by_split != 0
 * is a stable radix sort of ceil((bits(max split id) + 1) / 8) passes and takes the by_split == 0 path when every split id is 0.
 * Errors: ELP_ERR_ARG for a NULL context, ELP_ERR_UNSUPPORTED for more than 2^32-16 records. */
int elp_order_keep(elp_ctx *ctx, int by_split);
/* number of records that survive RemoveOptionalReads = staged records without the sr tag: the first elp_num_sorted() entries of
 * the permutation (of either sort, or of elp_order_keep) are the output of the run, the tagged copies follow behind them */
uint64_t elp_num_sorted(const elp_ctx *ctx);

/* ---- mark duplicates: filters.MarkDuplicates (filters/mark-duplicates.go:398-445) ----
 * Sets FLAG |= 0x400 on the staged flag column exactly as the reference's fragment/pair tournaments do
 * (deterministic total order: score, then QNAME, then later arrival — the single-threaded execution of the
 * reference).  also_opticals is accepted for signature parity (it only changes which reads carry a LIBID temp). */
int elp_mark_duplicates(elp_ctx *ctx, int also_opticals);
int elp_get_flags(elp_ctx *ctx, uint16_t *flag_out /* n, staging order */);
/* adapted values of filters/mark-duplicates.go:79-110 (unclipped 5' position) and :57-68 (Phred-sum score);
 * 0 for records that are not duplicate-marking candidates.  Either pointer may be NULL. */
int elp_get_adapted(elp_ctx *ctx, int32_t *upos_out, int32_t *score_out);

/* ---- DuplicationMetrics counters: filters.MarkOpticalDuplicates (filters/mark-optical-duplicates.go:469-525) ----
 * counters: [(n_lib + 1)][7] int64 in the order UnpairedReadsExamined, ReadPairsExamined, SecondaryOrSupplementaryReads,
 * UnmappedReads, UnpairedReadDuplicates, ReadPairDuplicates, ReadPairOpticalDuplicates; row n_lib = "Unknown Library".
 * Requires elp_mark_duplicates.  Derived float metrics (PERCENT_DUPLICATION, ESTIMATED_LIBRARY_SIZE, :527-569) and the
 * Picard text (:608-699) stay on the host.  Runs on a side lane of the context (see elp_sort_coordinate): it reads what mark duplicates
 * left and writes nothing another call reads, so it may be called from a second host thread while the context sorts or gathers.
 * QNAMEs are parsed for tile / x / y (computeTileInfo, :50-71) where the reference parses them: every member of a strand list of 2 to
 * 300000 listed reads.  One of those whose tile / x / y field is not a strconv.ParseInt(s, 10, 64) integer fails the call with
 * ELP_ERR_DATA (the reference panics); a bad name anywhere else is not an error. */
#define ELP_NCTR 7
int elp_dup_metrics(elp_ctx *ctx, int optical_pixel_distance, int64_t *counters);
/* The same plus the three set-size histograms the reference keeps per library (duplicatesCountHistogram,
 * nonOpticalDuplicatesCountHistogram, opticalDuplicatesCountHistogram, filters/mark-optical-duplicates.go:104-174, 310-324):
 * hist = [(n_lib + 1)][3][hist_len] int64; a set of n listed reads with k optical duplicates counts into bin n of the first,
 * bin n - k (if > 0) of the second and bin k + 1 (if k > 0) of the third histogram; indices >= hist_len count into the last bin
 * (the reference's maps are unbounded); hist_len >= 2. */
int elp_dup_metrics_hist(elp_ctx *ctx, int optical_pixel_distance, int64_t *counters, int64_t *hist, int hist_len);

/* ---- BQSR inputs: NewBaseRecalibrator(knownSites, referenceFasta) (filters/bqsr.go:424-443) ----
 * bases = raw .elfasta bytes of one contig (fasta.MappedFasta.Seq, fasta/fasta-files.go:355);
 * start_end = known-site intervals [n][2], 1-based inclusive, ALREADY sorted by start and flattened
 * (intervals.ParallelSortByStart + ParallelFlatten, intervals/intervals.go:77-132) — the host keeps doing that. */
int elp_bqsr_set_reference(elp_ctx *ctx, int32_t refid, const uint8_t *bases, int64_t len);
int elp_bqsr_set_known_sites(elp_ctx *ctx, int32_t refid, const int32_t *start_end, int64_t n);

/* ---- BQSR gather: BaseRecalibrator.Recalibrate (filters/bqsr.go:467-551) ----
 * Walks the records in any order (integer sums) and fills dense {observations, mismatches} int64 tables:
 *   qual_tbl  [n_cov][94][2]
 *   cycle_tbl [n_cov][94][2*max_cycle+1][2]     cycle c at index c + max_cycle
 *   ctx_tbl   [n_cov][94][16][2]                context key k (filters/bqsr.go:64-76) at index (k >> 4) & 15
 * A Go map entry of the reference exists iff observations > 0.  Uses the staged flag column (duplicates excluded,
 * recalibrateAln filters/bqsr.go:225-244), so call after elp_mark_duplicates. */
#define ELP_NQUAL 94
#define ELP_NCTX 16
int elp_bqsr_gather(elp_ctx *ctx, int max_cycle, int64_t *qual_tbl, int64_t *cycle_tbl, int64_t *ctx_tbl);

/* The same, but the tables stay in HBM (ctx-owned) for the device group's all-reduce below; elp_bqsr_tables_fetch copies them out.
 * The copy runs on a stream of its own behind the last writer of the tables, and it is the ONE call that may run on a second host
 * thread while the context is busy with another call (elp_dup_metrics): the host fetches and finalises the tables while the GPU
 * counts optical duplicates - the two steps the reference runs one after the other (cmd/filter.go:162-196). */
int elp_bqsr_gather_device(elp_ctx *ctx, int max_cycle);
int elp_bqsr_tables_fetch(elp_ctx *ctx, int64_t *qual_tbl, int64_t *cycle_tbl, int64_t *ctx_tbl);
/* The rows form of the device tables (round 5): with many read groups the dense tables are tens of megabytes around a few hundred rows
 * that hold anything (a Go map of the reference has those entries only, filters/bqsr.go:445-459).  elp_bqsr_quals_counted: bit q of
 * bits[q / 64] = quality q had table slots in the gather that made the tables (no other quality's rows hold anything).
 * elp_bqsr_tables_fetch_rows: the rows of `quals` only - q_rows [n_cov][n_quals][2], c_rows [n_cov][n_quals][2*max_cycle+1][2], x_rows
 * [n_cov][n_quals][16][2]; returns 1 and copies nothing if a quality that was not asked for has observations (tables summed with
 * another context's or rank's: fetch the dense tables then).  Same threading rule as elp_bqsr_tables_fetch. */
int elp_bqsr_quals_counted(elp_ctx *ctx, uint64_t *bits /* [2] */);
int elp_bqsr_tables_fetch_rows(elp_ctx *ctx, const uint8_t *quals, int n_quals, int64_t *q_rows, int64_t *c_rows, int64_t *x_rows);

/* ---- device group and its one collective: the table / metrics combination of `elprep sfm`'s merge phase ----
 * LoadAndCombineBQSRTables (filters/print-bqsr.go:310-329) and LoadAndCombineDuplicateMetrics
 * (filters/mark-optical-duplicates.go:711-731) sum what the per-split `filter --bqsr-tables-only` runs produced.  One process per
 * GPU; rank 0 makes the group id (RCCL's ncclUniqueId) and the host hands it to the other ranks by whatever channel it has (the Go
 * host: a file next to the split files, or its parent `sfm` process); every rank then joins with its context.  A group of one needs
 * no id and makes every collective a no-op.
 *   elp_bqsr_tables_add        dst += src on the device: the contexts (splits) of ONE rank are summed before the collective
 *   elp_bqsr_tables_allreduce  ONE ncclAllReduce(ncclInt64, ncclSum) over xGMI, in place on the tables in HBM; `counters`
 *                              (n_counters <= 4096 int64 in host memory, e.g. the duplication counters) ride behind the tables
 *                              through the same call and come back summed
 *   elp_allreduce_i64          the same collective for a plain host buffer */
#define ELP_GROUP_ID_BYTES 128
int elp_group_probe(void); /* 0 if the communication library (RCCL) can be loaded and has every entry point the group needs; no GPU needed */
int elp_group_unique_id(uint8_t *id_out /* ELP_GROUP_ID_BYTES */);
int elp_group_init(elp_ctx *ctx, int rank, int world, const uint8_t *id /* ELP_GROUP_ID_BYTES; may be NULL if world == 1 */);
/* The same group over a transport of the caller's (a host without RCCL, or a host program that already has its own communicator - MPI,
 * gloo, the Go side's net/rpc): `allreduce` must sum `n` int64 values over all ranks, in place, and return 0; it is called on the calling
 * thread of elp_bqsr_tables_allreduce / elp_allreduce_i64 with a page-locked host buffer (the device tables make one round trip over PCIe).
 * Replaces: nothing in the reference (elprep sfm merges per-split tables through files, cmd/split-filter-merge.go:413-470). */
typedef int (*elp_allreduce_fn)(void *user, int64_t *values, size_t n);
int elp_group_init_transport(elp_ctx *ctx, int rank, int world, elp_allreduce_fn allreduce, void *user);
/* Point-to-point messages of such a group: `sendrecv` must deliver send_bytes from send_buf to rank send_peer and fill recv_buf with the
 * recv_bytes that rank recv_peer sends to this rank in its matching call (a peer of -1: nothing that way), then return 0; page-locked
 * host buffers.  An RCCL group (elp_group_init) needs no callback: ncclSend / ncclRecv over xGMI, device to device. */
typedef int (*elp_sendrecv_fn)(void *user, int send_peer, const void *send_buf, size_t send_bytes, int recv_peer, void *recv_buf, size_t recv_bytes);
int elp_group_set_p2p(elp_ctx *ctx, elp_sendrecv_fn sendrecv, void *user);
/* The split phase of `elprep sfm` between PROCESSES (sam/split-merge.go:280-293 writes a record to the file of the split it belongs
 * to; with one process per GPU the "file" is a context of another rank): one step of the all-to-all.  The records `idx` (staging
 * indices, n of them) of `src` are gathered on its GPU as elp_copy_records gathers them - new_split / tag_sr as there - and sent to rank
 * send_peer of the device group; the records that rank recv_peer selected for this rank in ITS matching call are appended to `dst`.  Either
 * direction may be absent (peer -1; then src resp. dst may be NULL).  Every rank calls it world - 1 times, step s with send_peer =
 * (rank + s) % world and recv_peer = (rank - s + world) % world; src or dst must belong to the group.  No host copy of a record: the
 * records move in pieces of at most 4 M records (columns below 4 GiB each); per piece and direction a 160-byte header (with the sender's
 * status), an 8-byte verdict back from the receiver, then three device buffers (fixed columns, variable-length pools, scans).  A failure
 * on either side of a direction reaches the other side in the header or the verdict: both calls return an error, neither waits in a
 * message its peer will not post. */
int elp_exchange_records(elp_ctx *src, int send_peer, const uint32_t *idx, uint64_t n, int new_split, int tag_sr, elp_ctx *dst, int recv_peer);
/* elp_group_share: `ctx` joins the device group `member` belongs to by BORROWING its communicator / transport (same process, same
 * device; `member` must outlive the use, calls of the two contexts on the group must not overlap): the reader context of the split phase
 * exchanges records through the group the rank's processing context reduces its tables in - one communicator per rank. */
int elp_group_share(elp_ctx *ctx, elp_ctx *member);
int elp_group_rank(const elp_ctx *ctx);
int elp_group_size(const elp_ctx *ctx);
int elp_bqsr_tables_add(elp_ctx *dst, elp_ctx *src);
int elp_bqsr_tables_allreduce(elp_ctx *ctx, int64_t *counters, size_t n_counters);
int elp_allreduce_i64(elp_ctx *ctx, int64_t *buf, size_t n);

/* ---- BQSR apply: BaseRecalibratorTables.ApplyBQSR (filters/bqsr.go:936-1005) ----
 * lut: [n_cov][94][2*max_cycle+1][17] bytes = the reference's memo map applyKey{rg, qual, cycle, context} -> uint8,
 * densely tabulated by the host from the finalized tables (context index 16 = key -1); cov_present[c] = 0 means the read
 * group is absent from the tables (read left untouched, :953-955).  Rewrites the staged qual column in place. */
int elp_bqsr_apply(elp_ctx *ctx, int max_cycle, const uint8_t *lut, const uint8_t *cov_present);
/* The LUT's way to the device ahead of the call: from the thread that built it (Go: the goroutine that ran FinalizeBQSRTables), on a copy
 * stream of the context, while other calls (sort, metrics) run on the context from another thread; elp_bqsr_apply(ctx, max_cycle, NULL,
 * NULL) then uses it.  The only other call that may share a context with running calls is elp_bqsr_tables_fetch.  Ordering the
 * caller must keep: no staging call (elp_stage*, elp_reset, elp_rollback) and no elp_bqsr_gather* runs on the context at the same time -
 * the upload reads the staged read length and the gather's quality hint without a lock; sort, metrics, emit and tables_fetch may.
 * A `lut` in page-locked memory (elp_pinned_alloc) is copied from where it lies (no staging copy: with 16 read groups the LUT is 25 MB):
 * the caller then leaves it unchanged until the elp_bqsr_apply that uses it has been called and the context synchronised. */
int elp_bqsr_lut_upload(elp_ctx *ctx, int max_cycle, const uint8_t *lut, const uint8_t *cov_present);
/* The same for the LUT in rows form: rows [n_cov][n_quals][2*max_cycle+1][17] for the qualities `quals`, defaults [n_cov][94] = the one byte
 * every other (read group, quality) row consists of (a row without cycle and context entries is its prior whatever the cycle and the
 * context); the dense LUT is made from them on the device.  With 16 read groups 1.9 MB instead of 25.6 MB cross PCIe. */
int elp_bqsr_lut_upload_rows(elp_ctx *ctx, int max_cycle, const uint8_t *quals, int n_quals, const uint8_t *rows, const uint8_t *defaults,
                             const uint8_t *cov_present);
int elp_get_qual(elp_ctx *ctx, uint8_t *qual_out /* qual_bytes, staging order and offsets */);

/* ---- CleanSam (filters/simple-filters.go:292-306, `elprep filter --clean-sam`: a filter of the phase-1 pipeline, cmd/filter.go:747) ----
 * On the staged records, in front of elp_mark_duplicates: MAPQ of unmapped reads becomes 0; an alignment whose End() lies behind the
 * LN of its reference sequence is soft-clipped there by softClipEndOfRead (filters/utils.go:102-119) - with that function's arithmetic as
 * it stands in the reference (the running position accumulates, the clip's length is ReadLengthFromCigar + clipFrom): a drop-in writes
 * what the reference writes.  The CIGAR column is rebuilt if any record is rewritten (a rewritten CIGAR can be one operation longer).
 * n_clipped_out (may be NULL): records rewritten.  ELP_ERR_DATA where the reference panics ("Unexpected non-0 relative clipping
 * position in CleanSam."), ELP_ERR_UNSUPPORTED for a clip length that does not fit the 28 bits of a BAM CIGAR field. */
int elp_clean_sam(elp_ctx *ctx, uint64_t *n_clipped_out);

/* ---- the HaplotypeCaller's Smith-Waterman: runSmithWaterman (filters/sw.go:110-316; csrc/sw.hip, sw_core.hpp, sw_plan.hpp) ----
 * The one kernel of the HaplotypeCaller whose arithmetic is all int32.  The reference calls it once per read of every assembly region
 * against the read's best haplotype (filters/realign.go:310: 10, -15, -30, -5, softclip), per dangling tail or head
 * (filters/assemble-reads.go:1042,1152: 25, -50, -110, -6, leadingIndel) and per haplotype through calculateCigar (filters/sw.go:401: 200,
 * -150, -260, -11, softclip).  A batch is a pool of reference sequences, a pool of alternate sequences - bytes as the Go strings hold
 * them, sequence s of a pool = pool[off[s] .. off[s + 1]) - and n problems (ref_of[k], alt_of[k]); both forms are flat (cgo: no
 * pointers to pointers).  elp_sw_align_reads takes its alternates from staged records: problem k's is SEQ.AsString() of staged record
 * read_idx[k] (any order, repeats allowed), the nibbles decoded by "=ACMGRSVTWYHKDBN" - from the BAM records of elp_stage_bam /
 * elp_stage_bgzf / elp_stage_sam, because column staging (elp_stage) keeps A, C, G, T and "other" only: ELP_ERR_ARG there.
 *   Result, exactly what runSmithWaterman returns: problem k's CIGAR is cigar_out[cigar_off_out[k] .. cigar_off_out[k + 1]) in BAM's
 * len << 4 | op words as elp_batch.cigar holds them (only M, I, D and S occur), its alignment offset offset_out[k] (negative offsets
 * included: `ignore` returns p1 - p2).  *n_ops_out = all operations.  A CIGAR never has more than len(ref) + len(alt) + 2 operations
 * (the traceback makes at most len(ref) + len(alt) steps, each at most one segment, the tails add two, and a leading S takes at least one step away), so a buffer of the sum of
 * that over the problems always suffices; if *n_ops_out exceeds cigar_cap the call returns ELP_ERR_ARG, *n_ops_out holds the need and
 * the output arrays are unspecified.  n == 0 succeeds with cigar_off_out[0] = 0.
 *   What is reproduced (sw.go line by line): the exact-substring shortcut of softclip and ignore (:113-118) - the LAST occurrence of the
 * raw alternate in the reference under fasta.ToUpperAndN (lastIndex, :96-108: acgtn / ACGTN -> ACGTN, the other IUPAC letters -> N); the
 * recurrence on raw bytes with bestGap += gapExtend in front of the strict test, diagonal if >= both, else right if >= down, else down,
 * interior cells clamped at -100000000 and the first row and column of indel / leadingIndel not clamped (:141-210); the end search
 * (:212-238); the traceback, the three strategy tails, the reversal and the clean-up loop as it stands, which does not compare the
 * element in front of a removed zero-length one with what moves up (:240-315).
 *   Stated limits (ELP_ERR_UNSUPPORTED): a sequence (one that a problem uses) longer than 4095 bytes - a gap length then fits the int16 the
 * backtrack is stored in -, a parameter whose absolute value exceeds 65535, 2^31 or more problems.  With both limits no int32 of the
 * reference can wrap: bestGap starts at MinInt32 / 2 = -1073741824 and falls by at most 4095 * 65535 = 268365825 to -1342107649 >
 * MinInt32 = -2147483648; a score is a sum of at most 8190 parameters, within +-536731650 < 2^30.
 *   ELP_ERR_ARG: a NULL context or output pointer, strategy outside 0 .. 3, offsets that do not start at 0 or decrease, an index outside
 * its pool, read_idx[k] >= elp_num_records, and an EMPTY sequence that a problem uses (the reference's answer there - a 0M, or an
 * out-of-range index - is an accident of its loops; it is refused, not reproduced).
 *   The call runs on the context's stream, reads the staged records and nothing else of the context, changes no staged or derived
 * state, and uses the context's scratch (sw_plan.hpp lists the slots); as every call on one context it must not overlap another.
 * The problems that miss the shortcut run in chunks of at most 1 GiB of scratch (elp_set_tuning "sw_scratch_bytes"). */
typedef enum elp_sw_strategy { ELP_SW_SOFTCLIP = 0, ELP_SW_INDEL = 1, ELP_SW_LEADING_INDEL = 2, ELP_SW_IGNORE = 3 } elp_sw_strategy; /* sw.go:31-36 */
int elp_sw_align(elp_ctx *ctx, uint64_t n_a, const uint8_t *a, const uint64_t *a_off /* n_a + 1 */, uint64_t n_b, const uint8_t *b, const uint64_t *b_off /* n_b + 1 */,
                 uint64_t n, const uint32_t *ref_of /* n, index into a */, const uint32_t *alt_of /* n, index into b */, int32_t match, int32_t mismatch, int32_t gap_open,
                 int32_t gap_extend, int strategy, uint32_t *cigar_out, uint64_t cigar_cap /* in ops */, uint64_t *cigar_off_out /* n + 1 */, int32_t *offset_out /* n */,
                 uint64_t *n_ops_out);
int elp_sw_align_reads(elp_ctx *ctx, uint64_t n_a, const uint8_t *a, const uint64_t *a_off, uint64_t n, const uint32_t *ref_of, const uint32_t *read_idx /* n staging indices */,
                       int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int strategy, uint32_t *cigar_out, uint64_t cigar_cap, uint64_t *cigar_off_out,
                       int32_t *offset_out, uint64_t *n_ops_out);

/* Measurement and test harness entry points of the same library (snapshot / rollback of the mutable columns, pinned kernel choices, per-kernel
 * timing) are declared in elprep_hip_debug.h: they are not part of the reference's interface and a drop-in host does not need them. */

#ifdef __cplusplus
}
#endif
#endif /* ELPREP_HIP_H */
