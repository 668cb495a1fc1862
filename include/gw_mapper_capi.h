/*
 * gw_mapper_capi.h -- flat C API of cudamapper (libcudamapper.so), for foreign-function bindings
 * (genomeworks_amd/cudamapper.py): index creation from host reads, the anchor matcher, the triggered overlapper, one
 * call for a whole mapping of one index pair, overlap post-processing, end rescue and alignment of overlaps into
 * CIGARs, their cutting into POA windows for polishing, their pileups, packed host copies of indices, the index batcher and the cached batched driver behind the cudamapper tool.
 * Functions returning int give 0 on success; those returning a count give it, or GW_MAPPER_ERROR; creators return NULL.
 * On an error the exception text is in gw_mapper_last_error().
 *
 * Reads are passed as one byte array and n_reads + 1 offsets: read i is bases[offsets[i] .. offsets[i+1]).
 * Anchors use the layout of cudamapper::Anchor (4 x uint32, 16 B), overlaps that of cudamapper::Overlap (36 B).
 */
#ifndef GW_MAPPER_CAPI_H
#define GW_MAPPER_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GW_MAPPER_ERROR (-1)

typedef struct gw_mapper_index gw_mapper_index;
typedef struct gw_mapper_matcher gw_mapper_matcher;

/* last error (exception text) of the calling thread */
const char* gw_mapper_last_error(void);

/* Index::create_index_async + wait_to_be_ready over reads first_read_id .. first_read_id + n_reads - 1. */
gw_mapper_index* gw_mapper_index_create(const char* bases, const int64_t* offsets, int32_t n_reads,
                                        uint32_t first_read_id, int32_t kmer_size, int32_t window_size,
                                        int32_t hash_representations, double filtering_parameter, void* stream);
void gw_mapper_index_destroy(gw_mapper_index* index);

/* sizes[3]: representations, unique_representations, first_occurrence_of_representations;
   reads[4]: number_of_reads, smallest_read_id, largest_read_id, number_of_basepairs_in_longest_read;
   stage_ms[4]: device time of sketch, sort, unique, filter. Any pointer may be NULL. */
int gw_mapper_index_info(const gw_mapper_index* index, int64_t* sizes, uint32_t* reads, float* stage_ms);

/* copies the index arrays (sizes from gw_mapper_index_info) to host; any pointer may be NULL */
int gw_mapper_index_copy(const gw_mapper_index* index, uint64_t* representations, uint32_t* read_ids,
                         uint32_t* positions_in_reads, uint8_t* directions, uint64_t* unique_representations,
                         uint32_t* first_occurrence_of_representations);

/* test hook: an index from host arrays (see gwm_index_from_arrays in gwhip_mapper.h), for the matcher on hand-built
   indices */
gw_mapper_index* gw_mapper_index_from_arrays(int64_t n, const uint32_t* read_ids, const uint32_t* positions_in_reads,
                                             int64_t n_unique, const uint64_t* unique_representations,
                                             const uint32_t* first_occurrence_of_representations,
                                             uint32_t first_read_id, uint32_t number_of_reads,
                                             uint32_t number_of_basepairs_in_longest_read);

/* Matcher::create_matcher(query, target): the sorted anchors stay on the device */
gw_mapper_matcher* gw_mapper_matcher_create(const gw_mapper_index* query, const gw_mapper_index* target, void* stream);
void gw_mapper_matcher_destroy(gw_mapper_matcher* matcher);
int64_t gw_mapper_matcher_anchor_count(const gw_mapper_matcher* matcher);
/* copies min(capacity, count) anchors; stage_ms[2] (match, anchor sort) may be NULL */
int gw_mapper_matcher_copy_anchors(const gw_mapper_matcher* matcher, void* anchors, int64_t capacity, float* stage_ms);

/* Overlapper::get_overlaps over the matcher's anchors. `overlaps` needs room for anchor_count / 3 + 1 records (a kept
   chain holds at least 3 anchors); negative thresholds are an error. Returns the
   number of overlaps; chain_fuse_filter_ms may be NULL. */
int64_t gw_mapper_get_overlaps(const gw_mapper_matcher* matcher, int32_t all_to_all, int64_t min_residues,
                               int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
                               void* overlaps, float* chain_fuse_filter_ms, void* stream);

/* the same over n sorted host anchors (uploaded first); `overlaps` needs room for n / 3 + 1 records */
int64_t gw_mapper_get_overlaps_host(const void* anchors, int64_t n, int32_t all_to_all, int64_t min_residues,
                                    int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
                                    void* overlaps, void* stream);

/* The chaining overlapper over the matcher's anchors (gwm_chain_overlaps in gwhip_mapper.h has rules C1-C8).
   chaining[5] = kmer_size, max_gap, bandwidth, min_chain_score, max_chains. Writes min(capacity, count) records to
   `overlaps` and as many int32 chain scores to `scores` (either may be NULL) and returns count, or GW_MAPPER_ERROR
   with nothing written; chain_ms may be NULL. */
int64_t gw_mapper_chain_overlaps(const gw_mapper_matcher* matcher, const int32_t chaining[5], int32_t all_to_all,
                                 int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                 float min_overlap_fraction, void* overlaps, int32_t* scores, int64_t capacity,
                                 float* chain_ms, void* stream);

/* the same over n sorted host anchors (uploaded first) */
int64_t gw_mapper_chain_overlaps_host(const void* anchors, int64_t n, const int32_t chaining[5], int32_t all_to_all,
                                      int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                      float min_overlap_fraction, void* overlaps, int32_t* scores, int64_t capacity,
                                      float* chain_ms, void* stream);

/* gw_mapper_chain_overlaps that also hands out the chains (gwm_chain_overlaps_anchored): for the records written,
   anchor_offsets[min(capacity, count) + 1] (int64) and, as far as anchor_capacity pairs reach, their anchors in chain
   order as (query_position_in_read, target_position_in_read) pairs of uint32 in anchor_positions; twice the anchor
   count always suffices. *n_chain_anchors is the number of pairs of all kept records. Any output may be NULL. */
int64_t gw_mapper_chain_overlaps_anchored(const gw_mapper_matcher* matcher, const int32_t chaining[5], int32_t all_to_all,
                                          int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                          float min_overlap_fraction, void* overlaps, int32_t* scores, int64_t capacity,
                                          int64_t* anchor_offsets, uint32_t* anchor_positions, int64_t anchor_capacity,
                                          int64_t* n_chain_anchors, float* chain_ms, void* stream);

/* the same over n sorted host anchors (uploaded first) */
int64_t gw_mapper_chain_overlaps_anchored_host(const void* anchors, int64_t n, const int32_t chaining[5],
                                               int32_t all_to_all, int64_t min_residues, int64_t min_overlap_len,
                                               int64_t min_bases_per_residue, float min_overlap_fraction, void* overlaps,
                                               int32_t* scores, int64_t capacity, int64_t* anchor_offsets,
                                               uint32_t* anchor_positions, int64_t anchor_capacity,
                                               int64_t* n_chain_anchors, float* chain_ms, void* stream);

/* Whole mapping of one index pair: queries against targets, or all against all when target_bases is NULL
   (all_to_all then drops self-mappings). Writes min(capacity, count) overlaps and returns count. */
int64_t gw_mapper_map(const char* query_bases, const int64_t* query_offsets, int32_t n_queries,
                      const char* target_bases, const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size,
                      int32_t window_size, double filtering_parameter, int64_t min_residues, int64_t min_overlap_len,
                      int64_t min_bases_per_residue, float min_overlap_fraction, void* overlaps, int64_t capacity,
                      void* stream);

/* ---- what cudamapper does with the overlaps of an index pair before it prints them -------------------------------
   The rules are spelled out next to gwm_post_process_overlaps / gwm_rescue_overlap_ends in gwhip_mapper.h. */

/* Overlapper::post_process_overlaps over n host overlaps: the originals (without the members of fusing pairs when
   drop_fused_overlaps is set), then one fused record per run. Returns their number (at most n + n / 2) and writes
   min(capacity, count) of them to `out`; fuse_ms (device time) may be NULL. */
int64_t gw_mapper_post_process_overlaps(const void* overlaps, int64_t n, int32_t drop_fused_overlaps, void* out,
                                        int64_t capacity, void* stream, float* fuse_ms);

/* Overlapper::rescue_overlap_ends over n host overlaps, in place. Query and target reads as everywhere in this
   header; target_bases NULL means the target set is the query set. Read id r is read r - first_*_read_id of its
   set. 0 <= extension <= 78. A read id outside its set, or a start or end beyond its read (undefined behaviour or an
   exception in the reference), is an error: GW_MAPPER_ERROR, and the overlaps are left as they were. */
int gw_mapper_rescue_overlap_ends(void* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                                  int32_t n_queries, const char* target_bases, const int64_t* target_offsets,
                                  int32_t n_targets, uint32_t first_query_read_id, uint32_t first_target_read_id,
                                  int32_t extension, float required_similarity, void* stream, float* rescue_ms);

/* gwm_extend_overlaps of gwhip_mapper.h over n host overlaps, in place: the ends moved by the affine X-drop extension.
   Reads and read ids as for gw_mapper_rescue_overlap_ends. extension[0..5] = match, mismatch, gap_open, gap_extend, band,
   xdrop; 0 <= max_extension <= 2^19. extensions: host, [n][4] = head q, head t, tail q, tail t; scores: host, [n][2]. On an
   error (GW_MAPPER_ERROR: a value out of range, a read id outside its set, an overlap beyond its read) the overlaps are
   left as they were. */
int gw_mapper_extend_overlaps(void* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                              int32_t n_queries, const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                              uint32_t first_query_read_id, uint32_t first_target_read_id, const int32_t* extension,
                              int32_t max_extension, int64_t max_device_bytes, void* stream, int32_t* extensions,
                              int32_t* scores);

/* CIGARs of n host overlaps over host reads (uploaded for the call; target_bases NULL means the target set is the
   query set): gwm_align_overlaps of gwhip_mapper.h, which states slices, strand, complement, aligner and text format.
   A read id outside its set, start > end or an end beyond its read is an error (NULL). The CIGARs stay on the device
   until gw_mapper_cigars_copy: text (text_bytes bytes, back to back), offsets[count + 1], edit_distances[count]
   (-1: the aligner gave no result), stage_ms[3] (device time of gather, align, CIGAR text); any pointer may be NULL. */
typedef struct gw_mapper_cigars gw_mapper_cigars;
gw_mapper_cigars* gw_mapper_align_overlaps(const void* overlaps, int64_t n, const char* query_bases,
                                           const int64_t* query_offsets, int32_t n_queries,
                                           uint32_t first_query_read_id, const char* target_bases,
                                           const int64_t* target_offsets, int32_t n_targets,
                                           uint32_t first_target_read_id, int64_t max_device_bytes, void* stream);
/* The same under affine gap costs (gwm_align_overlaps_scored of gwhip_mapper.h): scoring[0..3] = mismatch (1..255),
   gap_open (0..255), gap_extend (1..255), band (>= 0); NULL is gw_mapper_align_overlaps itself. A scoring out of range is
   refused before anything reaches the device (NULL). An overlap whose band has more than 2048 diagonals has an empty
   CIGAR and edit distance -1. */
gw_mapper_cigars* gw_mapper_align_overlaps_scored(const void* overlaps, int64_t n, const char* query_bases,
                                                  const int64_t* query_offsets, int32_t n_queries,
                                                  uint32_t first_query_read_id, const char* target_bases,
                                                  const int64_t* target_offsets, int32_t n_targets,
                                                  uint32_t first_target_read_id, const int32_t* scoring,
                                                  int64_t max_device_bytes, void* stream);
/* The same under two-piece gap costs (gwm_align_overlaps_scored2): scoring[0..5] = mismatch, gap_open, gap_extend,
   gap_open2 (0..255), gap_extend2 (1..255), band; NULL is gw_mapper_align_overlaps itself. Refused out of range before
   anything reaches the device (NULL). An overlap whose band has more than 1024 diagonals has an empty CIGAR and -1. */
gw_mapper_cigars* gw_mapper_align_overlaps_scored2(const void* overlaps, int64_t n, const char* query_bases,
                                                   const int64_t* query_offsets, int32_t n_queries,
                                                   uint32_t first_query_read_id, const char* target_bases,
                                                   const int64_t* target_offsets, int32_t n_targets,
                                                   uint32_t first_target_read_id, const int32_t* scoring,
                                                   int64_t max_device_bytes, void* stream);
/* The same with every overlap cut at anchors of its chain and aligned piece by piece (gwm_align_overlaps_anchored of
   gwhip_mapper.h has rules G1-G6). Overlap i has the host anchors anchor_positions[anchor_offsets[i] ..
   anchor_offsets[i + 1]) as (query, target) pairs of uint32, what gw_mapper_chain_overlaps_anchored returns;
   anchor_kmer_size 1..32, anchor_spacing >= 1. scoring_values 0: the default aligner; 4: scoring[0..3] as for
   gw_mapper_align_overlaps_scored; 6: scoring[0..5] as for gw_mapper_align_overlaps_scored2. Refused before anything
   reaches the device (NULL): a scoring, k or S out of range, another scoring_values, offsets that do not start at 0,
   decrease, or do not end at n_anchors. Valid anchors of a record that are not strictly increasing are an error that
   names the record. */
gw_mapper_cigars* gw_mapper_align_overlaps_anchored(const void* overlaps, int64_t n, const char* query_bases,
                                                    const int64_t* query_offsets, int32_t n_queries,
                                                    uint32_t first_query_read_id, const char* target_bases,
                                                    const int64_t* target_offsets, int32_t n_targets,
                                                    uint32_t first_target_read_id, const int64_t* anchor_offsets,
                                                    const uint32_t* anchor_positions, int64_t n_anchors,
                                                    int32_t anchor_kmer_size, int32_t anchor_spacing,
                                                    const int32_t* scoring, int32_t scoring_values,
                                                    int64_t max_device_bytes, void* stream);
int64_t gw_mapper_cigars_count(const gw_mapper_cigars* cigars);
int64_t gw_mapper_cigars_text_bytes(const gw_mapper_cigars* cigars);
int gw_mapper_cigars_copy(const gw_mapper_cigars* cigars, char* text, int64_t* offsets, int32_t* edit_distances,
                          float* stage_ms);
void gw_mapper_cigars_destroy(gw_mapper_cigars* cigars);

/* ---- polishing: aligned overlaps cut into POA windows --------------------------------------------------------------
   The target reads are cut into windows of window_length bases; every window is its backbone, target[k W, end_k),
   followed by its layers: the slices of the query reads whose alignment spans the window. Segments are
   gwm_window_segments of gwhip_mapper.h (24 B records of six uint32: overlap, window, target_first, target_last,
   query_begin, query_end); the selection rules are spelled out next to gwm::select_layers in mapper/gwm_windows.hpp and
   in INTEGRATION.md section 3j. */

/* The windows of n host overlaps over host reads (target_bases NULL: the target set is the query set). The reads are
   uploaded once; the overlaps are aligned as gw_mapper_align_overlaps aligns them and their segments written on the
   device; the records (24 B each) are copied to the host, where the layers are selected; then the sequences of every
   window are gathered on the device and copied out once. Errors as for gw_mapper_align_overlaps, plus
   window_length < 1 and max_depth < 0 (NULL). */
typedef struct gw_mapper_windows gw_mapper_windows;
gw_mapper_windows* gw_mapper_window_overlaps(const void* overlaps, int64_t n, const char* query_bases,
                                             const int64_t* query_offsets, int32_t n_queries,
                                             uint32_t first_query_read_id, const char* target_bases,
                                             const int64_t* target_offsets, int32_t n_targets,
                                             uint32_t first_target_read_id, int32_t window_length, int32_t max_depth,
                                             int64_t max_device_bytes, void* stream);
/* The segments pass of gw_mapper_window_overlaps alone: reads and overlaps uploaded, the segment records, their
   offsets and the edit distances copied out; no selection, no gather, so the window counts are 0 and the fourth
   stage time is 0. */
gw_mapper_windows* gw_mapper_window_segments(const void* overlaps, int64_t n, const char* query_bases,
                                             const int64_t* query_offsets, int32_t n_queries,
                                             uint32_t first_query_read_id, const char* target_bases,
                                             const int64_t* target_offsets, int32_t n_targets,
                                             uint32_t first_target_read_id, int32_t window_length,
                                             int64_t max_device_bytes, void* stream);
/* counts[4]: windows, sequences, bases, segments */
int gw_mapper_windows_counts(const gw_mapper_windows* windows, int64_t* counts);
/* segments (24 B each), segment_offsets[n + 1], edit_distances[n] (as gw_mapper_cigars_copy) and stage_ms[4]: device
   time of gather, align, segments and the window gather; any pointer may be NULL */
int gw_mapper_windows_copy_segments(const gw_mapper_windows* windows, void* segments, int64_t* segment_offsets,
                                    int32_t* edit_distances, float* stage_ms);
/* bases (back to back), sequence_offsets[sequences + 1], and per window its number of sequences (backbone first), its
   target read (position in the target set) and its index in that read; windows come by target read, then by index.
   Any pointer may be NULL. */
int gw_mapper_windows_copy_windows(const gw_mapper_windows* windows, char* bases, int64_t* sequence_offsets,
                                   int32_t* sequences_per_window, uint32_t* window_target_read, uint32_t* window_index);
void gw_mapper_windows_destroy(gw_mapper_windows* windows);

/* The selection alone, over host arrays; it needs no device. Returns the number of sequences, or GW_MAPPER_ERROR;
   *n_windows is the number of windows. plan (5 uint32 per sequence: set -- 0 query, 1 target --, read, begin, end,
   reversed) and window_table (4 uint32 per window: target read, window, first sequence, sequences) are written when
   they are not NULL and their capacities (in sequences / windows) suffice. */
int64_t gw_mapper_select_layers(const void* segments, int64_t n_segments, const void* overlaps, int64_t n_overlaps,
                                int32_t n_queries, uint32_t first_query_read_id, const int64_t* target_lengths,
                                int32_t n_targets, uint32_t first_target_read_id, int32_t window_length,
                                int32_t max_depth, uint32_t* plan, int64_t plan_capacity, int64_t* n_windows,
                                uint32_t* window_table, int64_t window_capacity);

/* ---- read correction: POA windows of both reads from one alignment --------------------------------------------------
   There is one read set, and the overlaps are those of the set mapped against itself. The rules (C1 to C4) are in
   INTEGRATION.md section 3k and next to gwm::select_pairs / gwm::select_correction_layers in mapper/gwm_windows.hpp. */

/* C1, over host records; it needs no device. Records of a read with itself are dropped; per unordered pair of reads
   the record with the greatest query end - query start is kept, on ties the first. Returns the number of pairs, or
   GW_MAPPER_ERROR; positions (input positions of the pairs, ascending) is written when it is not NULL and capacity
   suffices. */
int64_t gw_mapper_select_pairs(const void* overlaps, int64_t n_overlaps, int64_t* positions, int64_t capacity);

/* C3 and C4, over host arrays; it needs no device. target_role / query_role: the records of gwm_pair_segments for
   `pairs`. Returns, and writes plan and window_table, as gw_mapper_select_layers does; every plan entry is of set 0
   and a window's "target read" is the read that owns it. */
int64_t gw_mapper_select_correction_layers(const void* target_role, int64_t n_target_role, const void* query_role,
                                           int64_t n_query_role, const void* pairs, int64_t n_pairs,
                                           const int64_t* read_lengths, int32_t n_reads, uint32_t first_read_id,
                                           int32_t window_length, int32_t max_depth, uint32_t* plan, int64_t plan_capacity,
                                           int64_t* n_windows, uint32_t* window_table, int64_t window_capacity);

/* The windows of every read of the set: pairs selected on the host (C1), uploaded and aligned once each, the records of
   both roles written on the device (gwm_pair_segments) and copied to the host, the layers selected there (C3, C4), the
   sequences gathered on the device and copied out once. All windows of all reads are built at once: the handle holds
   the bases of every backbone and layer, at most (1 + max_depth) sequences of up to 2 * window_length bases per
   window, and the device holds the read set once plus that gather. The accessors of gw_mapper_windows serve the
   handle: its segments, offsets and edit distances are the target-role records of the pairs, by pair. Errors as for
   gw_mapper_window_overlaps. */
gw_mapper_windows* gw_mapper_correction_windows(const void* overlaps, int64_t n, const char* bases,
                                                const int64_t* offsets, int32_t n_reads, uint32_t first_read_id,
                                                int32_t window_length, int32_t max_depth, int64_t max_device_bytes,
                                                void* stream);
/* The segments pass alone over records that are taken for pairs as they stand: no pair selection, no layer selection,
   no gather. */
gw_mapper_windows* gw_mapper_pair_segments(const void* pairs, int64_t n, const char* bases, const int64_t* offsets,
                                           int32_t n_reads, uint32_t first_read_id, int32_t window_length,
                                           int64_t max_device_bytes, void* stream);
/* What a handle of the two calls above holds beyond the others. Returns the number of query-role records; *n_pairs is
   the number of pairs. segments (24 B each, written when capacity suffices), query_role_offsets[pairs + 1],
   pair_positions[pairs] (the pairs' positions in the input) and *query_role_ms (device time of the query-role records;
   stage_ms[2] of gw_mapper_windows_copy_segments is that of the target-role ones); any pointer may be NULL. A handle
   of gw_mapper_window_overlaps holds none of it: 0 records, 0 pairs. */
int64_t gw_mapper_windows_copy_query_role_segments(const gw_mapper_windows* windows, void* segments, int64_t capacity,
                                                   int64_t* query_role_offsets, int64_t* pair_positions, int64_t* n_pairs,
                                                   float* query_role_ms);

/* ---- base-quality weights for polishing and read correction ---------------------------------------------------------
   The rules (Q1 to Q4) are in INTEGRATION.md section 3l. The qualities of a read set are Phred+33 bytes that share the
   offsets of its bases; every byte must lie in 33..126, which is checked on the host before anything is uploaded, and
   the weight of byte c is c - 33. A set's qualities are uploaded once, next to its reads, and stay on the device:
   what reaches the host beyond the unweighted calls is 4 B per segment record (its quality sum) and one weight byte
   per window base. */

/* gw_mapper_window_overlaps with qualities. Either quality pointer may be NULL: that set has none. Where the queries
   have qualities, the quality sum of every record is computed on the device (gwm_segment_quality_sums) and a record
   is a layer only if it also passes Q2 with min_mean_quality (>= 0; racon's -q); where they have none, the layers are
   those of gw_mapper_window_overlaps. The weights of every window sequence are gathered on the device by the plan of
   its bases (gwm_gather_weights): c - 33 from a set with qualities, reversed and not complemented on '-' layers, 1
   throughout from a set without. Without target bases the targets are the queries, with the queries' qualities.
   Errors as for gw_mapper_window_overlaps, plus a quality byte outside 33..126 and a negative min_mean_quality, both
   before any device work. */
gw_mapper_windows* gw_mapper_window_overlaps_weighted(const void* overlaps, int64_t n, const char* query_bases,
                                                      const int64_t* query_offsets, int32_t n_queries,
                                                      uint32_t first_query_read_id, const char* target_bases,
                                                      const int64_t* target_offsets, int32_t n_targets,
                                                      uint32_t first_target_read_id, const char* query_qualities,
                                                      const char* target_qualities, int32_t min_mean_quality,
                                                      int32_t window_length, int32_t max_depth,
                                                      int64_t max_device_bytes, void* stream);
/* gw_mapper_correction_windows with the qualities of the one read set (NULL: unit weights and the layers of
   gw_mapper_correction_windows). The records of both roles get quality sums: a target-role record's layer is supplied
   by the pair's query read, a query-role record's by its target read. */
gw_mapper_windows* gw_mapper_correction_windows_weighted(const void* overlaps, int64_t n, const char* bases,
                                                         const int64_t* offsets, int32_t n_reads,
                                                         uint32_t first_read_id, const char* qualities,
                                                         int32_t min_mean_quality, int32_t window_length,
                                                         int32_t max_depth, int64_t max_device_bytes, void* stream);
/* What a handle of the two calls above holds beyond the others: weights (one per base of
   gw_mapper_windows_copy_windows, in the same order), quality_sums (one per record of gw_mapper_windows_copy_segments;
   none when the supplying set had no qualities), query_role_quality_sums (one per record of
   gw_mapper_windows_copy_query_role_segments, likewise) and ms[2]: device time of the quality sums and of the weight
   gather. Any pointer may be NULL. A handle of the unweighted calls holds none of it. */
int gw_mapper_windows_copy_weights(const gw_mapper_windows* windows, int8_t* weights, uint32_t* quality_sums,
                                   uint32_t* query_role_quality_sums, float* ms);

/* gw_mapper_select_layers with Q2: quality_sums[n_segments] (NULL: exactly gw_mapper_select_layers) and
   min_mean_quality (negative: an error). It needs no device. */
int64_t gw_mapper_select_layers_weighted(const void* segments, int64_t n_segments, const void* overlaps,
                                         int64_t n_overlaps, int32_t n_queries, uint32_t first_query_read_id,
                                         const int64_t* target_lengths, int32_t n_targets,
                                         uint32_t first_target_read_id, int32_t window_length, int32_t max_depth,
                                         const uint32_t* quality_sums, int32_t min_mean_quality, uint32_t* plan,
                                         int64_t plan_capacity, int64_t* n_windows, uint32_t* window_table,
                                         int64_t window_capacity);
/* gw_mapper_select_correction_layers with Q2: the sums of the records of either role, either may be NULL */
int64_t gw_mapper_select_correction_layers_weighted(const void* target_role, int64_t n_target_role,
                                                    const void* query_role, int64_t n_query_role, const void* pairs,
                                                    int64_t n_pairs, const int64_t* read_lengths, int32_t n_reads,
                                                    uint32_t first_read_id, int32_t window_length, int32_t max_depth,
                                                    const uint32_t* target_role_quality_sums,
                                                    const uint32_t* query_role_quality_sums, int32_t min_mean_quality,
                                                    uint32_t* plan, int64_t plan_capacity, int64_t* n_windows,
                                                    uint32_t* window_table, int64_t window_capacity);
/* Q1 alone, over host arrays: the records (24 B each) and the overlaps they index, the supplying set's qualities and
   offsets, are uploaded, gwm_segment_quality_sums runs, and sums[n_segments] is copied back. query_role 0: the
   supplier of a record is its overlap's query read; otherwise its target read. sums_ms (device time) may be NULL. */
int gw_mapper_segment_quality_sums(const void* segments, int64_t n_segments, const void* overlaps, int64_t n_overlaps,
                                   int32_t query_role, const char* qualities, const int64_t* offsets, int32_t n_reads,
                                   uint32_t first_read_id, uint32_t* sums, void* stream, float* sums_ms);

/* ---- pileups: per-base counts of aligned overlaps --------------------------------------------------------------------
   Six uint32 counters per base of the read that owns the position -- channels 0..5 = A, C, G, T, deletion, insertion --,
   added up on the device from the alignment states (gwm_overlap_pileup and gwm_pair_pileup of gwhip_mapper.h; the rules
   are in INTEGRATION.md section 3m). Neither the states nor any CIGAR text reach the host: the counters do, once. */

/* The pileup of the target set under n host overlaps over host reads (target_bases NULL: the target set is the query
   set). The reads are uploaded once, the overlaps are aligned as gw_mapper_align_overlaps aligns them and counted on
   the device as they stand: no overlap is selected here. The handle keeps the counters on the device until they are
   copied. Without overlaps every counter is 0. Errors as for gw_mapper_align_overlaps (NULL). */
typedef struct gw_mapper_pileup gw_mapper_pileup;
gw_mapper_pileup* gw_mapper_overlap_pileup(const void* overlaps, int64_t n, const char* query_bases,
                                           const int64_t* query_offsets, int32_t n_queries,
                                           uint32_t first_query_read_id, const char* target_bases,
                                           const int64_t* target_offsets, int32_t n_targets,
                                           uint32_t first_target_read_id, int64_t max_device_bytes, void* stream);
/* The pileup of one read set under records that are taken for pairs as they stand (no pair selection): every pair is
   aligned once and counted for both of its reads, the target read in the target role and the query read in the query
   role, into the one array. */
gw_mapper_pileup* gw_mapper_pair_pileup(const void* pairs, int64_t n, const char* bases, const int64_t* offsets,
                                        int32_t n_reads, uint32_t first_read_id, int64_t max_device_bytes,
                                        void* stream);
/* bases of the owner set: offsets[n_reads] */
int64_t gw_mapper_pileup_bases(const gw_mapper_pileup* pileup);
/* counts[6 * bases], channel-major planes: counts[c * bases + offsets[read] + p] is channel c of position p of read
   `read` (position in its set) -- one copy from the device --, and stage_ms[3]: device time of gather, align and
   pileup. Either pointer may be NULL. */
int gw_mapper_pileup_copy(const gw_mapper_pileup* pileup, uint32_t* counts, float* stage_ms);
void gw_mapper_pileup_destroy(gw_mapper_pileup* pileup);

/* ---- variant calling: SNVs, deletions and insertion alleles of the target set ---------------------------------------
   gwm_overlap_variants of gwhip_mapper.h over host arrays; the rules are in INTEGRATION.md section 3n. One alignment
   pass leaves the pileup of the target set and the variants called from it on the device; the records (gwm_variant,
   32 B each) reach the host, and the counters if they are asked for. */

/* The variants of the target set under n host overlaps over host reads (target_bases NULL: the target set is the query
   set), aligned and counted as gw_mapper_overlap_pileup does it and called with min_count >= 1 and 0 <= min_percent
   <= 100, which are refused out of range before anything reaches the device. Without overlaps there are no records
   and every counter is 0. Errors as for gw_mapper_overlap_pileup (NULL). */
typedef struct gw_mapper_variants gw_mapper_variants;
gw_mapper_variants* gw_mapper_overlap_variants(const void* overlaps, int64_t n, const char* query_bases,
                                               const int64_t* query_offsets, int32_t n_queries,
                                               uint32_t first_query_read_id, const char* target_bases,
                                               const int64_t* target_offsets, int32_t n_targets,
                                               uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                                               int64_t max_device_bytes, void* stream);
/* The same over the alignments of gw_mapper_align_overlaps_scored; scoring as there, NULL is gw_mapper_overlap_variants. */
gw_mapper_variants* gw_mapper_overlap_variants_scored(const void* overlaps, int64_t n, const char* query_bases,
                                                      const int64_t* query_offsets, int32_t n_queries,
                                                      uint32_t first_query_read_id, const char* target_bases,
                                                      const int64_t* target_offsets, int32_t n_targets,
                                                      uint32_t first_target_read_id, int32_t min_count,
                                                      int32_t min_percent, const int32_t* scoring,
                                                      int64_t max_device_bytes, void* stream);
/* The same over the alignments of gw_mapper_align_overlaps_scored2; scoring as there. */
gw_mapper_variants* gw_mapper_overlap_variants_scored2(const void* overlaps, int64_t n, const char* query_bases,
                                                       const int64_t* query_offsets, int32_t n_queries,
                                                       uint32_t first_query_read_id, const char* target_bases,
                                                       const int64_t* target_offsets, int32_t n_targets,
                                                       uint32_t first_target_read_id, int32_t min_count,
                                                       int32_t min_percent, const int32_t* scoring,
                                                       int64_t max_device_bytes, void* stream);
/* the number of called records */
int64_t gw_mapper_variants_count(const gw_mapper_variants* variants);
/* records[count] (gwm_variant), ascending by cell, within a cell SNV, deletion, insertion -- one copy from the
   device --, and stage_ms[4]: device time of gather, align, pileup + insertion runs, vote + call. Either pointer may
   be NULL. */
int gw_mapper_variants_copy(const gw_mapper_variants* variants, void* records, float* stage_ms);
/* counts[6 * bases of the target set], as gw_mapper_pileup_copy gives them for the same input */
int gw_mapper_variants_pileup_copy(const gw_mapper_variants* variants, uint32_t* counts);
void gw_mapper_variants_destroy(gw_mapper_variants* variants);

/* group_reads_into_indices: consecutive reads while the running base count stays <= max_basepairs_per_index; a longer
   read gets an index of its own. The reference's loop as it stands: when the very first read is longer than the limit
   a descriptor of zero reads comes first, and no reads at all give the one descriptor {0, 0}. Returns the number of
   descriptors (at most n_reads + 1) and writes min(capacity, count) pairs (first_read, number_of_reads) to `out`,
   which may be NULL. */
int64_t gw_mapper_group_reads_into_indices(const int64_t* read_lengths, int64_t n_reads, int64_t max_basepairs_per_index,
                                           uint32_t* out, int64_t capacity);

/* The walk of the reference's cudamapper for one device: queries and targets grouped into indices (target_bases NULL:
   all against all over the query set; queries are grouped by max_basepairs_per_query_index, targets by
   max_basepairs_per_target_index), index pairs in (query index, target index) order, descriptors of zero reads and,
   all against all, pairs with target.first_read < query.first_read skipped; per pair index -> match -> overlaps ->
   post-process (if post_process) -> end rescue with extension 50 and similarity 0.5 (if rescue_overlap_ends), the
   overlaps staying on the device in between, then appended to the result. Read ids are positions in the query /
   target set (the id shift behind reads shorter than k + w - 1 applies within an index, as in gwm_index_build).
   One device. This is gw_mapper_map_batched_cached with one index per batch on every level. */
typedef struct gw_mapper_overlaps gw_mapper_overlaps;
gw_mapper_overlaps* gw_mapper_map_batched(const char* query_bases, const int64_t* query_offsets, int32_t n_queries,
                                          const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                                          int32_t kmer_size, int32_t window_size, double filtering_parameter,
                                          int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                          float min_overlap_fraction, int64_t max_basepairs_per_query_index,
                                          int64_t max_basepairs_per_target_index, int32_t post_process,
                                          int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, void* stream);
/* gw_mapper_map_batched with one more stage per index pair when align_overlaps is set: what is left of the pair after
   post-processing and end rescue is aligned where it lies (gwm_align_overlaps of gwhip_mapper.h: the default aligner,
   max_query_length = the longest query slice of the pair; max_device_bytes as there, 0 = choose), overlaps, reads and
   alignment states staying on the device; only the CIGAR text comes back. One CIGAR per returned overlap, in the same
   order. The read sets are uploaded once when end rescue or alignment asks for them. With align_overlaps set, a read
   shorter than kmer_size + window_size - 1 in either set is an error before any device work: the index skips such a
   read and numbers the reads behind it by rank, so read ids would no longer name input reads and the wrong sequences
   would be aligned. With align_overlaps 0 this is gw_mapper_map_batched. */
gw_mapper_overlaps* gw_mapper_map_batched_aligned(
    const char* query_bases, const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
    const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size, int32_t window_size, double filtering_parameter,
    int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
    int64_t max_basepairs_per_query_index, int64_t max_basepairs_per_target_index, int32_t post_process,
    int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, int32_t align_overlaps, int64_t max_device_bytes,
    void* stream);

/* ---- the index cache ----------------------------------------------------------------------------------------------
   generate_batches_of_indices of the reference's index batcher over read lengths: reads are grouped into indices
   (gw_mapper_group_reads_into_indices), indices into host batches of query_indices_in_host_memory x
   target_indices_in_host_memory (query blocks outside, target blocks inside), every host batch the same way into device
   batches of query_indices_in_device_memory x target_indices_in_device_memory. target_read_lengths NULL means the
   target set is the query set: only the upper triangle of blocks is formed (targets start at the query block's own
   position), and a host batch is split symmetrically only when its query and target lists are equal. Errors
   (GW_MAPPER_ERROR, nothing written): the same set with different host counts, device counts or index sizes; any count
   below 1; fewer indices in host memory than in device memory.
   Returns the number of uint32 words of the flat result and writes it when `out` is not NULL and capacity suffices:
   n_host_batches, then per host batch a batch record, n_device_batches and that many batch records; a batch record is
   n_query_indices, n_target_indices, then (first_read, number_of_reads) of every query index and of every target
   index. */
int64_t gw_mapper_generate_batches_of_indices(const int64_t* query_read_lengths, int64_t n_queries,
                                              const int64_t* target_read_lengths, int64_t n_targets,
                                              int64_t query_basepairs_per_index, int64_t target_basepairs_per_index,
                                              int32_t query_indices_in_host_memory,
                                              int32_t query_indices_in_device_memory,
                                              int32_t target_indices_in_host_memory,
                                              int32_t target_indices_in_device_memory, uint32_t* out, int64_t capacity);

/* IndexHostCopy: a packed copy of an index in pinned host memory (gwm_index_pack of gwhip_mapper.h: read ids,
   positions, one direction bit per element and the unique-representation tables). _create is synchronous on `stream`;
   _to_device (gwm_index_unpack, then a wait) returns an index equal to the packed one in all arrays and attributes.
   pack_ms / restore_ms (device time, HIP events) may be NULL. */
typedef struct gw_mapper_index_host_copy gw_mapper_index_host_copy;
gw_mapper_index_host_copy* gw_mapper_index_host_copy_create(const gw_mapper_index* index, void* stream, float* pack_ms);
int64_t gw_mapper_index_host_copy_bytes(const gw_mapper_index_host_copy* copy);
gw_mapper_index* gw_mapper_index_host_copy_to_device(const gw_mapper_index_host_copy* copy, void* stream,
                                                     float* restore_ms);
void gw_mapper_index_host_copy_destroy(gw_mapper_index_host_copy* copy);

/* gw_mapper_map_batched_aligned through the index cache (the reference's -Q -q -C -c). The index pairs are walked
   host batch by host batch (gw_mapper_generate_batches_of_indices; all against all with one index size is the same
   set). Per host batch: its indices are generated, those of the first device batch stay on the device and those a
   later device batch asks for get a packed host copy (none when there is one device batch); then the device batches
   are walked, and while one is mapped on `stream` the indices of the next are restored from their host copies on a
   second stream, with an event between the two. Within a device batch pairs go query-major, with the skips of
   gw_mapper_map_batched; per pair the stages are the same. Records and their order do not depend on the four counts
   beyond the order of the pairs; at 1, 1, 1, 1 that is the order of gw_mapper_map_batched_aligned.
   Reuse: before an index is built it is looked for (1) among the indices still on the device from the previous device
   batch, (2) among the host copies of the previous host batch -- of the same kind (query / target), or of either kind
   all against all. Only an index found in neither is built.
   Device footprint: the indices of two device batches, 2 x (query_indices_in_device_memory +
   target_indices_in_device_memory); while a host batch's indices are generated, what the previous device batch left
   and the new host batch asks for (the rest is freed first), the first device batch, and one index built only to be
   packed. At 1, 1, 1, 1 never more than the two indices of a pair. Host: the packed copies of one host batch, and
   those of the previous one until the current host batch ends. An allocation failure is an error; no pair is skipped.
   Errors as for gw_mapper_generate_batches_of_indices. */
gw_mapper_overlaps* gw_mapper_map_batched_cached(
    const char* query_bases, const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
    const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size, int32_t window_size, double filtering_parameter,
    int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
    int64_t max_basepairs_per_query_index, int64_t max_basepairs_per_target_index, int32_t post_process,
    int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, int32_t align_overlaps, int64_t max_device_bytes,
    int32_t query_indices_in_host_memory, int32_t query_indices_in_device_memory, int32_t target_indices_in_host_memory,
    int32_t target_indices_in_device_memory, void* stream);
/* gw_mapper_map_batched_cached with the chaining overlapper (gw_mapper_chain_overlaps) in the place of the triggered
   one in every index pair: max_gap, bandwidth, min_chain_score and max_chains are its parameters, and the k of the
   chains is kmer_size. Post-processing, end rescue, alignment and the index cache are those of gw_mapper_map_batched_cached;
   stage_ms[0] of the result is then the device time of the chaining. */
gw_mapper_overlaps* gw_mapper_map_batched_chained(
    const char* query_bases, const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
    const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size, int32_t window_size, double filtering_parameter,
    int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
    int64_t max_basepairs_per_query_index, int64_t max_basepairs_per_target_index, int32_t post_process,
    int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, int32_t align_overlaps, int64_t max_device_bytes,
    int32_t query_indices_in_host_memory, int32_t query_indices_in_device_memory, int32_t target_indices_in_host_memory,
    int32_t target_indices_in_device_memory, int32_t max_gap, int32_t bandwidth, int32_t min_chain_score,
    int32_t max_chains, void* stream);
/* indices built from bases, indices restored from a host copy, and pack_unpack_ms[2]: summed device time of packing
   and of restoring (HIP events); any pointer may be NULL */
int gw_mapper_overlaps_cache_counts(const gw_mapper_overlaps* result, int64_t* index_builds, int64_t* index_restores,
                                    float* pack_unpack_ms);
int64_t gw_mapper_overlaps_count(const gw_mapper_overlaps* result);
/* bytes of all CIGARs of an aligned result, back to back; GW_MAPPER_ERROR when it was mapped without alignment */
int64_t gw_mapper_overlaps_cigar_text_bytes(const gw_mapper_overlaps* result);
/* text (cigar_text_bytes bytes, no separators), offsets[count + 1], edit_distances[count] (-1: no alignment) and
   stage_ms[3] (summed device time of gather, align, CIGAR text); any pointer may be NULL */
int gw_mapper_overlaps_copy_cigars(const gw_mapper_overlaps* result, char* text, int64_t* offsets,
                                   int32_t* edit_distances, float* stage_ms);
/* copies min(capacity, count) overlaps; stage_ms[3] (summed device time of chain/fuse/filter, post-processing, end
   rescue) and index_pairs (pairs walked) may be NULL */
int gw_mapper_overlaps_copy(const gw_mapper_overlaps* result, void* overlaps, int64_t capacity, float* stage_ms,
                            int64_t* index_pairs);
void gw_mapper_overlaps_destroy(gw_mapper_overlaps* result);

#ifdef __cplusplus
}
#endif

#endif
