/*
 * gw_mapper_capi.h -- flat C API of cudamapper (libcudamapper.so), for foreign-function bindings
 * (genomeworks_amd/cudamapper.py): index creation from host reads, the anchor matcher, the triggered overlapper and
 * one call for a whole mapping. Functions returning int give 0 on success; those returning a count give it, or
 * GW_MAPPER_ERROR; creators return NULL. On an error the exception text is in gw_mapper_last_error().
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

/* Whole mapping of one index pair: queries against targets, or all against all when target_bases is NULL
   (all_to_all then drops self-mappings). Writes min(capacity, count) overlaps and returns count. */
int64_t gw_mapper_map(const char* query_bases, const int64_t* query_offsets, int32_t n_queries,
                      const char* target_bases, const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size,
                      int32_t window_size, double filtering_parameter, int64_t min_residues, int64_t min_overlap_len,
                      int64_t min_bases_per_residue, float min_overlap_fraction, void* overlaps, int64_t capacity,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif
