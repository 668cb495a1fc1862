/*
 * gwhip_mapper.h -- kernel-level C-ABI of the cudamapper engine (libcudamapper.so): (k,w)-minimizer sketch, index
 * (stable sort, unique representations, frequency filter), anchor matcher and the triggered overlapper (chain, fuse,
 * filter), all on gfx950.
 *
 * The object-level API on top of it is gw_mapper_capi.h (flat C) and genomeworks_amd.cudamapper (Python). This header
 * is kept apart from gwhip.h on purpose: the POA / aligner kernel set and its source digest are not affected.
 *
 * Every array a stage returns is a device allocation owned by the returned struct; free it with the matching
 * gwm_*_free. Functions return 0, or -1 with gwm_last_error() set. Zero-sized stages launch nothing.
 */
#ifndef GWHIP_MAPPER_H
#define GWHIP_MAPPER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == cudamapper::Anchor (16 B) */
typedef struct gwm_anchor
{
    uint32_t query_read_id;
    uint32_t target_read_id;
    uint32_t query_position_in_read;
    uint32_t target_position_in_read;
} gwm_anchor;

/* == cudamapper::Overlap (36 B, same field order and padding) */
typedef struct gwm_overlap
{
    uint32_t query_read_id;
    uint32_t target_read_id;
    uint32_t query_start_position_in_read;
    uint32_t target_start_position_in_read;
    uint32_t query_end_position_in_read;
    uint32_t target_end_position_in_read;
    uint8_t relative_strand; /* '+' or '-' */
    uint32_t num_residues;
    uint8_t overlap_complete;
} gwm_overlap;

/* One index over reads [first_read_id, first_read_id + number_of_reads). Device arrays:
 *   representations, read_ids, positions_in_reads, directions (0 forward, 1 reverse): n elements, sorted by
 *   representation, ties in (read id, position) order; unique_representations: n_unique;
 *   first_occurrence_of_representations: n_unique + 1 (trailing total), or 0 entries when the index is empty. */
typedef struct gwm_index
{
    int64_t n;
    int64_t n_unique;
    uint64_t* representations;
    uint32_t* read_ids;
    uint32_t* positions_in_reads;
    uint8_t* directions;
    uint64_t* unique_representations;
    uint32_t* first_occurrence_of_representations;
    int64_t n_first_occurrence;
    uint32_t first_read_id;
    uint32_t number_of_reads;
    uint32_t number_of_basepairs_in_longest_read;
    /* device time (ms, HIP events) of the stages: sketch, sort, unique, filter */
    float stage_ms[4];
} gwm_index;

/* Builds the index of n_reads host reads: bases[offsets[i] .. offsets[i+1]) is read first_read_id + i. Reads shorter
 * than k + w - 1 contribute nothing, and, as in the reference, the read ids of the reads after them move down (the
 * read id of a sketch element is first_read_id + its rank among the reads kept). 1 <= k <= 32, w >= 1.
 * filtering_parameter >= 1.0 turns the frequency filter off. Synchronous on `stream` when it returns. */
int gwm_index_build(const char* bases, const int64_t* offsets, int32_t n_reads, uint32_t first_read_id, int32_t k,
                    int32_t w, int32_t hash_representations, double filtering_parameter, void* stream, gwm_index* out);
void gwm_index_free(gwm_index* index);

/* All anchors of query x target, sorted by (query read, target read, query position, target position). */
typedef struct gwm_anchors
{
    int64_t n;
    gwm_anchor* anchors; /* device */
    /* device time (ms): lookup + count + scan + generate, anchor sort */
    float stage_ms[2];
} gwm_anchors;

/* Uploads an index given as host arrays (test hook: the matcher on hand-built indices). n elements with their read ids
 * and positions, n_unique representations ascending with n_unique + 1 first occurrences; element representations are
 * filled in from the sections, directions are forward. */
int gwm_index_from_arrays(int64_t n, const uint32_t* read_ids, const uint32_t* positions_in_reads, int64_t n_unique,
                          const uint64_t* unique_representations, const uint32_t* first_occurrence,
                          uint32_t first_read_id, uint32_t number_of_reads, uint32_t number_of_basepairs_in_longest_read,
                          gwm_index* out);

int gwm_match(const gwm_index* query, const gwm_index* target, void* stream, gwm_anchors* out);
void gwm_anchors_free(gwm_anchors* anchors);

/* Triggered overlapper over sorted device anchors[0..n): chains (adjacent anchors of one read pair with
 * q(cur) - q(prev) < 150 unsigned and |t(cur) - t(prev)| < 150), chains of >= 3 anchors, fusion of adjacent kept
 * chains (same read pair, ||dq| - |dt|| < 300 between their first anchors), then the reference's overlap filter.
 * The kept overlaps are copied to the host array `out`, which needs room for n / 3 + 1 records (a kept chain holds at
 * least 3 anchors); *count is their number. Negative min_residues, min_overlap_len or min_bases_per_residue are an
 * error. */
int gwm_find_overlaps(const gwm_anchor* anchors, int64_t n, int32_t all_to_all, int64_t min_residues, int64_t min_overlap_len,
                int64_t min_bases_per_residue, float min_overlap_fraction, void* stream, gwm_overlap* out,
                int64_t* count, float* chain_fuse_filter_ms);

const char* gwm_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
