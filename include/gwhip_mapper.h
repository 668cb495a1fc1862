/*
 * gwhip_mapper.h -- kernel-level C-ABI of the cudamapper engine (libcudamapper.so): (k,w)-minimizer sketch, index
 * (stable sort, unique representations, frequency filter), anchor matcher, the triggered overlapper (chain, fuse,
 * filter), the post-processing of its overlaps (fusion of neighbours, end rescue) and their alignment into CIGARs, all
 * on gfx950.
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
    /* NULL for an index that was built: its six arrays are six allocations. An index restored by gwm_index_unpack
     * lives in this one allocation and its array pointers point into it. gwm_index_free frees either kind. */
    void* device_slab;
} gwm_index;

/* Builds the index of n_reads host reads: bases[offsets[i] .. offsets[i+1]) is read first_read_id + i. Reads shorter
 * than k + w - 1 contribute nothing, and, as in the reference, the read ids of the reads after them move down (the
 * read id of a sketch element is first_read_id + its rank among the reads kept). 1 <= k <= 32, w >= 1.
 * filtering_parameter >= 1.0 turns the frequency filter off. Synchronous on `stream` when it returns. */
int gwm_index_build(const char* bases, const int64_t* offsets, int32_t n_reads, uint32_t first_read_id, int32_t k,
                    int32_t w, int32_t hash_representations, double filtering_parameter, void* stream, gwm_index* out);
void gwm_index_free(gwm_index* index);

/* A packed copy of an index in pinned host memory (hipHostMalloc), made so that bringing the index back costs as few
 * bytes over the host link as possible. The slab is: a 64 B header (n, n_unique, n_first_occurrence, first_read_id,
 * number_of_reads, number_of_basepairs_in_longest_read), read_ids[n], positions_in_reads[n], one direction bit per
 * element (bit i % 64 of 64-bit word i / 64, zero beyond n), unique_representations[n_unique] and
 * first_occurrence_of_representations[n_first_occurrence], each section starting at a multiple of 16 B. That is
 * 8 n + 8 ceil(n / 64) + 12 n_unique + O(1) bytes against 17 n + 12 n_unique for the six arrays: the 8 B
 * representation of every element is left out, because it is the unique representation of the section of
 * first_occurrence the element lies in, and is filled in on the device again. */
typedef struct gwm_index_host_copy
{
    void* slab;    /* pinned host memory, `bytes` long; NULL after gwm_index_host_copy_free */
    int64_t bytes;
    float pack_ms; /* device time of gwm_index_pack: bitmap kernel and the copies (HIP events) */
} gwm_index_host_copy;

/* Packs a device index into a new host copy; the index is not changed. A kernel turns the direction bytes into the
 * bitmap (one 64-bit ballot per wave64), then the arrays are copied to the slab with asynchronous copies on `stream`.
 * Synchronous on `stream` when it returns: the slab is complete. Packing never changes a value: a direction byte
 * other than 0 or 1 is an error (-1, no copy is left behind). The empty index packs into a header alone. */
int gwm_index_pack(const gwm_index* index, void* stream, gwm_index_host_copy* out);
/* Restores the index of a host copy into one device allocation: one asynchronous copy of the slab on `stream`, a
 * kernel that gives element i the representation of its section (upper-bound search of i in first_occurrence, so empty
 * sections are skipped; an element outside every section gets 0, as gwm_index_from_arrays leaves it) and a kernel that
 * turns the bitmap back into direction bytes. The result equals the packed index in all six arrays and all attributes
 * (stage_ms is zero: nothing was built); the empty index comes back with no arrays. Asynchronous: the work is queued
 * on `stream` when this returns, so the copy must outlive it and the index may be used on `stream`, or on another
 * stream behind an event recorded on `stream`. */
int gwm_index_unpack(const gwm_index_host_copy* copy, void* stream, gwm_index* out);
void gwm_index_host_copy_free(gwm_index_host_copy* copy);
int64_t gwm_index_host_copy_bytes(const gwm_index_host_copy* copy);

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

/* gwm_find_overlaps with the result left on the device: *out is a device array of *count records (NULL when there are
 * none) that the caller frees with gwm_device_free. */
int gwm_find_overlaps_device(const gwm_anchor* anchors, int64_t n, int32_t all_to_all, int64_t min_residues,
                             int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
                             void* stream, gwm_overlap** out, int64_t* count, float* chain_fuse_filter_ms);
void gwm_device_free(void* device_pointer);

/* The parameters of the chaining overlapper. The defaults the layers above fill in -- max_gap 5000, bandwidth 500,
 * min_chain_score 40, max_chains 4 -- are minimap2's conventions (its -g, -r and -m); they are not tuned here. */
typedef struct gwm_chaining
{
    int32_t kmer_size;       /* k, 1..32: what one anchor is worth */
    int32_t max_gap;         /* G >= 1 */
    int32_t bandwidth;       /* B >= 0 */
    int32_t min_chain_score; /* S >= 0 */
    int32_t max_chains;      /* M, 1..64: chains per read pair and orientation */
} gwm_chaining;

/* Chaining overlapper over sorted device anchors[0..n): a dynamic programme over the anchors of every read pair, in
 * both orientations, instead of the neighbour test of gwm_find_overlaps. All arithmetic is in integers and exact
 * (positions are uint32, their differences are taken as signed numbers that never wrap):
 *   C1  A group is a maximal run of anchors of one (query_read_id, target_read_id); its anchors are 0 .. m - 1 in
 *       sort order. With all_to_all a group of a read with itself yields nothing, and no group of fewer than
 *       min_residues anchors does (the filter would drop their records). m >= 2^24 is an error: scores are int32.
 *   C2  Every group is chained twice, for '+' and for '-', independently; an anchor may be in one chain of each.
 *       dq = q_i - q_j; dt = t_i - t_j for '+', t_j - t_i for '-'.
 *   C3  j may precede i iff i - 64 <= j < i, 0 < dq <= G, 0 < dt <= G and |dq - dt| <= B.
 *   C4  gain = min(dq, dt, k) - cost(|dq - dt|); cost(0) = 0, cost(d) = d * k / 100 + (floor(log2 d) >> 1), integer
 *       division.
 *   C5  best = max over the predecessors j of f(j) + gain(j, i). If best > k: f(i) = best and p(i) the largest such j.
 *       Otherwise f(i) = k and i has no predecessor (a tie with k starts a new chain).
 *   C6  Per group and orientation, rounds r = 0 .. M - 1: e = the unused anchor of largest f, the smallest index on
 *       ties; stop when there is none or f(e) < S. Walk e, p(e), p(p(e)), ... until an anchor has no predecessor or
 *       its predecessor is used; the anchors visited are the chain and become used. score = f(e) - f(u) when the
 *       walk stopped in front of a used anchor u, else f(e). The chain is a candidate iff score >= S; a round whose
 *       chain is not one still uses up its anchors and its round.
 *   C7  One record per candidate: query start / end = q of the chain's first / last anchor; target start / end = t of
 *       the first / last anchor for '+', of the last / first for '-'; relative_strand the orientation, num_residues
 *       the number of anchors, overlap_complete 1. Positions are minimizer starts, as in gwm_find_overlaps. Every
 *       candidate then passes the filter of gwm_find_overlaps, the same arithmetic. scores[i] is the score of kept
 *       record i.
 *   C8  Groups in anchor order; within a group the '+' rounds in round order, then the '-' rounds.
 * min(capacity, *count) records and scores are copied to the host arrays `out` and `scores` (either may be NULL);
 * *count is the number kept. chain_ms (device time, HIP events) may be NULL. Errors, on which nothing is written:
 * a parameter outside the ranges above, a negative min_residues, min_overlap_len or min_bases_per_residue,
 * n >= 2^32, a group of 2^24 anchors or more. */
int gwm_chain_overlaps(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                       int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                       float min_overlap_fraction, void* stream, gwm_overlap* out, int32_t* scores, int64_t capacity,
                       int64_t* count, float* chain_ms);

/* gwm_chain_overlaps with the result left on the device: *out and *scores (scores may be NULL) are device arrays of
 * *count elements, NULL when there are none, that the caller frees with gwm_device_free. */
int gwm_chain_overlaps_device(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                              int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                              float min_overlap_fraction, void* stream, gwm_overlap** out, int32_t** scores,
                              int64_t* count, float* chain_ms);

/* Overlapper::post_process_overlaps over device overlaps[0..n), in the order get_overlaps gave them. Two neighbours
 * fuse when they share strand ('+' or '-') and read pair and (a) both gaps are below 500, or (b) the float ratio of
 * the smaller gap to the larger exceeds the double 0.8, or (c) both gaps, as float fractions of the summed query /
 * target lengths, are below the double 0.2. A gap is abs() of the uint32 difference read as int32 (query: start of
 * the second minus end of the first; target likewise on '+', start of the first minus end of the second on '-'); a
 * difference of exactly 2^31 is undefined in the reference and stays -2^31 here. Every maximal run of fusing
 * neighbours gives one record, written after the originals in run order: query start and '+' target start from the
 * run's first member, query end and '+' target end from its last ('-': target start from the last, target end from
 * the first), num_residues the sum, every other field from the run's last member -- or from its second to last when
 * the run reaches the end of the array. With drop_fused_overlaps the originals that belong to a fusing pair are
 * removed, order kept. `out` is a device array with room for n + n / 2 records and must not alias `overlaps`;
 * *count is the number written. fuse_ms (device time, HIP events) may be NULL. */
int gwm_post_process_overlaps(const gwm_overlap* overlaps, int64_t n, int32_t drop_fused_overlaps, void* stream,
                              gwm_overlap* out, int64_t* count, float* fuse_ms);

/* Overlapper::rescue_overlap_ends over device overlaps[0..n), in place. The reads of the query set and of the target
 * set are device arrays in the layout gwm_index_build takes (bases, n + 1 offsets); read id r of an overlap is read
 * r - first_*_read_id of its set. Per overlap, three rounds of: head window = min(query start, target start,
 * extension) bases before the starts, tail window = min(extension, query length - query end, target length - target
 * end) bases after the ends; an end moves by its whole window when float(shared) / float(union) of the two windows'
 * 15-mers (stride 1, multisets; a window shorter than 15 bases, the empty one too, is a single k-mer) is >=
 * required_similarity. Bytes compare as bytes. A '-' overlap is handled in the coordinates of the reverse-complemented
 * target (A<->T, C<->G; every other byte stays as it is -- the reference leaves the other upper-case letters alone
 * and is undefined for the rest; the middle base of an odd-length target is not complemented, as the reference's
 * in-place swap of len / 2 pairs skips it) and moved back. 0 <= extension <= 78 (one k-mer per lane of a wave64); anything
 * else is an error. Where the reference is undefined or throws -- a read id outside its set, a start or end beyond
 * its read -- the call returns -1, says so in gwm_last_error() and leaves the overlaps as they were; the kernel never
 * reads outside the reads it was given. rescue_ms may be NULL. */
int gwm_rescue_overlap_ends(gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                            int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                            const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                            int32_t extension, float required_similarity, void* stream, float* rescue_ms);

/* The CIGARs of n overlaps. Device arrays, owned by the struct; free them with gwm_cigars_free. */
typedef struct gwm_cigars
{
    int64_t n;               /* overlaps */
    int64_t text_bytes;      /* cigar_offsets[n] */
    char* text;              /* device: CIGARs back to back, no separators, no NUL; NULL when text_bytes is 0 */
    int64_t* cigar_offsets;  /* device [n + 1] */
    int32_t* edit_distances; /* device [n]: columns that are not a match; -1 where the aligner gave no result */
    float stage_ms[3];       /* HIP events, summed over the chunks: gather, align, cigar text */
} gwm_cigars;

/* Global alignment of device overlaps[0..n), each over its own slices, with bases and alignment states staying on the
 * device. Read sets as for gwm_rescue_overlap_ends. Overlap i aligns Q[query read][query start, query end) against
 * T[target read][target start, target end) (forward target coordinates); on '-' against the reverse complement of that
 * target slice, taken with the aligner's table: "TGAC"[(c >> 1) & 3] for every byte, what cudaaligner's
 * add_alignment(..., reverse_complement_target = true) does -- not the complement of end rescue. The aligner is the
 * default one (gwhip_hirschberg_myers of gwhip.h, Hirschberg + Myers) with max_query_length = the longest query slice of
 * the call. CIGAR i is the text of Alignment::convert_to_cigar() in its basic format (match and mismatch both M and
 * merged, I a base of the target only, D one of the query only, as cudaaligner names them) at
 * text[cigar_offsets[i] .. cigar_offsets[i + 1]). Where the aligner reports no columns the CIGAR is empty and the edit
 * distance -1, or 0 when both slices are empty.
 *
 * Consecutive overlaps are aligned in chunks: as many as keep gwm_align_bytes_needed's sum for the chunk -- gathered
 * bases, state slots, the aligner's workspace, the text at its upper bound of two bytes per column, and the small per-
 * overlap arrays -- within max_device_bytes; 0 means half of the device memory that is free at the call. An overlap
 * that does not fit alone is an error. The result does not depend on the chunking. The overlap records (36 B each) are
 * copied to the host to size the chunks; bases and states are not.
 *
 * A read id outside its set, start > end, or an end beyond its read return -1 with gwm_last_error() set before anything
 * is aligned, and leave *out zeroed (as every error does); the kernels never read outside the reads they were given.
 * n == 0 launches nothing. Synchronous on `stream` when it returns. */
int gwm_align_overlaps(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                       int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                       const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                       int64_t max_device_bytes, void* stream, gwm_cigars* out);
void gwm_cigars_free(gwm_cigars* cigars);
/* Device bytes gwm_align_overlaps counts for a chunk that holds one overlap with slices of these lengths, in a call
 * whose longest query slice is max_query_length: the smallest max_device_bytes that overlap can be aligned with.
 * Host arithmetic only. */
int64_t gwm_align_bytes_needed(int32_t query_length, int32_t target_length, int32_t max_query_length);

/* Affine gap costs for the alignments of a call (include/gwhip_affine.h states the rules): costs are minimised, a match
 * costs 0, a gap run of L columns gap_open + L * gap_extend; 1 <= mismatch <= 255, 0 <= gap_open <= 255,
 * 1 <= gap_extend <= 255; band >= 0 diagonals on either side of the corners' diagonals. */
typedef struct gwm_scoring
{
    int32_t mismatch;
    int32_t gap_open;
    int32_t gap_extend;
    int32_t band;
} gwm_scoring;

/* gwm_align_overlaps with the aligner chosen by `scoring`: NULL is gwm_align_overlaps itself; otherwise the slices,
 * gathered as there, are aligned by gwhip_affine_align under these costs inside this band, and the CIGARs and
 * edit_distances (still the columns that are not a match) describe those alignments. An overlap whose band has more
 * than GWHIP_AFFINE_MAX_DIAGONALS diagonals (|m - n| + 2 band + 1) is the aligner's "no result": an empty CIGAR and -1.
 * The budget counts gwhip_affine_workspace_bytes in place of the default aligner's workspace
 * (gwm_align_bytes_needed_scored); the result does not depend on it. A scoring out of range is an error before anything
 * is launched. */
int gwm_align_overlaps_scored(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                              int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                              const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                              const gwm_scoring* scoring, int64_t max_device_bytes, void* stream, gwm_cigars* out);
/* gwm_align_bytes_needed for a call with a scoring of this band. Host arithmetic only. */
int64_t gwm_align_bytes_needed_scored(int32_t query_length, int32_t target_length, int32_t band);

/* Scores, band and X-drop of the affine X-drop extension (include/gwhip_affine.h, gwhip_extend; INTEGRATION.md section
 * 3q), in gwhip_extend_args' ranges. */
typedef struct gwm_extension
{
    int32_t match;
    int32_t mismatch;
    int32_t gap_open;
    int32_t gap_extend;
    int32_t band;
    int32_t xdrop;
} gwm_extension;

/* Moves the ends of device overlaps[0..n) in place over what the affine X-drop extension aligns beyond them. With reads of
 * Lq and Lt bases and M = max_extension (0 .. 2^19), in the target's strand coordinates (T' = T on '+'; on '-' its reverse
 * complement by the aligner's table, [ts', te') = [Lt - te, Lt - ts)): the tail extends Q[qe : qe + min(M, Lq - qe)]
 * against T'[te' : te' + min(M, Lt - te')], then qe += i*, te' += j*; the head extends the slices of the same caps in
 * front of qs and ts', both read back to front, then qs -= i*, ts' -= j*; on '-' ts', te' are mapped back. Every other
 * field of a record stays. The 2 n pairs go through gwhip_extend in score-only mode, chunk by chunk within
 * max_device_bytes (0: half of the free device memory; the result does not depend on it; an overlap that does not fit
 * alone is an error; a chunk of m overlaps counts its gathered bases + 90 m + 1360 bytes). extensions: device, [n][4] = head i*, head j*, tail i*, tail j*; scores: device, [n][2] = head, tail.
 * M == 0 changes nothing and gives zeros. A read id outside its set, start > end, an end beyond its read and a value out of
 * range return -1 with gwm_last_error() set before anything is written. Synchronous on `stream` when it returns. */
int gwm_extend_overlaps(gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                        int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                        const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                        const gwm_extension* extension, int32_t max_extension, int64_t max_device_bytes, void* stream,
                        int32_t* extensions, int32_t* scores);

/* Two-piece gap costs (include/gwhip_affine.h, gwhip_affine2_align): a gap run of L columns
 * costs min(gap_open + L * gap_extend, gap_open2 + L * gap_extend2); both pieces in gwm_scoring's ranges, in any order. */
typedef struct gwm_scoring2
{
    int32_t mismatch;
    int32_t gap_open;
    int32_t gap_extend;
    int32_t gap_open2;
    int32_t gap_extend2;
    int32_t band;
} gwm_scoring2;

/* gwm_align_overlaps_scored under two-piece costs: NULL is gwm_align_overlaps itself. The budget counts what
 * gwm_align_bytes_needed_scored states; an overlap whose band has more than GWHIP_AFFINE2_MAX_DIAGONALS diagonals is the
 * aligner's "no result": an empty CIGAR and -1. */
int gwm_align_overlaps_scored2(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                               int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                               const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                               const gwm_scoring2* scoring, int64_t max_device_bytes, void* stream, gwm_cigars* out);

/* The chains of gwm_chain_overlaps with their anchors: everything gwm_chain_overlaps does and returns, and for kept
 * record i the anchors of its chain in chain order (ascending anchor index), anchor_positions[anchor_offsets[i] ..
 * anchor_offsets[i + 1]) as (query_position_in_read, target_position_in_read) pairs; record i owns num_residues of
 * them. Records, scores and their order are those of gwm_chain_overlaps. min(capacity, *count) records, scores and
 * that many + 1 offsets are copied to the host arrays, and the anchors of those records as far as anchor_capacity pairs
 * reach (2 n always suffices: an anchor is in at most one chain of each orientation); *n_chain_anchors is the number of
 * pairs of all kept records. Any output array may be NULL. Membership is found on the device: the extraction marks
 * every anchor it visits with its record slot, a scan of the kept slots turns slots into record indices, and a stable
 * radix sort by record index brings the marked anchors into record order. */
int gwm_chain_overlaps_anchored(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                                int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                float min_overlap_fraction, void* stream, gwm_overlap* out, int32_t* scores, int64_t capacity,
                                int64_t* anchor_offsets, uint32_t* anchor_positions, int64_t anchor_capacity, int64_t* count,
                                int64_t* n_chain_anchors, float* chain_ms);

/* gwm_chain_overlaps_anchored with the result left on the device: *out, *scores (may be NULL), *anchor_offsets
 * (*count + 1 entries) and *anchor_positions (*n_chain_anchors pairs) are device arrays, NULL when *count is 0, that the
 * caller frees with gwm_device_free. */
int gwm_chain_overlaps_anchored_device(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                                       int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                       float min_overlap_fraction, void* stream, gwm_overlap** out, int32_t** scores,
                                       int64_t** anchor_offsets, uint32_t** anchor_positions, int64_t* count,
                                       int64_t* n_chain_anchors, float* chain_ms);

/* The anchors of the records of one gwm_align_overlaps_anchored call: record i has anchors positions[offsets[i] ..
 * offsets[i + 1]) as (query_position_in_read, target_position_in_read) pairs in forward read coordinates, minimizer
 * starts as gwm_anchor has them -- what gwm_chain_overlaps_anchored_device returns. */
typedef struct gwm_anchor_lists
{
    const int64_t* offsets;    /* device [n + 1] */
    const uint32_t* positions; /* device [n_anchors][2] */
    int64_t n_anchors;
    int32_t kmer_size; /* k, 1..32: the anchors' k-mers */
    int32_t spacing;   /* S >= 1; the layers above fill in 256, a convention that is not tuned */
} gwm_anchor_lists;

/* gwm_align_overlaps with every overlap cut at anchors of its chain and aligned piece by piece (INTEGRATION.md section
 * 3s). scoring_pieces 0: the default aligner, `scoring` is not read; 1 / 2: gwhip_affine_align / gwhip_affine2_align
 * under `scoring` (with one piece gap_open2 and gap_extend2 are not read). anchors NULL is the call without anchors.
 *   G1  n, m are the slice lengths. An anchor (q, t) lies at u = q - query_start and, on '+', v = t - target_start; on
 *       '-', v = target_end - t - k, the start of the k-mer in the reverse-complemented target slice that the gather
 *       produces. Signed 64-bit arithmetic; nothing wraps.
 *   G2  An anchor is valid iff 0 < u < n and 0 < v < m. The others are dropped silently: a chained record starts and
 *       ends on an anchor, so its first and last anchor normally are; after gwm_extend_overlaps has moved the ends
 *       they normally are not.
 *   G3  The valid anchors of a record must be strictly increasing in both u and v, in list order; otherwise the call
 *       returns -1 with an error that names the first such record, before any alignment is launched. The chains of
 *       gwm_chain_overlaps always are (C3).
 *   G4  A valid anchor is a cut iff it is the first valid anchor of its record, or floor(u / S) differs from that of
 *       the valid anchor before it.
 *   G5  With cuts c_1 .. c_p, c_0 = (0, 0) and c_(p+1) = (n, m), piece j is Q[u_j, u_(j+1)) against
 *       T'[v_j, v_(j+1)), a global alignment by the call's aligner; the band of the scoring applies to every piece, and
 *       the default aligner's max_query_length is the longest query side of a piece of the call. A record without
 *       valid anchors is one piece: the alignment of gwm_align_overlaps, byte for byte.
 *   G6  The states of a record are its pieces' states concatenated, so CIGARs and edit distances read as before. If
 *       a piece has no result the record has none (an empty CIGAR and -1). Every piece is what its aligner returns for
 *       that pair alone; the whole is a valid global alignment of the slices. It is not re-priced across cuts -- a gap
 *       run that a cut divides stays two runs in the pieces' costs -- and no global optimality is claimed for it.
 * Pieces are gathered piece-major from the resident reads, aligned in one aligner call per chunk, and a wave64 per
 * record stitches the pieces' states into the record's slot. The chunks still hold whole records; a chunk's budget
 * counts gwm_align_bytes_needed_anchored over its pieces. What the plan of the whole call keeps on the device besides
 * the chunks -- 28 B per piece and 8 B per record, and while it is built 56 B per anchor -- lies outside
 * max_device_bytes.
 * Refused before anything is launched: k or S out of range, offsets that do not start at 0, decrease, or do not end at
 * n_anchors; then what gwm_align_overlaps refuses, then G3. */
int gwm_align_overlaps_anchored(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                                int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                                const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                                const gwm_anchor_lists* anchors, int32_t scoring_pieces, const gwm_scoring2* scoring,
                                int64_t max_device_bytes, void* stream, gwm_cigars* out);

/* Device bytes gwm_align_overlaps_anchored counts for a chunk that holds one overlap of these pieces: piece_starts[0 ..
 * 2 pieces] are the exclusive sums of query and target length of piece 0, of piece 1, ... (host). scoring_pieces and
 * band as above; max_query_length, read with scoring_pieces 0 only, is the longest query side of a piece of the call.
 * Host arithmetic only. */
int64_t gwm_align_bytes_needed_anchored(const int64_t* piece_starts, int32_t pieces, int32_t scoring_pieces, int32_t band,
                                        int32_t max_query_length);

/* ---- polishing: from aligned overlaps to POA windows ----------------------------------------------------------------
 * The target reads are cut into windows of window_length bases: window k of a read is its bases [k W, (k + 1) W). */

/* What one overlap's alignment covers of one window of its target read (24 B). Over the aligned columns (match or
 * mismatch) of the overlap whose target base lies in the window: */
typedef struct gwm_segment
{
    uint32_t overlap;      /* position of the overlap in the call */
    uint32_t window;       /* target position / window_length */
    uint32_t target_first; /* smallest target position, forward target coordinates */
    uint32_t target_last;  /* largest target position */
    uint32_t query_begin;  /* smallest query position */
    uint32_t query_end;    /* largest query position + 1 */
} gwm_segment;

/* The segments of n overlaps. Device arrays, owned by the struct; free them with gwm_segments_free. */
typedef struct gwm_segments
{
    int64_t n;                /* overlaps */
    int64_t n_segments;       /* segment_offsets[n] */
    gwm_segment* segments;    /* device: ordered by overlap, then by ascending window; NULL when there are none */
    int64_t* segment_offsets; /* device [n + 1]: the records of overlap i are [segment_offsets[i], segment_offsets[i + 1]) */
    int32_t* edit_distances;  /* device [n], as in gwm_cigars */
    float stage_ms[3];        /* HIP events, summed over the chunks: gather, align, segments */
} gwm_segments;

/* gwm_align_overlaps with another consumer of the alignment states: the same arguments, slices, strand, aligner,
 * chunking (and its independence of max_device_bytes) and errors, plus window_length < 1 as an error; instead of CIGAR
 * text it leaves the segments of every overlap on the device. With the per-column states in forward column order
 * (0 match, 1 mismatch, 2 a target base only, 3 a query base only), a(j) / b(j) the number of columns before j whose
 * state is not 2 / not 3, an aligned column (state < 2) has query position query start + a(j), target position
 * target start + b(j) on '+' and target end - 1 - b(j) on '-', and window target position / window_length. Every window
 * that holds an aligned column of the overlap gives one record; a window of nothing but state 2 gives none, and
 * neither does an alignment without columns (no result, or two empty slices). One wave64 per alignment over tiles of 64
 * columns; a counting pass, a scan and a writing pass. The states are not copied anywhere. max_device_bytes bounds a
 * chunk's working set exactly as for gwm_align_overlaps (gwm_align_bytes_needed, whose two bytes per column stand for
 * the chunk's records here); the records themselves, 24 B each and kept for all chunks until the call returns, are the
 * result and lie outside that budget, as the CIGAR text of earlier chunks does there. */
int gwm_window_segments(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                        int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                        const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                        int32_t window_length, int64_t max_device_bytes, void* stream, gwm_segments* out);
void gwm_segments_free(gwm_segments* segments);

/* Read correction: the segments of both reads of every pair out of one alignment. There is one read set, and query and
 * target ids both name reads of it. Pair i is aligned exactly as gwm_align_overlaps(pairs, n, bases, ..., bases, ...)
 * aligns it, once. *target_role gets what gwm_window_segments gives for the same arguments, byte for byte, the edit
 * distances included. *query_role gets the records of the query read's windows: an aligned column with query position
 * q and target position t (both as above) lies in window q / window_length of the query read, and every such window
 * that holds an aligned column gives one record {overlap = i, window, target_first = min q, target_last = max q,
 * query_begin = min t, query_end = max t + 1} -- target_* describe the read that owns the window, query_* the read
 * that supplies the layer, in either role. A window of nothing but state 3 gives none. Records are ordered by pair,
 * then by ascending window; query_role->edit_distances is NULL (the edit distances are filled once, in *target_role).
 * stage_ms[0..1] are the same in both; stage_ms[2] is each role's own kernels and scan. Both roles are written by the
 * same chunk consumer, the states of a chunk are read on the device by both and copied nowhere; the query-role records
 * lie outside max_device_bytes like the others. Errors as for gwm_window_segments; both structs are left zeroed. */
int gwm_pair_segments(const gwm_overlap* pairs, int64_t n, const char* bases, const int64_t* offsets, int32_t n_reads,
                      uint32_t first_read_id, int32_t window_length, int64_t max_device_bytes, void* stream,
                      gwm_segments* target_role, gwm_segments* query_role);

/* ---- pileups: per-base counts of aligned overlaps ----------------------------------------
 * Six counters per base of the read that owns the position, channels 0..5 = A, C, G, T, deletion, insertion. */

/* The pileup of a read set of n_bases bases (offsets[n_reads]). Device array, owned by the struct; free it with
 * gwm_pileup_free. */
typedef struct gwm_pileup
{
    int64_t n_bases;   /* bases of the owner set */
    uint32_t* counts;  /* device [6 * n_bases], channel-major planes: counts[c * n_bases + offsets[read] + p] is channel c
                          of position p of read `read` (position in its set); NULL when n_bases is 0 */
    float stage_ms[3]; /* HIP events, summed over the chunks: gather, align, pileup */
} gwm_pileup;

/* gwm_window_segments with a third consumer of the alignment states: the same arguments without window_length, the
 * same slices, strand, aligner, chunking (and its independence of max_device_bytes) and errors; instead of records it
 * leaves the pileup of the target set on the device, zeroed by the call and then added to. With the states, a(j), b(j),
 * q and t of a column as for gwm_window_segments, A and B those counts over the whole alignment (the slice lengths of
 * an alignment that has a result), and the owner the target read, positions in forward target coordinates:
 *   state < 2: +1 at (t, channel of Q[q]), the complement channel on '-';
 *   state 2:   +1 at (t, deletion);
 *   a maximal run of state 3 that starts at column j with 1 <= b(j) <= B - 1: +1 at (p, insertion), p the smaller
 *   target position of its two neighbours, target start + b(j) - 1 on '+' and target end - 1 - b(j) on '-'. A run at
 *   either end of the alignment, which has no neighbour on one side, is not counted.
 * The channel of a base byte c is (0, 1, 3, 2)[(c >> 1) & 3], the aligner's folding read as A, C, G, T, and the
 * complement of channel k is 3 - k; a byte other than ACGT (and their lower-case forms) counts as the letter the
 * aligner folds it to, N as G. An alignment without columns (no result, or two empty slices) adds nothing; a record
 * given twice counts twice. For every position the channels 0..4 sum to the number of records with a result whose
 * target slice covers it.
 * One wave64 per alignment over tiles of 64 columns, one returnless atomic add per counted column or run; the
 * supplier's base is read from the resident read set. The states are not copied anywhere. max_device_bytes bounds a
 * chunk's working set exactly as for gwm_align_overlaps; the counters, 24 B per base of the target set, are the
 * result and lie outside that budget, as the segment records do. n == 0 launches no kernel and gives zeroed counters.
 * On an error the call returns -1, sets gwm_last_error() and leaves *out zeroed. */
int gwm_overlap_pileup(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                       int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                       const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                       int64_t max_device_bytes, void* stream, gwm_pileup* out);
void gwm_pileup_free(gwm_pileup* pileup);

/* Read correction's pileup: one read set, as for gwm_pair_segments, and one array of counters into which both roles of
 * every pair are added out of one alignment, by the same chunk consumer. The target role is that of gwm_overlap_pileup.
 * In the query role the owner is the query read and positions are query positions, ascending on both strands:
 *   state < 2: +1 at (q, channel of T[t]), the complement channel on '-';
 *   state 3:   +1 at (q, deletion);
 *   a maximal run of state 2 that starts at column j with 1 <= a(j) <= A - 1: +1 at (query start + a(j) - 1, insertion).
 * Memory and errors as for gwm_overlap_pileup. */
int gwm_pair_pileup(const gwm_overlap* pairs, int64_t n, const char* bases, const int64_t* offsets, int32_t n_reads,
                    uint32_t first_read_id, int64_t max_device_bytes, void* stream, gwm_pileup* out);

/* ---- variant calling: SNVs, deletions and insertion alleles of the target set -------------
 * A small-variant caller by counting: no genotypes, no likelihoods, no base qualities. */

/* One called variant (32 B). Channels are those of the pileup: A, C, G, T = 0..3. */
typedef struct gwm_variant
{
    uint32_t target_read; /* position of the target read in its set */
    uint32_t position;    /* p, forward target coordinates: the base an SNV replaces, the deleted base, the base an
                             insertion follows */
    uint32_t count;       /* SNV: n[alt]; deletion: n[deletion]; insertion: the run records of the called allele */
    uint32_t depth;       /* d(p) = n[A] + n[C] + n[G] + n[T] + n[deletion] */
    uint8_t kind;         /* 0 SNV, 1 deletion, 2 insertion */
    uint8_t ref;          /* r: the channel of the target's own byte at p */
    uint8_t alt;          /* SNV: the called channel; 0 otherwise */
    uint8_t length;       /* insertion: L, 1..32 bases; 0 otherwise */
    uint32_t reserved;    /* 0 */
    uint64_t key;         /* insertion: the allele, sum of code(allele[i]) << 2 (L - 1 - i); 0 otherwise */
} gwm_variant;

/* The called variants of a target set and its pileup. Device arrays, owned by the struct; free them with
 * gwm_variants_free. */
typedef struct gwm_variants
{
    int64_t n_variants;
    gwm_variant* variants; /* device: ascending by cell (offsets[read] + p), within a cell SNV, deletion, insertion; NULL
                              when there are none */
    gwm_pileup pileup;     /* what gwm_overlap_pileup gives for the same arguments, its stage_ms included */
    float stage_ms[4];     /* HIP events: gather, align, pileup + insertion runs (summed over the chunks), vote + call */
} gwm_variants;

/* gwm_overlap_pileup with a fourth consumer of the alignment states in the same chunk callback, and a calling stage
 * behind the chunks: the same arguments, slices, strand, aligner, chunking and errors, and every overlap is aligned
 * once. It leaves the pileup of the target set and the variants called from it on the device. With n[0..5] the
 * counters of base p of a target read as gwm_overlap_pileup defines them, r the channel of the target's own byte at p
 * and d = n[0] + ... + n[4], a count k passes at depth d when k >= min_count and 100 k >= min_percent d (64-bit
 * integers; min_count >= 1, 0 <= min_percent <= 100, anything else is an error before anything is launched):
 *   SNV: alt is the channel other than r with the greatest count, the smallest such channel on a tie; called when
 *   n[alt] passes at d.
 *   Deletion of base p: called when n[4] passes at d. One record per base; neighbours are not joined.
 *   Insertion after base p: every maximal run of state 3 that the pileup counts at cell p (it starts at column j with
 *   1 <= b(j) <= B - 1) and whose length L is 1..32 gives one run record (cell, L, key). Its allele is the run's query
 *   bases in forward target coordinates: Q[q .. q + L) on '+', their reverse complement on '-'; key = the sum of
 *   code(allele[i]) << 2 (L - 1 - i), codes A, C, G, T = 0..3 after the aligner's folding, so that among alleles of
 *   one length key order is alphabetical order. Runs of more than 32 bases stay counted in n[5] and give no record.
 *   Records are equal when (L, key) are; the best allele of a cell is the one with the most records, on a tie the
 *   shorter, then the one with the smaller key. The insertion is called when the record count of the best allele --
 *   not n[5] -- passes at d(p).
 * A cell yields at most one record of each kind. The records are a function of the multiset of alignments: they depend
 * neither on the order of the atomics, nor on the chunking, nor on the order of the overlaps.
 * Device: one wave64 per alignment finds the heads of the runs as the pileup kernel does; a head lane reads its run's
 * length from the up to 32 state bytes behind it and packs the query bytes itself, so a run that crosses a 64-column
 * tile is no special case. A counting pass, a scan, a writing pass; the run records are sorted by (cell, L, key) with
 * rocPRIM, run-length encoded and reduced per cell to the best allele. One thread per base flags SNV and deletion, one
 * per best allele applies the threshold; rocPRIM selects compact the three kinds and two merges give the order.
 * max_device_bytes bounds a chunk's working set exactly as for gwm_align_overlaps; the counters (24 B per base of the
 * target set), one flag byte per base, the run records (24 B each, kept for all chunks until the vote) and the variant
 * records lie outside that budget, as the segment records do. n == 0 launches no kernel and gives zeroed counters and
 * no records. On an error the call returns -1, sets gwm_last_error() and leaves *out zeroed. */
int gwm_overlap_variants(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                         int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                         const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                         int32_t min_count, int32_t min_percent, int64_t max_device_bytes, void* stream,
                         gwm_variants* out);
/* gwm_overlap_variants over the alignments of gwm_align_overlaps_scored: NULL is gwm_overlap_variants itself. */
int gwm_overlap_variants_scored(const gwm_overlap* overlaps, int64_t n, const char* query_bases,
                                const int64_t* query_offsets, int32_t n_queries, uint32_t first_query_read_id,
                                const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                                uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                                const gwm_scoring* scoring, int64_t max_device_bytes, void* stream, gwm_variants* out);
/* gwm_overlap_variants over the alignments of gwm_align_overlaps_scored2: NULL is gwm_overlap_variants itself. */
int gwm_overlap_variants_scored2(const gwm_overlap* overlaps, int64_t n, const char* query_bases,
                                 const int64_t* query_offsets, int32_t n_queries, uint32_t first_query_read_id,
                                 const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                                 uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                                 const gwm_scoring2* scoring, int64_t max_device_bytes, void* stream, gwm_variants* out);
void gwm_variants_free(gwm_variants* variants);

/* One sequence of a gather plan (20 B): bases [begin, end) of read `read` (position in its set) of the query set
 * (set 0) or the target set (set 1); reversed != 0: back to front, every byte through "TGAC"[(c >> 1) & 3]. */
typedef struct gwm_gather_entry
{
    uint32_t set;
    uint32_t read;
    uint32_t begin;
    uint32_t end;
    uint32_t reversed;
} gwm_gather_entry;

/* Writes the n sequences of a device plan into the device array out[0 .. out_bytes): sequence i at out_starts[i]
 * (device, caller-given), end - begin bytes. Read sets as for gwm_align_overlaps (device arrays). One block per
 * sequence. A set other than 0 / 1, a read outside its set, begin > end, an end beyond its read or a sequence that
 * does not lie within out return -1 before anything is written. gather_ms (device time) may be NULL. Synchronous on
 * `stream` when it returns. */
int gwm_gather_sequences(const gwm_gather_entry* plan, int64_t n, const int64_t* out_starts, const char* query_bases,
                         const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
                         const int64_t* target_offsets, int32_t n_targets, char* out, int64_t out_bytes, void* stream,
                         float* gather_ms);

/* ---- base qualities: the weights of polishing and read correction ------------------------
 * The qualities of a read set are Phred+33 bytes that share the offsets of its bases: byte j of read i is the quality
 * of base j. The weight of byte c is c - 33; the callers of this header refuse bytes outside 33..126 on the host, and
 * the kernels clamp a weight to 0..93. */

/* Q1: sums[j] = the sum of the weights of the supplier's quality bytes [query_begin, query_end) of record j, saturating
 * at 2^32 - 1 -- what the layer of the record would weigh. The supplier of a record is its overlap's query read
 * (query_role 0: the records of gwm_window_segments and the target role of gwm_pair_segments) or its target read
 * (query_role != 0: the query role of gwm_pair_segments). Device arrays throughout: the records and the overlaps they
 * index, the supplier set's qualities and offsets (read ids first_read_id .. first_read_id + n_reads - 1), and
 * sums[n_segments]. One wave64 per record, whose lanes stride the bytes; a record may be of any length. A record that
 * names an overlap or a read that does not exist, or a range beyond its read, returns -1 before anything is written.
 * The sums depend on the records alone, not on how the alignment was chunked. sums_ms (device time of the sums
 * kernel) may be NULL. Synchronous on `stream` when it returns. */
int gwm_segment_quality_sums(const gwm_segment* segments, int64_t n_segments, const gwm_overlap* overlaps,
                             int64_t n_overlaps, int32_t query_role, const char* qualities, const int64_t* offsets,
                             int32_t n_reads, uint32_t first_read_id, uint32_t* sums, void* stream, float* sums_ms);

/* Q3: gwm_gather_sequences with qualities in place of bases: the weights of the n sequences of a device plan into the
 * device array out[0 .. out_bytes), those of sequence i at out_starts[i], so that weight j of a sequence belongs to
 * base j of what gwm_gather_sequences writes for the same plan. reversed != 0: back to front, nothing is complemented.
 * Either quality pointer may be NULL: the entries of that set get weight 1 throughout; its offsets are needed all the
 * same. Errors and timing as for gwm_gather_sequences. */
int gwm_gather_weights(const gwm_gather_entry* plan, int64_t n, const int64_t* out_starts, const char* query_qualities,
                       const int64_t* query_offsets, int32_t n_queries, const char* target_qualities,
                       const int64_t* target_offsets, int32_t n_targets, int8_t* out, int64_t out_bytes, void* stream,
                       float* gather_ms);

const char* gwm_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
