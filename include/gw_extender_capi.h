/*
 * gw_extender_capi.h -- flat C API over cudaextender::Extender (libcudaextender.so), for foreign-function bindings
 * (genomeworks_amd/cudaextender.py). Each function flattens one method of extender.hpp with the same argument meaning;
 * int returns are cudaextender::StatusType values (0 = success), or GW_EXTENDER_ERROR when an exception was caught, its
 * text then being in gw_extender_last_error().
 *
 * Seed pairs and segments use the memory layouts of SeedPair {query, target} (8 B) and ScoredSegmentPair
 * {query, target, length, score} (16 B).
 */
#ifndef GW_EXTENDER_CAPI_H
#define GW_EXTENDER_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GW_EXTENDER_ERROR (-1)

typedef struct gw_extender gw_extender;

/* last error (exception text) of the calling thread */
const char* gw_extender_last_error(void);

/* create_extender(score_matrix, score_matrix_dim, xdrop_threshold, no_entropy, stream, device_id,
   create_default_device_allocator(max_device_memory or 2 GiB if <= 0, stream), extension_type).
   NULL on an unsupported matrix size or extension type. */
gw_extender* gw_extender_create(const int32_t* score_matrix, int32_t score_matrix_dim, int32_t xdrop_threshold,
                                int32_t no_entropy, void* stream, int32_t device_id, int64_t max_device_memory,
                                int32_t extension_type);

/* Extender::extend_async, host-pointer overload. seed_pairs: num_seed_pairs SeedPair records. */
int gw_extender_extend_host(gw_extender* h, const int8_t* query, int32_t query_length, const int8_t* target,
                            int32_t target_length, int32_t score_threshold, const void* seed_pairs, int64_t num_seed_pairs);

/* Extender::extend_async, device-pointer overload. */
int gw_extender_extend_device(gw_extender* h, const int8_t* d_query, int32_t query_length, const int8_t* d_target,
                              int32_t target_length, int32_t score_threshold, const void* d_seed_pairs,
                              int32_t num_seed_pairs, void* d_scored_segment_pairs, int32_t* d_num_scored_segment_pairs);

/* Extender::sync */
int gw_extender_sync(gw_extender* h);

/* size of Extender::get_scored_segment_pairs(); -1 (error text set) when it would throw */
int64_t gw_extender_result_count(gw_extender* h);

/* copies Extender::get_scored_segment_pairs() into out (capacity records) */
int gw_extender_copy_results(gw_extender* h, void* out, int64_t capacity);

/* Extender::reset */
void gw_extender_reset(gw_extender* h);

void gw_extender_destroy(gw_extender* h);

/* ---- instrumentation and test hooks (not part of the reference API) ---- */

/* seeds per chunk (default: 4 Mi per GiB of device memory); each chunk is sorted and de-duplicated on its own */
int gw_extender_set_chunk_size(gw_extender* h, int32_t seeds_per_chunk);

/* times every chunk with HIP events and counts the columns the extension kernel examines (costs a wait per chunk) */
int gw_extender_set_instrumentation(gw_extender* h, int32_t enable);

/* of the last extend call with instrumentation on: device time of the extension kernel, of compaction + sort +
   de-duplication, and the columns examined */
int gw_extender_last_timing(gw_extender* h, double* kernel_ms, double* sort_unique_ms, int64_t* positions);

/* gwx_sort_unique (gwhip_extender.h) with its own scratch: device segments[0..n) filtered by keep[0..n), sorted and
   de-duplicated into d_out; *count is the host result count */
int gw_extender_sort_unique_hook(const void* d_segments, const uint8_t* d_keep, int32_t n, void* d_out, int32_t* count,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif
