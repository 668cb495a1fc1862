/*
 * gwhip_extender.h -- kernel-level C-ABI of the cudaextender engine (libcudaextender.so): ungapped X-drop extension
 * of seed pairs on gfx950, then compaction, sort and adjacent de-duplication of the segments on the device.
 *
 * The object-level API on top of it is claraparabricks/genomeworks/cudaextender/extender.hpp (C++) and
 * gw_extender_capi.h (flat C). This header is kept apart from gwhip.h on purpose: the POA / aligner kernel set and
 * its source digest are not affected by the extender.
 *
 * Encoding: A=0 C=1 G=2 T=3, lower-case acgt=4, N/n=5, other=6, '&'=7; the score of a column (t, q) is
 * score_matrix[8 * t + q]. Symbols outside 0..7 are the caller's error (they index the matrix).
 */
#ifndef GWHIP_EXTENDER_H
#define GWHIP_EXTENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == cudaextender::SeedPair (8 B) */
typedef struct gwx_seed
{
    uint32_t query;
    uint32_t target;
} gwx_seed;

/* == cudaextender::ScoredSegmentPair (16 B) */
typedef struct gwx_segment
{
    uint32_t query;
    uint32_t target;
    int32_t length;
    int32_t score;
} gwx_segment;

typedef struct gwx_problem
{
    const int8_t* target; /* device */
    int32_t target_length;
    const int8_t* query; /* device */
    int32_t query_length;
    const int32_t* score_matrix; /* device, 64 entries */
    int32_t xdrop_threshold;
    int32_t score_threshold;
    int32_t no_entropy;
} gwx_problem;

/* Device scratch (bytes) that gwx_extend_chunk needs for up to `max_seeds` seeds. */
size_t gwx_workspace_bytes(int32_t max_seeds);

/* Extends seeds[0..n) (n <= the max_seeds the workspace was sized for) and writes the chunk's sorted, de-duplicated
 * segments to out[0..*count). Enqueued on `stream`; *count (host) is known on return, which waits for the stream
 * once, after compaction, and once more at the end. Returns 0, or -1 with gwx_last_error() set. Optional timing: if
 * `events` is non-null, events[0..2] (hipEvent_t) are recorded before the extension kernel, after it, and after the
 * last sort/unique step. */
int gwx_extend_chunk(const gwx_problem* problem, const gwx_seed* seeds, int32_t n, gwx_segment* out, int32_t* count,
                     void* workspace, size_t workspace_bytes, void* stream, void* const* events);

/* Writes `value` to the device int32 at d_dst, ordered on `stream` (no host wait). */
int gwx_store_count(int32_t* d_dst, int32_t value, void* stream);

/* Test hook: the compact/sort/unique step alone. segments[0..n) and keep[0..n) (device; keep[i] != 0 selects
 * segment i, in input order) -> out[0..*count) (device), the same step gwx_extend_chunk runs after its kernel. */
int gwx_sort_unique(const gwx_segment* segments, const uint8_t* keep, int32_t n, gwx_segment* out, int32_t* count,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Number of columns the last gwx_extend_chunk examined (both directions, entropy pass excluded), when built with
 * position counting enabled via gwx_count_positions(1); 0 otherwise. For throughput reports only. */
int gwx_count_positions(int32_t enable);
int64_t gwx_last_positions(void);

/* last error of the calling thread */
const char* gwx_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
