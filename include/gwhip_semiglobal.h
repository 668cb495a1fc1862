/*
 * gwhip_semiglobal.h -- kernel-level C-ABI of the infix / prefix alignment types of cudaaligner (libgwsemiglobal.so):
 * a score-only Myers scan that finds where a query ends (and, for infix, begins) in its target, and the gather of the
 * target slices into the layout gwhip_hirschberg_myers (gwhip.h) takes.
 *
 * The object-level API on top of it is cudaaligner::create_aligner(..., infix_alignment | prefix_alignment, ...) (C++),
 * gw_aligner_create_typed (gw_capi.h) and CudaAlignerBatch(alignment_type=...) (Python). This header is kept apart from
 * gwhip.h on purpose: the POA / aligner kernel set and its source digest are not affected by it.
 *
 * Semantics. Query Q of n bases, target T of m bases, unit costs, D[i][0] = i, D[0][j] = j (prefix) or 0 (infix). A
 * query base q matches a target base t when q == "ACTG"[(t >> 1) & 3] -- the predicate of the default global aligner.
 *   d  = min_j D[n][j]
 *   te = the smallest j with D[n][j] == d (column 0 counts)
 *   tb = 0 (prefix); the largest b <= te with global_distance(Q, T[b:te]) == d (infix)
 */
#ifndef GWHIP_SEMIGLOBAL_H
#define GWHIP_SEMIGLOBAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum
{
    GWHIP_SEMIGLOBAL_INFIX  = 0,
    GWHIP_SEMIGLOBAL_PREFIX = 1
};

/* queries of up to this many bases keep their column in registers; longer ones keep it in the workspace */
#define GWHIP_SEMIGLOBAL_REGISTER_QUERY 16384

typedef struct gwhip_semiglobal_args
{
    int32_t n_pairs;
    int32_t mode;                   /* GWHIP_SEMIGLOBAL_INFIX / _PREFIX */
    const char* sequences;          /* device, concatenated: q0 t0 q1 t1 ... */
    const int64_t* sequence_starts; /* device, [2n + 1] */
    int32_t max_query_length;       /* >= every query of the batch: selects the kernel variant and sizes the workspace */
    int32_t* ends;                  /* device, [3n]: d, tb, te of pair i at ends[3i .. 3i + 2]; tb = -1 reports a scan
                                       that did not find its begin (a defect, never an input's property) */
    void* workspace;                /* device, gwhip_semiglobal_workspace_bytes(n_pairs, max_query_length) */
    size_t workspace_bytes;
} gwhip_semiglobal_args;

/* O(query) words per pair for queries beyond GWHIP_SEMIGLOBAL_REGISTER_QUERY, 256 otherwise. No matrix is stored. */
size_t gwhip_semiglobal_workspace_bytes(int32_t n_pairs, int32_t max_query_length);

/* The forward scan (d, te; tb = 0) and, for infix, the reversed anchored scan (tb), one wave64 per pair, asynchronous
   on `stream`. Returns 0 or a hipError_t as int (gwhip_semiglobal_last_error). */
int gwhip_semiglobal_ends(const gwhip_semiglobal_args* args, void* stream);

/* The input of the traceback: sub-pair s (of n_sub) is pair pair_index[s]; writes its query to
   out[out_starts[2s] .. out_starts[2s + 1]) and T[tb:te] to out[out_starts[2s + 1] .. out_starts[2s + 2]). out_starts is the
   caller's ([2 n_sub + 1], device): its lengths must be the pairs' n and te - tb. */
int gwhip_semiglobal_gather(int32_t n_sub, const int32_t* pair_index, const char* sequences, const int64_t* sequence_starts,
                            const int32_t* ends, const int64_t* out_starts, char* out, void* stream);

const char* gwhip_semiglobal_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
