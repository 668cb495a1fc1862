/*
 * gwhip_affine.h -- kernel-level C-ABI of the affine-gap global aligner (libgwaffine.so): a batch of pairs aligned end
 * to end under gap-open / gap-extend costs inside a diagonal band, forward pass and traceback on the device.
 *
 * The object-level API on top of it is cudaaligner::create_aligner_affine (C++, cudaaligner/aligner_affine.hpp),
 * gw_aligner_create_affine (gw_capi.h) and CudaAlignerBatch(algorithm="affine") (Python); cudamapper reaches it through
 * gwm_align_overlaps_scored / gwm_overlap_variants_scored (gwhip_mapper.h). This header is kept apart from gwhip.h on
 * purpose, as gwhip_semiglobal.h is: the POA / aligner kernel set and its source digest are not affected by it.
 *
 * Rules (genomeworks_amd/affine/gwaffine_rules.h is their code). Query Q of n bases,
 * target T of m bases; q matches t when q == "ACTG"[(t >> 1) & 3]. Costs are minimised: match 0, mismatch x, a gap
 * run of L columns o + L e. Diagonal d = j - i; the band is [min(0, m - n) - B, max(0, m - n) + B], W = |m - n| + 2 B + 1
 * diagonals; a cell outside it does not exist. H[0][0] = 0,
 *   E[i][j] = min(E[i][j-1] + e, H[i][j-1] + o + e)    (state 2, a target-only column)
 *   F[i][j] = min(F[i-1][j] + e, H[i-1][j] + o + e)    (state 3, a query-only column)
 *   H[i][j] = min(H[i-1][j-1] + sub, E[i][j], F[i][j])
 * with ties: extension before opening, diagonal before E before F. The traceback follows the recorded choices from
 * (n, m) in H. A pair with W > GWHIP_AFFINE_MAX_DIAGONALS or n + m >= 2^21 gets no result: length 0, cost -1.
 */
#ifndef GWHIP_AFFINE_H
#define GWHIP_AFFINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GWHIP_AFFINE_MAX_DIAGONALS 2048

typedef struct gwhip_affine_args
{
    int32_t n_alignments;
    const char* sequences;               /* device, concatenated: q0 t0 q1 t1 ... (as gwhip_hirschberg_args) */
    const int64_t* sequence_starts;      /* device, [2n + 1] */
    const int64_t* sequence_starts_host; /* host, [2n + 1], the same lengths (only differences are read): sizes the
                                            workspace check and selects the kernel variant from the widest band */
    int32_t mismatch;                    /* 1 .. 255 */
    int32_t gap_open;                    /* 0 .. 255 */
    int32_t gap_extend;                  /* 1 .. 255 */
    int32_t band;                        /* B >= 0 */
    int8_t* results;                     /* device: alignment i's states (0 match, 1 mismatch, 2 target-only column,
                                            3 query-only column) BACK TO FRONT in the slot
                                            [sequence_starts[2i], sequence_starts[2i + 2]) */
    int32_t* result_lengths;             /* device, [n]: columns; 0 = no result, or two empty sequences */
    int32_t* costs;                      /* device, [n]: H[n][m]; -1 = no result */
    uint8_t* optimal;                    /* device, [n]: 1 when cost <= 2 o + e (|m - n| + 2 B + 2), the cheapest path that
                                            leaves the band: the cost is then the full-matrix optimum */
    void* workspace;                     /* device, gwhip_affine_workspace_bytes(...) */
    size_t workspace_bytes;
} gwhip_affine_args;

/* 8 (n + 1) bytes of offsets and, per aligned pair, one byte per cell of the band's half-rows:
   (n + m + 1) * roundup4((W + 2) / 2), each part rounded up to 256. */
size_t gwhip_affine_workspace_bytes(int32_t n_alignments, const int64_t* sequence_starts_host, int32_t band);

/* Offsets, forward pass and traceback (one wave64 per pair each), asynchronous on `stream`. Parameters
   out of range, a missing pointer and a workspace smaller than gwhip_affine_workspace_bytes() are refused before
   anything is launched. Returns 0 or a hipError_t as int (gwhip_affine_last_error). */
int gwhip_affine_align(const gwhip_affine_args* args, void* stream);

/* measurement aid: as gwhip_affine_align, recording the caller's three HIP events (hipEvent_t) on `stream`: before the
   forward pass, between it and the traceback, behind the traceback. Nothing is waited for. */
int gwhip_affine_align_events(const gwhip_affine_args* args, void* stream, void* const events[3]);

/* ---- two-piece gap costs (genomeworks_amd/affine/gwaffine2_rules.h is their code) --------------
 * Query, target, match predicate, band, W, the workspace's stride and layout and the states written are those above. A
 * gap run of L columns costs g(L) = min(o1 + L e1, o2 + L e2); no order between the two pieces is required.
 *   E1[i][j] = min(E1[i][j-1] + e1, H[i][j-1] + o1 + e1)    E2 likewise with (o2, e2)    (state 2)
 *   F1[i][j] = min(F1[i-1][j] + e1, H[i-1][j] + o1 + e1)    F2 likewise with (o2, e2)    (state 3)
 *   H[i][j]  = min(H[i-1][j-1] + sub, E1[i][j], F1[i][j], E2[i][j], F2[i][j])
 * with ties: extension before opening in each of the four gap matrices; for H the diagonal, E1, F1, E2, F2 in this order,
 * a later one only when strictly smaller. A cell's byte (this instantiation's alone): bits 0-2 src (0 diagonal, 1 E1,
 * 2 F1, 3 E2, 4 F2), bit 3 E1ext, bit 4 F1ext, bit 5 E2ext, bit 6 F2ext, bit 7 mismatch. The traceback walks five
 * matrices: from H a non-zero src switches matrix and emits nothing; a gap matrix emits its state, steps, and returns to
 * H when its ext bit is clear (E2 and F2 open from H, never from E1 or F1). A pair with
 * W > GWHIP_AFFINE2_MAX_DIAGONALS or n + m >= 2^21 gets no result: length 0, cost -1, flag 0. */
#define GWHIP_AFFINE2_MAX_DIAGONALS 1024

typedef struct gwhip_affine2_args
{
    int32_t n_alignments;
    const char* sequences;               /* as gwhip_affine_args, field by field, ... */
    const int64_t* sequence_starts;
    const int64_t* sequence_starts_host;
    int32_t mismatch;                    /* 1 .. 255 */
    int32_t gap_open;                    /* o1, 0 .. 255 */
    int32_t gap_extend;                  /* e1, 1 .. 255 */
    int32_t gap_open2;                   /* ... plus o2, 0 .. 255 */
    int32_t gap_extend2;                 /* and e2, 1 .. 255 */
    int32_t band;                        /* B >= 0 */
    int8_t* results;
    int32_t* result_lengths;
    int32_t* costs;
    uint8_t* optimal;                    /* device, [n]: 1 when cost <= g(B + 1) + g(B + 1 + |m - n|), the cheapest path that
                                            leaves the band (with one piece: 2 o + e (|m - n| + 2 B + 2)) */
    void* workspace;                     /* device, gwhip_affine2_workspace_bytes(...) */
    size_t workspace_bytes;
} gwhip_affine2_args;

/* gwhip_affine_workspace_bytes' formula; a pair of more than GWHIP_AFFINE2_MAX_DIAGONALS diagonals counts 0. */
size_t gwhip_affine2_workspace_bytes(int32_t n_alignments, const int64_t* sequence_starts_host, int32_t band);

/* As gwhip_affine_align and gwhip_affine_align_events, under the two-piece costs: the same launches, the same refusals
   before anything is launched (a value out of range, a missing pointer, a workspace smaller than
   gwhip_affine2_workspace_bytes()), nothing launched for an empty batch. Errors: gwhip_affine_last_error. */
int gwhip_affine2_align(const gwhip_affine2_args* args, void* stream);
int gwhip_affine2_align_events(const gwhip_affine2_args* args, void* stream, void* const events[3]);

const char* gwhip_affine_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
