/*
 * gwhip_affine.h -- kernel-level C-ABI of the affine-gap global aligner (libgwaffine.so): a batch of pairs aligned end
 * to end under gap-open / gap-extend costs inside a diagonal band, forward pass and traceback on the device.
 *
 * The object-level API on top of it is cudaaligner::create_aligner_affine (C++, cudaaligner/aligner_affine.hpp),
 * gw_aligner_create_affine (gw_capi.h) and CudaAlignerBatch(algorithm="affine") (Python); cudamapper reaches it through
 * gwm_align_overlaps_scored / gwm_overlap_variants_scored (gwhip_mapper.h). This header is kept apart from gwhip.h on
 * purpose, as gwhip_semiglobal.h is: the POA / aligner kernel set and its source digest are not affected by it. The
 * affine X-drop extension of the same library (gwhip_extend; create_aligner_extension, gw_aligner_create_extension,
 * CudaAlignerBatch(algorithm="extend")) is stated at the end of this header.
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

/* ---- affine X-drop extension (genomeworks_amd/affine/gwaffine_extend_rules.h is its code) ------
 * Not a global alignment: it starts at cell (0, 0) of Q and T and stops where the similarity stops. Scores are
 * maximised: match +a, mismatch -x, a gap run of L columns -(o + L e). It is the DP above under the derived costs
 * x' = 2 (a + x), o' = 2 o, e' = a + 2 e: the best score of Q[:i] with T[:j] is (a (i + j) - H'[i][j]) / 2, and the cell
 * update, its ties and the cell's byte are the one-piece ones. The band is d = j - i in [-B, B] whatever n and m are;
 * the last anti-diagonal with a cell is a_max = min(n + m, 2 min(n, m) + B).
 * Stop rule, per anti-diagonal A = i + j, in the doubled score D = a (i + j) - H': top(A) is the largest D of A's cells,
 * best the largest D so far, A included. After A >= 1 with xdrop >= 0: when max(top(A), top(A - 1)) < best - 2 xdrop the
 * extension stops, dropped = 1, and no later anti-diagonal counts. The end cell is the cell of largest D up to there,
 * on ties the smallest anti-diagonal, then the smallest d; (0, 0) with score 0 is always a candidate. The states of the
 * path from the end cell back to (0, 0) are written back to front, as above. A pair with n + m >= 2^21, or one that does
 * not fit the workspace given, gets score -1, ends -1, length 0. */
#define GWHIP_EXTEND_MAX_BAND 511
#define GWHIP_EXTEND_MAX_XDROP (1 << 20)

typedef struct gwhip_extend_args
{
    int32_t n_alignments;
    const char* sequences;               /* as gwhip_affine_args: device, q0 t0 q1 t1 ... */
    const int64_t* sequence_starts;      /* device, [2n + 1] */
    const int64_t* sequence_starts_host; /* host, [2n + 1] */
    int32_t match;                       /* a >= 1 */
    int32_t mismatch;                    /* x >= 0, a + x <= 127 */
    int32_t gap_open;                    /* o in 0 .. 127 */
    int32_t gap_extend;                  /* e >= 1, a + 2 e <= 255 */
    int32_t band;                        /* B in 0 .. GWHIP_EXTEND_MAX_BAND */
    int32_t xdrop;                       /* X in 0 .. GWHIP_EXTEND_MAX_XDROP, or -1: never stop */
    int8_t* results;                     /* device, states BACK TO FRONT in the pair's slot as above; NULL: score-only mode,
                                            no bit is written, no traceback runs, result_lengths and workspace may be NULL */
    int32_t* result_lengths;             /* device, [n]: columns of the path from the end cell; 0 = none */
    int32_t* scores;                     /* device, [n]: the end cell's score; -1 = no result */
    int32_t* query_ends;                 /* device, [n]: i of the end cell, Q[:i] is aligned; -1 = no result */
    int32_t* target_ends;                /* device, [n]: j of the end cell; -1 = no result */
    uint8_t* dropped;                    /* device, [n]: 1 when the stop rule ended the extension before a_max */
    void* workspace;                     /* device, gwhip_extend_workspace_bytes(..., 1) */
    size_t workspace_bytes;
} gwhip_extend_args;

/* with_traceback != 0: 8 (n + 1) bytes of offsets and, per pair with n + m < 2^21, (a_max + 1) * roundup4((2 B + 3) / 2)
   bytes, each part rounded up to 256. with_traceback == 0: 0, score-only mode needs no workspace. Arguments that no call
   would be accepted with (n_alignments <= 0, no sequence_starts_host, a band outside 0 .. GWHIP_EXTEND_MAX_BAND, starts that
   do not ascend) give 256, the size of an empty batch's offsets, as gwhip_affine_workspace_bytes does. */
size_t gwhip_extend_workspace_bytes(int32_t n_alignments, const int64_t* sequence_starts_host, int32_t band, int32_t with_traceback);

/* Offsets, forward pass and traceback (one wave64 per pair each; the forward pass alone in score-only mode), asynchronous
   on `stream`. A value out of range, a missing pointer and a workspace smaller than gwhip_extend_workspace_bytes() are
   refused before anything is launched; an empty batch launches nothing. Returns 0 or a hipError_t as int
   (gwhip_affine_last_error). gwhip_extend_events records the caller's three HIP events as gwhip_affine_align_events. */
int gwhip_extend(const gwhip_extend_args* args, void* stream);
int gwhip_extend_events(const gwhip_extend_args* args, void* stream, void* const events[3]);

const char* gwhip_affine_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
