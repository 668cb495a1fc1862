// poa_debug_flags.h -- the registry of GWHIP_DEBUG, the one integer that steers the POA kernels' debug instantiations.
//
// Plain C++ (no HIP): poa_device.h includes it, so every device unit sees it, and a host-only program may include it too.
// genomeworks_amd/debug_flags.py holds the same names for the tests and tools (tests/test_debug_flags.py keeps the two equal).
//
// The environment variable is parsed with atoi (gwhip_switches.h), arrives in the kernels as KernelArgs::debug_flags and is
// handed down as `dbg`. Any value but 0 launches the debug instantiation of a window kernel; the production instantiation
// folds the integer to 0. Every name below keeps the number it has always had: committed profiles, scripts and notes that
// quote a raw value stay true.
//
// Three kinds of names:
//   AB    A/B switches: another routine computes the same thing. Results must be bit-identical with and without.
//   ABL   ablations: a piece of the work is left out. Results are garbage; only timings mean anything.
//   PROF  profiling selectors and counters: something is timed or counted into the "other" phase accumulator
//         (gwhip_poa_args::phase_cycles). Results are unchanged.
// A multi-bit field has a name for its bits in place (k...Field), a shift, a mask and names for its values.
//
// X(kind, name, bits): one line per name, with the routine that reads it.
#pragma once
#include <stdint.h>

// clang-format off
#define GWHIP_DEBUG_NAMES(X)                                                                                                        \
    /* ---- A/B switches ---- */                                                                                                    \
    X(AB,   kDbgConsensusNodeByNode,  1 << 4)  /* poa_consensus_lds_kernel: the first bundle pass node by node */                   \
    X(AB,   kDbgTbNoLanes,            1 << 5)  /* nw_banded: traceback_banded_lanes (LDS tables) is passed over */                  \
    X(AB,   kDbgTbNoWideMoves,        1 << 6)  /* nw_banded: not traceback_moves over the pipelined pass's move bytes */            \
    X(AB,   kDbgTbNoStaged,           1 << 7)  /* nw_banded: traceback_banded_tiled_staged is passed over */                        \
    X(AB,   kDbgNoPackedPasses,       1 << 8)  /* nw_banded, nw_banded_tb_packed, nw_full_packed: the generic passes instead */     \
    X(AB,   kDbgRingToGeneral,        1 << 9)  /* classify_kinds: ring rows (kinds 2, 3) through the general routine (4) */         \
    X(AB,   kDbgRegistersToRing,      1 << 10) /* classify_kinds: register rows (kinds 0, 1) through the ring (2) */                \
    X(AB,   kDbgRegistersToGeneral,   1 << 11) /* classify_kinds: register rows (kinds 0, 1) through the general routine (4) */     \
    X(AB,   kDbgMovedToRing,          1 << 15) /* classify_kinds: rows of a moved band (kind 1) through the ring (2) */             \
    X(AB,   kDbgTopsortIncrHbmOnly,   1 << 16) /* poa_window_kernel, graphs beyond the LDS tables: topsort_kahn_incr_hbm only */    \
    X(AB,   kDbgTopsortCachedFull,    1 << 17) /* poa_window_kernel, graphs beyond the LDS tables: topsort_kahn_cached */           \
    X(AB,   kDbgSingleWaveForward,    1 << 18) /* nw_banded: no generic_forward_skew across the wavefronts of a block */            \
    X(AB,   kDbgTopsortFullResort,    1 << 21) /* poa_window_kernel: a full re-sort after every read, no incremental order */       \
    X(AB,   kDbgRerunEveryStep,       1 << 23) /* nw_banded: every recomputed step of traceback_moves asks for the score rows */    \
    X(AB,   kDbgEveryRowStoresScores, 1 << 25) /* nw_banded, full_forward_moves: mark_score_rows keeps no score row out of HBM */   \
    X(AB,   kDbgManyPredsToGeneral,   1 << 30) /* classify_kinds, without kDbgKindFine: rows of 4..6 predecessors -> general */     \
    /* ---- ablations ---- */                                                                                                       \
    X(ABL,  kDbgNoScoreStores,        1 << 0)  /* banded_forward_1pass, nw_banded's generic rows: no score row to HBM */            \
    X(ABL,  kDbgNoRingStores,         1 << 1)  /* nw_banded's generic rows: no score row to the LDS ring */                         \
    X(ABL,  kDbgAblationsOn,          1 << 14) /* banded_forward_moves, full_forward_moves: honour the kDbgAbl... bits */           \
    X(ABL,  kDbgAblNoRows,            1 << 16) /* banded_forward_moves (tools/microbench_rows.hip): no rows at all */               \
    X(ABL,  kDbgAblNoMoveBytes,       1 << 17) /* banded_forward_moves (microbench): no move bytes */                               \
    X(ABL,  kDbgAblNoScan,            1 << 18) /* banded_forward_moves (microbench): no cross-lane scan */                          \
    X(ABL,  kDbgAblNoGuard,           1 << 19) /* banded_forward_moves (microbench): no guard write */                              \
    X(ABL,  kDbgAblNoRingWrite,       1 << 20) /* banded_forward_moves (microbench): no ring write */                               \
    X(ABL,  kDbgAblNoScoreRowStores,  1 << 26) /* banded_forward_moves, full_forward_moves: no score-row stores */                  \
    X(ABL,  kDbgAblNoMoveRowStores,   1 << 27) /* banded_forward_moves, full_forward_moves: no move-row stores */                   \
    /* ---- profiling selectors and counters ---- */                                                                                \
    X(PROF, kDbgTbCountAllSteps,      1 << 1)  /* traceback_banded_lanes: add the walk's steps */                                   \
    X(PROF, kDbgTimeGeneralRows,      1 << 2)  /* banded_forward_1pass: cycles in the rows of the general path */                   \
    X(PROF, kDbgCountGeneralRows,     1 << 3)  /* banded_forward_1pass, with kDbgTimeGeneralRows: their number instead */           \
    X(PROF, kDbgKindCount,            1 << 12) /* banded_forward_moves: rows of the selected kind counted, not timed; without a */  \
                                               /* row-kind selector the per-read prologue is timed */                               \
    X(PROF, kDbgKindFine,             1 << 13) /* banded_forward_moves: the selector names a descriptor kind, counts in units of */ \
                                               /* 2^32 / 2^48; nw_banded: a counted rerun adds 2^40; classify_kinds: see bit 30 */  \
    X(PROF, kDbgRowsPerPath,          1 << 20) /* nw_banded's generic rows: 1 per row served from the ring, 2^20 per other row */   \
    X(PROF, kDbgCountReruns,          1 << 24) /* nw_banded: reruns of the packed pass with every score row stored */               \
    X(PROF, kDbgSkewField,            15 << 12) /* generic_forward_skew: kDbgSkew... */                                             \
    X(PROF, kDbgMergeField,           7 << 16) /* add_alignment: kDbgMerge... */                                                    \
    X(PROF, kDbgTbField,              7 << 22) /* nw_banded (sink), traceback_banded_lanes: kDbgTb... */                            \
    X(PROF, kDbgTopsortField,         7 << 25) /* topsort_kahn_incr_lds: kDbgTopsort... */                                          \
    X(PROF, kDbgRowKindField,         7 << 28) /* banded_forward_moves: row kind + 1 (kDbgRowKindSelect) */
// clang-format on

namespace gwhip
{

#define GWHIP_DEBUG_CONSTANT(kind, name, bits) constexpr int32_t name = bits;
GWHIP_DEBUG_NAMES(GWHIP_DEBUG_CONSTANT)
#undef GWHIP_DEBUG_CONSTANT

// generic_forward_skew (sum over the wavefronts)
constexpr int32_t kDbgSkewShift = 12, kDbgSkewMask = 15;
constexpr int32_t kDbgSkewRowsWorked          = 1;  // rows worked on
constexpr int32_t kDbgSkewRowsSkipped         = 2;  // rows skipped
constexpr int32_t kDbgSkewBlockBarriers       = 3;  // block barriers (x 1000)
constexpr int32_t kDbgSkewPassCycles          = 4;  // cycles in the pass
constexpr int32_t kDbgSkewLeftWaitCycles      = 5;  // cycles waiting for the left neighbour
constexpr int32_t kDbgSkewRingWaitCycles      = 6;  // cycles waiting for ring space
constexpr int32_t kDbgSkewGeneralRows         = 7;  // rows on the general path
constexpr int32_t kDbgSkewBodyCycles          = 8;  // cycles in the row bodies (waits included)
constexpr int32_t kDbgSkewPolls               = 9;  // polls
constexpr int32_t kDbgSkewRowStartWaitCycles  = 10; // cycles waiting for the left neighbour at the start of a row
constexpr int32_t kDbgSkewFirstBlockCycles    = 11; // cycles in the bodies of first-block rows
constexpr int32_t kDbgSkewFirstBlockRows      = 12; // their number
constexpr int32_t kDbgSkewRowTableCycles      = 13; // cycles in the row-table batches
constexpr int32_t kDbgSkewFarBarrierCycles    = 14; // cycles in the block barriers of far rows

// add_alignment: cycles of one of its phases
constexpr int32_t kDbgMergeShift = 16, kDbgMergeMask = 7;
constexpr int32_t kDbgMergeLoad     = 1;
constexpr int32_t kDbgMergeClassify = 2;
constexpr int32_t kDbgMergeCreate   = 3;
constexpr int32_t kDbgMergeEdges    = 4;

// nw_banded's sink selection and traceback_banded_lanes
constexpr int32_t kDbgTbShift = 22, kDbgTbMask = 7;
constexpr int32_t kDbgTbSinkCycles     = 1; // cycles of the sink selection
constexpr int32_t kDbgTbStepCycles     = 4; // cycles in the steps (tile loads included)
constexpr int32_t kDbgTbSteps          = 5; // their number (x 1000)
constexpr int32_t kDbgTbPostPassCycles = 6; // cycles of the post-pass

// topsort_kahn_incr_lds
constexpr int32_t kDbgTopsortShift = 25, kDbgTopsortMask = 7;
constexpr int32_t kDbgTopsortPhase1Cycles = 1;
constexpr int32_t kDbgTopsortBlockCycles  = 2; // cycles in the replayed blocks
constexpr int32_t kDbgTopsortStepCycles   = 3; // cycles in the ordinary steps
constexpr int32_t kDbgTopsortPhase3Cycles = 4;
constexpr int32_t kDbgTopsortBlocks       = 5; // number of blocks (x 1000)
constexpr int32_t kDbgTopsortSteps        = 6; // number of ordinary steps (x 1000)

// banded_forward_moves: the field holds a row kind + 1 -- a table kind (0..4: 3 = every ring row of several predecessors), or
// with kDbgKindFine a descriptor kind (kDk... of poa_forward_row_operands.h, 0..6)
constexpr int32_t kDbgRowKindShift = 28, kDbgRowKindMask = 7;
constexpr int32_t kDbgRowKindSelect(int32_t kind) { return (kind + 1) << kDbgRowKindShift; }

// ------------------------------------------------------------------------------------------------
// The overlaps. Names of one row share bits; every pair of names that share a bit is listed, and nothing else is
// (checked below: a new name on a used bit does not compile until it has a row here).
//
//   names                                             bits    can they meet?
//   kDbgNoRingStores / kDbgTbCountAllSteps             1      yes, one kernel reads both: an ablated run (garbage anyway) also
//                                                             adds its traceback steps to "other"
//   kDbgSkewField / kDbgKindCount, kDbgKindFine,       12-15  no: generic_forward_skew runs only in the multi-wave kernels without
//     kDbgAblationsOn, kDbgMovedToRing                        LDS tables, the other four are read by the packed passes, which need
//                                                             the LDS tables
//   kDbgMergeField / kDbgTopsortIncrHbmOnly,           16-18  yes: add_alignment runs in every kernel, so each of the three A/B
//     kDbgTopsortCachedFull, kDbgSingleWaveForward            switches also selects kDbgMergeLoad, kDbgMergeClassify or
//                                                             kDbgMergeEdges: cycles arrive in "other", results do not change
//   kDbgAblNoRows, kDbgAblNoMoveBytes, kDbgAblNoScan   16-18  only with kDbgAblationsOn, meant for tools/microbench_rows.hip, which
//     / the three A/B switches and kDbgMergeField             has neither topsort nor merge; in a window kernel they meet and the
//                                                             results are garbage
//   kDbgAblNoRingWrite / kDbgRowsPerPath               20     no within a window: the packed pass (with kDbgAblationsOn) or the
//                                                             generic rows run, never both
//   kDbgTbField / kDbgRerunEveryStep, kDbgCountReruns  22-24  the two bits are read only after a packed pass, kDbgTbStepCycles ..
//                                                             kDbgTbPostPassCycles only by traceback_banded_lanes, which runs when
//                                                             no packed pass did, and kDbgTbSinkCycles (1) is neither bit. In a
//                                                             batch that mixes both sorts of windows kDbgCountReruns is also
//                                                             kDbgTbStepCycles for the windows without a packed pass
//   kDbgTopsortField / kDbgEveryRowStoresScores        25     yes: the switch also selects kDbgTopsortPhase1Cycles when phase
//                                                             cycles are collected; results do not change
//   kDbgTopsortField / kDbgAblNoScoreRowStores,        26-27  yes, which is why the two are honoured only with kDbgAblationsOn:
//     kDbgAblNoMoveRowStores                                  the topsort selectors 2, 3, 4 and 6 alone ablate nothing
//   kDbgRowKindField / kDbgManyPredsToGeneral          30     yes: without kDbgKindFine a kind selector of 4 and more demotes the
//                                                             rows of 4..6 predecessors (and the switch alone selects table kind
//                                                             3 for the row counters); with kDbgKindFine nothing is demoted
// ------------------------------------------------------------------------------------------------
namespace debug_flags_check
{
enum Kind { AB, ABL, PROF };
#define GWHIP_DEBUG_ID(kind, name, bits) id_##name,
enum Id { GWHIP_DEBUG_NAMES(GWHIP_DEBUG_ID) kNames };
#undef GWHIP_DEBUG_ID
struct Name { Kind kind; int32_t bits; };
#define GWHIP_DEBUG_ENTRY(kind, name, bits) {kind, name},
constexpr Name kAll[kNames] = {GWHIP_DEBUG_NAMES(GWHIP_DEBUG_ENTRY)};
#undef GWHIP_DEBUG_ENTRY
struct Overlap { Id a, b; };
constexpr Overlap kOverlaps[] = {
    {id_kDbgNoRingStores, id_kDbgTbCountAllSteps},
    {id_kDbgSkewField, id_kDbgKindCount}, {id_kDbgSkewField, id_kDbgKindFine}, {id_kDbgSkewField, id_kDbgAblationsOn},
    {id_kDbgSkewField, id_kDbgMovedToRing},
    {id_kDbgMergeField, id_kDbgTopsortIncrHbmOnly}, {id_kDbgMergeField, id_kDbgTopsortCachedFull}, {id_kDbgMergeField, id_kDbgSingleWaveForward},
    {id_kDbgAblNoRows, id_kDbgTopsortIncrHbmOnly}, {id_kDbgAblNoMoveBytes, id_kDbgTopsortCachedFull}, {id_kDbgAblNoScan, id_kDbgSingleWaveForward},
    {id_kDbgAblNoRows, id_kDbgMergeField}, {id_kDbgAblNoMoveBytes, id_kDbgMergeField}, {id_kDbgAblNoScan, id_kDbgMergeField},
    {id_kDbgAblNoRingWrite, id_kDbgRowsPerPath},
    {id_kDbgTbField, id_kDbgRerunEveryStep}, {id_kDbgTbField, id_kDbgCountReruns},
    {id_kDbgTopsortField, id_kDbgEveryRowStoresScores}, {id_kDbgTopsortField, id_kDbgAblNoScoreRowStores}, {id_kDbgTopsortField, id_kDbgAblNoMoveRowStores},
    {id_kDbgRowKindField, id_kDbgManyPredsToGeneral},
};
constexpr bool listed(int i, int j)
{
    for (const Overlap& o : kOverlaps)
        if ((o.a == i && o.b == j) || (o.a == j && o.b == i)) return true;
    return false;
}
constexpr bool overlaps_are_the_listed_ones()
{
    for (int i = 0; i < kNames; i++)
        for (int j = i + 1; j < kNames; j++)
            if (((kAll[i].bits & kAll[j].bits) != 0) != listed(i, j)) return false;
    return true;
}
constexpr bool ab_switches_are_disjoint()
{
    for (int i = 0; i < kNames; i++)
        for (int j = i + 1; j < kNames; j++)
            if (kAll[i].kind == AB && kAll[j].kind == AB && (kAll[i].bits & kAll[j].bits) != 0) return false;
    return true;
}
constexpr bool no_name_uses_bit_31() // (atoi parses the value: it must stay a positive int)
{
    for (const Name& n : kAll)
        if (n.bits <= 0) return false;
    return true;
}
static_assert(overlaps_are_the_listed_ones(), "GWHIP_DEBUG: two names share a bit and the table of overlaps does not say so (or says so wrongly)");
static_assert(ab_switches_are_disjoint(), "GWHIP_DEBUG: two A/B switches share a bit");
static_assert(no_name_uses_bit_31(), "GWHIP_DEBUG: bit 31 is out of atoi's reach");
static_assert((kDbgSkewMask << kDbgSkewShift) == kDbgSkewField && (kDbgMergeMask << kDbgMergeShift) == kDbgMergeField &&
                  (kDbgTbMask << kDbgTbShift) == kDbgTbField && (kDbgTopsortMask << kDbgTopsortShift) == kDbgTopsortField &&
                  (kDbgRowKindMask << kDbgRowKindShift) == kDbgRowKindField,
              "GWHIP_DEBUG: a field's shift and mask do not give its bits");
} // namespace debug_flags_check

} // namespace gwhip
