"""The names of GWHIP_DEBUG, the integer that steers the POA kernels' debug instantiations, for the tests and tools.

csrc/poa_debug_flags.h is the registry: what each name does, which routine reads it and which names share bits is said
there. This module holds the same names with the same values (tests/test_debug_flags.py keeps the two equal) and
env_value(), which turns names and field values into the string for the environment variable."""

# A/B switches: results must be bit-identical with and without
kDbgConsensusNodeByNode = 1 << 4
kDbgTbNoLanes = 1 << 5
kDbgTbNoWideMoves = 1 << 6
kDbgTbNoStaged = 1 << 7
kDbgNoPackedPasses = 1 << 8
kDbgRingToGeneral = 1 << 9
kDbgRegistersToRing = 1 << 10
kDbgRegistersToGeneral = 1 << 11
kDbgMovedToRing = 1 << 15
kDbgTopsortIncrHbmOnly = 1 << 16
kDbgTopsortCachedFull = 1 << 17
kDbgSingleWaveForward = 1 << 18
kDbgTopsortFullResort = 1 << 21
kDbgRerunEveryStep = 1 << 23
kDbgEveryRowStoresScores = 1 << 25
kDbgManyPredsToGeneral = 1 << 30

# ablations: results are garbage, only timings mean anything
kDbgNoScoreStores = 1 << 0
kDbgNoRingStores = 1 << 1
kDbgAblationsOn = 1 << 14
kDbgAblNoRows = 1 << 16
kDbgAblNoMoveBytes = 1 << 17
kDbgAblNoScan = 1 << 18
kDbgAblNoGuard = 1 << 19
kDbgAblNoRingWrite = 1 << 20
kDbgAblNoScoreRowStores = 1 << 26
kDbgAblNoMoveRowStores = 1 << 27

# profiling selectors and counters (they arrive in the "other" phase accumulator)
kDbgTbCountAllSteps = 1 << 1
kDbgTimeGeneralRows = 1 << 2
kDbgCountGeneralRows = 1 << 3
kDbgKindCount = 1 << 12
kDbgKindFine = 1 << 13
kDbgRowsPerPath = 1 << 20
kDbgCountReruns = 1 << 24
kDbgSkewField = 15 << 12
kDbgMergeField = 7 << 16
kDbgTbField = 7 << 22
kDbgTopsortField = 7 << 25
kDbgRowKindField = 7 << 28

kDbgSkewShift, kDbgSkewMask = 12, 15
kDbgSkewRowsWorked = 1
kDbgSkewRowsSkipped = 2
kDbgSkewBlockBarriers = 3
kDbgSkewPassCycles = 4
kDbgSkewLeftWaitCycles = 5
kDbgSkewRingWaitCycles = 6
kDbgSkewGeneralRows = 7
kDbgSkewBodyCycles = 8
kDbgSkewPolls = 9
kDbgSkewRowStartWaitCycles = 10
kDbgSkewFirstBlockCycles = 11
kDbgSkewFirstBlockRows = 12
kDbgSkewRowTableCycles = 13
kDbgSkewFarBarrierCycles = 14

kDbgMergeShift, kDbgMergeMask = 16, 7
kDbgMergeLoad = 1
kDbgMergeClassify = 2
kDbgMergeCreate = 3
kDbgMergeEdges = 4

kDbgTbShift, kDbgTbMask = 22, 7
kDbgTbSinkCycles = 1
kDbgTbStepCycles = 4
kDbgTbSteps = 5
kDbgTbPostPassCycles = 6

kDbgTopsortShift, kDbgTopsortMask = 25, 7
kDbgTopsortPhase1Cycles = 1
kDbgTopsortBlockCycles = 2
kDbgTopsortStepCycles = 3
kDbgTopsortPhase3Cycles = 4
kDbgTopsortBlocks = 5
kDbgTopsortSteps = 6

kDbgRowKindShift, kDbgRowKindMask = 28, 7


def kDbgRowKindSelect(kind):
    """The row-kind field for `kind` (a table kind, or with kDbgKindFine a descriptor kind): it holds kind + 1."""
    return (kind + 1) << kDbgRowKindShift


def env_value(*names, skew=0, merge=0, tb=0, topsort=0, row_kind=None):
    """The string for GWHIP_DEBUG: the single-bit `names` together with the given values of the profiling fields."""
    fields = ((skew, kDbgSkewShift, kDbgSkewMask), (merge, kDbgMergeShift, kDbgMergeMask), (tb, kDbgTbShift, kDbgTbMask),
              (topsort, kDbgTopsortShift, kDbgTopsortMask))
    value = 0
    for name in names:
        value |= name
    for v, shift, mask in fields:
        if not 0 <= v <= mask:
            raise ValueError("field value %d does not fit its mask %d" % (v, mask))
        value |= v << shift
    if row_kind is not None:
        if not 0 <= row_kind + 1 <= kDbgRowKindMask:
            raise ValueError("row kind %d does not fit the field" % row_kind)
        value |= kDbgRowKindSelect(row_kind)
    return str(value)
