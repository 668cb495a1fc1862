// gwm_column_walk.hpp -- device only: how the consumers of the chunk loop (gwm_align_chunks.hpp) read the alignments
// of an AlignedChunk, one wave64 per alignment over tiles of 64 columns in forward column order. WaveStates is where
// the states of the wave's alignment lie and how a lane loads its column; WaveAlignment adds the overlap record, and
// TileColumn gives every lane the query and target position of its column: ballots of the columns that consume a
// query / a target base, popcounts over the lower lanes, and the running counts that the caller carries between tiles
// in wave-uniform registers. The CIGAR writer (gwm_align.hip) needs no positions and uses WaveStates alone; the
// segment writer (gwm_segments.hip) and the pileup (gwm_pileup.hip) walk. What is done with a column is the kernel's.
#ifndef GWM_COLUMN_WALK_HPP
#define GWM_COLUMN_WALK_HPP

#include "gwm_align_chunks.hpp"

namespace
{

// The states of alignment i of a chunk: back to front at results[starts[2 i]], column j at s[len - 1 - j].
struct WaveStates
{
    int64_t slot;
    const uint8_t* s;
    uint32_t len;
    __device__ __forceinline__ WaveStates(const uint8_t* results, const int64_t* starts, const int32_t* result_lengths,
                                          int64_t i)
        : slot(starts[2 * i]), s(results + slot)
    {
        const int32_t stored = result_lengths[i];
        len                  = static_cast<uint32_t>(stored < 0 ? -stored : stored); // as the host aligner reads it
    }
    // the state of column base + lane of a tile, 0 behind the last column
    __device__ __forceinline__ uint32_t state(uint32_t base, uint32_t lane, bool valid) const
    {
        return valid ? s[len - 1 - base - lane] : 0u;
    }
    // `edits` columns that are not a match; -1: no result although a slice was not empty
    __device__ __forceinline__ int32_t edit_distance(uint32_t edits, const int64_t* starts, int64_t i) const
    {
        return len ? static_cast<int32_t>(edits) : (starts[2 * i + 2] == slot ? 0 : -1);
    }
};

// The alignment of a wave: its states and its overlap record. Forward column order is ascending query order, and
// ascending target order on '+', descending from te - 1 on '-'.
struct WaveAlignment : WaveStates
{
    gwm_overlap x;
    bool reverse;
    uint32_t qs, ts, te;
    __device__ __forceinline__ WaveAlignment(const gwm_overlap* o, const uint8_t* results, const int64_t* starts,
                                             const int32_t* result_lengths, int64_t i)
        : WaveStates(results, starts, result_lengths, i), x(o[i]), reverse(x.relative_strand == '-'),
          qs(x.query_start_position_in_read), ts(x.target_start_position_in_read), te(x.target_end_position_in_read)
    {
    }
};

// One step of the walk: what a lane knows of its column of the tile [base, base + 64) of w. lower = the lanes below
// this one. query_run_before / target_run_before: the columns before the tile that consume a query / a target base;
// the caller carries them from tile to tile and takes them, advanced, from query_run / target_run. (They go in by
// value and come out as members: counters advanced through a reference, or a tile returned from a function, cost
// the kernels registers.)
struct TileColumn
{
    bool valid;
    uint32_t state;
    uint64_t in_query, in_target; // the lanes whose columns consume a query / a target base
    uint32_t a, b;                // query / target bases consumed before this column
    uint32_t q, t; // its positions in the query / target read (of the next base to come where it consumes none)
    uint32_t query_run, target_run; // the running counts behind the tile (wave-uniform)
    __device__ __forceinline__ TileColumn(const WaveAlignment& w, uint32_t base, uint32_t lane, uint64_t lower,
                                          uint32_t query_run_before, uint32_t target_run_before)
    {
        valid      = lane < min(64u, w.len - base);
        state      = w.state(base, lane, valid);
        in_query   = __ballot(valid && state != 2);
        in_target  = __ballot(valid && state != 3);
        a          = query_run_before + static_cast<uint32_t>(__popcll(in_query & lower));
        b          = target_run_before + static_cast<uint32_t>(__popcll(in_target & lower));
        q          = w.qs + a;
        t          = w.reverse ? w.te - 1 - b : w.ts + b;
        query_run  = query_run_before + static_cast<uint32_t>(__popcll(in_query));
        target_run = target_run_before + static_cast<uint32_t>(__popcll(in_target));
    }
};

} // namespace

#endif
