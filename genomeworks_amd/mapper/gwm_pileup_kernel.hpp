// gwm_pileup_kernel.hpp -- device only: the pileup consumer of the chunk loop (gwm_align_chunks.hpp), shared by the
// two units that run it on a chunk's alignment states: gwm_pileup.hip, whose result the counters are, and
// gwm_variants.hip, which calls variants from them. pileup_kernel adds the alignments of a chunk into six counters per
// base of the owner set, add_role launches it for one role, zeroed_counts sizes and clears the counters. The rules are
// those of gwm_overlap_pileup and gwm_pair_pileup (include/gwhip_mapper.h).
#ifndef GWM_PILEUP_KERNEL_HPP
#define GWM_PILEUP_KERNEL_HPP

#include "gwm_column_walk.hpp"

namespace
{

constexpr uint32_t kChannels = 6, kDeletion = 4, kInsertion = 5;

// One wave64 per alignment of the chunk (states as AlignedChunk lays them out). counts: channel-major planes of
// n_bases cells each, counts[c * n_bases + owner.offsets[read] + p] for position p of a read of the owner set.
// kQueryRole says whose positions are counted: the target read's (`own` = the target position, `other` = the query
// position, the supplier is the query read) or, in the query role, the query read's, supplied by the target read. A
// column of state < 2 adds 1 to the channel of the supplier's base at `other`, complemented on '-'; a column that
// consumes a base of the owner alone (state 2, in the query role 3) adds 1 to the deletion channel; a maximal run of
// columns that consume none (state 3, in the query role 2) adds 1 to the insertion channel of the smaller owner
// position of its two neighbours, when it has a neighbour on both sides: 1 <= c <= slice length - 1 with c the owner
// bases consumed before the run. Every cell lies in the owner's slice and every supplier byte in the supplier's, which
// align_chunks() has checked against the reads; the counts are compared with the slice lengths all the same.
template <bool kQueryRole>
__global__ void __launch_bounds__(kThreads) pileup_kernel(const gwm_overlap* __restrict__ o,
                                                          const uint8_t* __restrict__ results,
                                                          const int64_t* __restrict__ starts,
                                                          const int32_t* __restrict__ result_lengths, int64_t m,
                                                          ReadSet qset, ReadSet tset, int64_t n_bases,
                                                          uint32_t* __restrict__ counts)
{
    const int64_t i     = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= m)
        return; // whole waves leave together
    const WaveAlignment w(o, results, starts, result_lengths, i);
    const gwm_overlap& x        = w.x;
    const uint32_t query_length = x.query_end_position_in_read - w.qs, target_length = w.te - w.ts;
    const uint32_t own_length   = kQueryRole ? query_length : target_length;
    const int64_t query_at      = qset.offsets[x.query_read_id - qset.first_read_id];
    const int64_t target_at     = tset.offsets[x.target_read_id - tset.first_read_id];
    const uint8_t* supplier     = kQueryRole ? tset.bases + target_at : qset.bases + query_at;
    uint32_t* cells             = counts + (kQueryRole ? query_at : target_at);
    constexpr uint32_t kSkips   = kQueryRole ? 2u : 3u; // the state that consumes no base of the owner
    const uint64_t lower        = (1ull << lane) - 1;
    // wave-uniform: columns walked so far that consume a query / a target base, the state of the last one
    uint32_t query_run = 0, target_run = 0, last_state = 0;
    for (uint32_t base = 0; base < w.len; base += 64)
    {
        const TileColumn c(w, base, lane, lower, query_run, target_run);
        query_run = c.query_run, target_run = c.target_run;
        const bool valid     = c.valid;
        const uint32_t state = c.state;
        const uint32_t own = kQueryRole ? c.q : c.t, other = kQueryRole ? c.t : c.q;
        const uint32_t consumed = kQueryRole ? c.a : c.b; // owner bases before this column
        // the previous column: the next lower lane, or the last column of the tile before
        uint32_t before = __shfl_up(state, 1, 64);
        if (lane == 0)
            before = last_state;
        if (valid && state != kSkips && consumed < own_length)
        {
            uint32_t channel = kDeletion;
            if (state < 2 && c.a < query_length && c.b < target_length)
            {
                const uint32_t code = (static_cast<uint32_t>(supplier[other]) >> 1) & 3u; // A, C, T, G = 0, 1, 2, 3
                channel             = code ^ (code >> 1);                                 // A, C, G, T = 0, 1, 2, 3
                if (w.reverse)
                    channel = 3u - channel;
            }
            (void)atomicAdd(cells + static_cast<int64_t>(channel) * n_bases + own, 1u);
        }
        else if (valid && state == kSkips && before != kSkips && consumed >= 1 && consumed + 1 <= own_length)
        {
            // a run's first column, with owner bases on both sides (a run in column 0 has consumed none)
            // `own` is the owner position behind the run in column order: the larger neighbour where it ascends
            const uint32_t p = !kQueryRole && w.reverse ? own : own - 1;
            (void)atomicAdd(cells + static_cast<int64_t>(kInsertion) * n_bases + p, 1u);
        }
        last_state = __shfl(state, 63, 64);
    }
}

// the zeroed counters of a read set whose offsets are on the device: six planes of offsets[n_reads] cells
int64_t zeroed_counts(const int64_t* offsets, int32_t n_reads, hipStream_t s, dbuf<uint32_t>& counts)
{
    const int64_t n_bases = offsets ? to_host(offsets + n_reads, s) : 0;
    if (n_bases < 0)
        throw std::invalid_argument("read offsets that end below 0");
    counts.resize(kChannels * n_bases);
    if (n_bases > 0)
        GWM_CHECK(hipMemsetAsync(counts.p, 0, sizeof(uint32_t) * static_cast<size_t>(kChannels * n_bases), s));
    return n_bases;
}

template <bool kQueryRole>
void add_role(const AlignedChunk& c, const ReadSet& q, const ReadSet& t, int64_t n_bases, uint32_t* counts,
              hipStream_t s)
{
    pileup_kernel<kQueryRole><<<c.m_waves, kThreads, 0, s>>>(c.overlaps, c.results, c.starts, c.result_lengths, c.m, q,
                                                              t, n_bases, counts);
    GWM_CHECK(hipGetLastError());
}

} // namespace

#endif
