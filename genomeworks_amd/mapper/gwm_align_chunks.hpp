// gwm_align_chunks.hpp -- the chunk loop that gwm_align_overlaps (gwm_align.hip), gwm_window_segments
// (gwm_segments.hip) and gwm_overlap_pileup (gwm_pileup.hip) share: validation of the overlap records, sizing on the host, and per chunk of consecutive
// overlaps the gather of the slices, gwhip_hirschberg_myers of libgwhip.so and the per-chunk buffers. What is done with
// the chunk's alignment states is the caller's: align_chunks() hands them to a consumer while they are on the device.
// The loop and its kernels are defined once, in gwm_align.hip.
#ifndef GWM_ALIGN_CHUNKS_HPP
#define GWM_ALIGN_CHUNKS_HPP

#include "gwhip_mapper.h"

#include "gwm_device_utils.hpp"

#include <functional>
#include <vector>

namespace gwm
{

// What a consumer sees of one chunk: overlaps [first, first + m) of the call, their states and where they lie. The
// states of alignment i of the chunk lie back to front at results[starts[2 i]], column j at [len - 1 - j], with
// len = |result_lengths[i]|; starts[2 i + 2] == starts[2 i] says that both slices are empty.
struct AlignedChunk
{
    int64_t first, m;
    unsigned m_waves; // blocks of a kernel that takes one wave64 per alignment
    const gwm_overlap* overlaps; // the chunk's first record
    const uint8_t* results;
    const int64_t* starts;
    const int32_t* result_lengths;
};

// Aligns device overlaps[0..n) chunk by chunk, as include/gwhip_mapper.h states it for gwm_align_overlaps, and calls
// consume(chunk) for every chunk while its states are on the device. stage_ms[0..2] += the device time (HIP events) of
// gather, align and the consumer, summed over the chunks. `name` opens the error texts. n > 0.
// The budget (max_device_bytes) counts a chunk's working set the same way for every consumer, as
// gwm_align_bytes_needed states it -- gathered bases, state slots, the aligner's workspace, the small per-overlap
// arrays and two bytes per column for the consumer's output of the chunk. What a consumer keeps beyond the chunk (the
// CIGAR text or the segment records of the chunks before, records beyond two bytes per column, which takes windows
// of fewer than 12 bases, and the counters of a pileup, 24 B per base of the owner set) lies outside it.
void align_chunks(const char* name, const gwm_overlap* overlaps, int64_t n, const char* query_bases,
                  const int64_t* query_offsets, int32_t n_queries, uint32_t first_query_read_id,
                  const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                  uint32_t first_target_read_id, int64_t max_device_bytes, hipStream_t s, float* stage_ms,
                  const std::function<void(const AlignedChunk&)>& consume);

} // namespace gwm

namespace
{

using gwm::AlignedChunk;

constexpr unsigned kWavesPerBlock = kThreads / 64;

inline void exclusive_sum(const int64_t* in, int64_t* out, int64_t n, Temp& t, hipStream_t s)
{
    size_t bytes = 0;
    GWM_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, int64_t(0), static_cast<size_t>(n), rocprim::plus<int64_t>(), s));
    GWM_CHECK(rocprim::exclusive_scan(t.get(bytes), bytes, in, out, int64_t(0), static_cast<size_t>(n),
                                      rocprim::plus<int64_t>(), s));
}

template <typename T>
void grow(dbuf<T>& b, int64_t n)
{
    if (n > b.n)
        b.resize(n);
}

} // namespace

#endif
