// gwm_align_chunks.hpp -- the chunk loop that gwm_align_overlaps (gwm_align.hip), gwm_window_segments
// (gwm_segments.hip), gwm_overlap_pileup (gwm_pileup.hip) and gwm_overlap_variants (gwm_variants.hip) share:
// validation of the overlap records, sizing on the host, and per chunk of consecutive overlaps the gather of the
// slices, the aligner (gwhip_hirschberg_myers of libgwhip.so, or gwhip_affine_align / gwhip_affine2_align of
// libgwaffine.so when the call names a scoring) and the per-chunk buffers. What is done with the chunk's alignment
// states is the caller's: align_chunks() hands them to a consumer while they are on the device. The loop and its
// kernels are defined once, in gwm_align.hip. Here as well: the check of the arguments every such entry point takes,
// and ChunkedOutput, the bookkeeping of a consumer that writes a variable number of items per alignment (CIGAR bytes,
// segment records, insertion-run records). How a consumer's kernel reads the states is in gwm_column_walk.hpp.
#ifndef GWM_ALIGN_CHUNKS_HPP
#define GWM_ALIGN_CHUNKS_HPP

#include "gwhip_mapper.h"

#include "gwm_device_utils.hpp"

#include <deque>
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

// How a call's slices are aligned. pieces 0: unit costs, the default aligner. pieces 1 / 2: the affine-gap aligner
// (include/gwhip_affine.h) under one-piece / two-piece gap costs inside `costs.band`; with one piece gap_open2 and
// gap_extend2 are not read.
struct Scoring
{
    int32_t pieces = 0;
    gwm_scoring2 costs{};
};

inline Scoring scoring_of(const gwm_scoring* s)
{
    return s == nullptr ? Scoring{} : Scoring{1, gwm_scoring2{s->mismatch, s->gap_open, s->gap_extend, 0, 0, s->band}};
}

inline Scoring scoring_of(const gwm_scoring2* s) { return s == nullptr ? Scoring{} : Scoring{2, *s}; }

// Aligns device overlaps[0..n) of the device read sets q and t chunk by chunk, as include/gwhip_mapper.h states it for
// gwm_align_overlaps, and calls consume(chunk) for every chunk while its states are on the device. stage_ms[0..2] +=
// the device time (HIP events) of gather, align and the consumer, summed over the chunks. `name` opens the error
// texts. n > 0.
// The budget (max_device_bytes) counts a chunk's working set the same way for every consumer, as
// gwm_align_bytes_needed states it -- gathered bases, state slots, the aligner's workspace, the small per-overlap
// arrays and two bytes per column for the consumer's output of the chunk. What a consumer keeps beyond the chunk (the
// CIGAR text or the segment records of the chunks before, records beyond two bytes per column, which takes windows
// of fewer than 12 bases, the counters of a pileup, 24 B per base of the owner set, and the insertion-run records of the
// variant caller, 24 B each) lies outside it.
// With a scoring of one or two pieces the affine-gap aligner writes the same results / result_lengths buffers, and
// gwhip_affine_workspace_bytes is what the budget counts for both (the two-piece aligner never needs more); a scoring
// out of range is refused before anything is launched.
// With `anchors` (none: everything above as it stands) every overlap is cut at anchors of its chain and aligned piece
// by piece, as include/gwhip_mapper.h states it for gwm_align_overlaps_anchored: the plan of the call's pieces is made
// before the chunk loop (gwm_anchored.hpp), a chunk still holds whole records, its gather and its one aligner call run
// over its pieces, and a stitch kernel leaves the records' states where the consumer reads them, so that a consumer
// sees no difference. The chunk's budget then counts the pieces' workspace, their state slots and their starts and
// result lengths besides; the stitch is timed with the aligner.
void align_chunks(const char* name, const gwm_overlap* overlaps, int64_t n, const ReadSet& q, const ReadSet& t,
                  int64_t max_device_bytes, const Scoring& scoring, hipStream_t s, float* stage_ms,
                  const std::function<void(const AlignedChunk&)>& consume, const gwm_anchor_lists* anchors = nullptr);

} // namespace gwm

namespace
{

using gwm::AlignedChunk;

constexpr unsigned kWavesPerBlock = kThreads / 64;

// what every entry point over align_chunks() refuses before it looks at n: `who` opens the texts
inline void check_chunk_arguments(const std::string& who, int32_t n_queries, int32_t n_targets,
                                  int64_t max_device_bytes, int64_t n)
{
    if (n_queries < 0 || n_targets < 0)
        throw std::invalid_argument(who + ": negative number of reads");
    if (max_device_bytes < 0)
        throw std::invalid_argument(who + ": negative max_device_bytes");
    if (n >= (int64_t(1) << 31))
        throw std::invalid_argument(who + ": 2^31 overlaps or more");
}

// a scoring outside the ranges of include/gwhip_affine.h; `who` opens the text
inline void check_scoring(const std::string& who, const gwm::Scoring& scoring)
{
    const gwm_scoring2& c = scoring.costs;
    if (scoring.pieces == 0)
        return;
    if (c.mismatch < 1 || c.mismatch > 255 || c.gap_open < 0 || c.gap_open > 255 || c.gap_extend < 1 || c.gap_extend > 255 ||
        c.band < 0)
        throw std::invalid_argument(who + "scoring (mismatch " + std::to_string(c.mismatch) + ", gap_open " +
                                    std::to_string(c.gap_open) + ", gap_extend " + std::to_string(c.gap_extend) + ", band " +
                                    std::to_string(c.band) + ") outside 1..255, 0..255, 1..255, >= 0");
    if (scoring.pieces == 2 && (c.gap_open2 < 0 || c.gap_open2 > 255 || c.gap_extend2 < 1 || c.gap_extend2 > 255))
        throw std::invalid_argument(who + "scoring (gap_open2 " + std::to_string(c.gap_open2) + ", gap_extend2 " +
                                    std::to_string(c.gap_extend2) + ") outside 0..255, 1..255");
}

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

// The output of a consumer that writes counts[i] items of T for alignment i, over the chunks of a call of n overlaps:
// per chunk a counting launch, the exclusive scan of its counts, one wait for the chunk's total, the chunk's part and
// a writing launch; behind the chunks the offsets of the call and the parts in one array.
template <typename T>
struct ChunkedOutput
{
    dbuf<int64_t> counts, local_offsets; // of the call (entry n stays 0) and of the chunk
    std::deque<dbuf<T>> parts;           // one per chunk
    std::vector<int64_t> part_sizes;
    ChunkedOutput(int64_t n, hipStream_t s)
        : counts(n + 1)
    {
        GWM_CHECK(hipMemsetAsync(counts.p, 0, sizeof(int64_t) * static_cast<size_t>(n + 1), s));
    }
    // count_launch(counts of the chunk's alignments) and write_launch(their offsets within the part, the part) launch
    // the consumer's two passes on s; the second is left out for a chunk without items
    template <typename Count, typename Write>
    void add(const AlignedChunk& c, Temp& temp, hipStream_t s, Count&& count_launch, Write&& write_launch)
    {
        grow(local_offsets, c.m + 1);
        count_launch(counts.p + c.first);
        GWM_CHECK(hipGetLastError());
        exclusive_sum(counts.p + c.first, local_offsets.p, c.m + 1, temp, s); // entry m of the input is not summed
        const int64_t items = to_host(local_offsets.p + c.m, s);
        parts.emplace_back(items);
        part_sizes.push_back(items);
        if (items > 0)
        {
            write_launch(static_cast<const int64_t*>(local_offsets.p), parts.back().p);
            GWM_CHECK(hipGetLastError());
        }
    }
    // the offsets of the call and the items of its chunks in one array, a lone part as it stands; returns the number
    // of items. Queued on s, so this object outlives the caller's wait for s.
    int64_t finish(int64_t n, Temp& temp, hipStream_t s, dbuf<int64_t>& offsets, dbuf<T>& items)
    {
        offsets.resize(n + 1);
        exclusive_sum(counts.p, offsets.p, n + 1, temp, s);
        int64_t total = 0;
        for (int64_t b : part_sizes)
            total += b;
        if (parts.size() == 1)
            items.p = parts[0].release();
        else
        {
            items.resize(total);
            int64_t at = 0;
            for (size_t c = 0; c < parts.size(); at += part_sizes[c], ++c)
                if (part_sizes[c] > 0)
                    GWM_CHECK(hipMemcpyAsync(items.p + at, parts[c].p, sizeof(T) * static_cast<size_t>(part_sizes[c]),
                                             hipMemcpyDeviceToDevice, s));
        }
        return total;
    }
};

} // namespace

#endif
