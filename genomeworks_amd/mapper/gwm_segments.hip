// gwm_segments.hip -- cudamapper on gfx950: from aligned overlaps to POA windows (include/gwhip_mapper.h,
// gwm_window_segments, gwm_pair_segments and gwm_gather_sequences). gwm_window_segments runs the chunk loop of
// gwm_align_chunks.hpp with the segment writer as its consumer: where gwm_align_overlaps turns the per-column states into text, this turns them
// into one 24 B record per (overlap, window of the target read) and leaves the states where they are. Only those
// records cross to the host, where the layers of every window are chosen (gwm_windows.cpp); gwm_gather_sequences then
// cuts backbones and layers out of the resident read sets.
//
// Segments: one wave64 per alignment over tiles of 64 columns in forward column order, by the walk of
// gwm_column_walk.hpp, which gives every lane the query and target position of its column; the last aligned column's
// (window, target position, query position) is carried between tiles in wave-uniform registers. An aligned column whose window differs from the previous aligned column's
// is a head: it opens a record and closes the one before it; lane 0 closes the last one behind the tiles. A counting
// pass, an exclusive scan of the record counts, a writing pass. Forward column order is ascending target order on '+'
// and descending on '-', where the record of the r-th head goes to the r-th place from the end: records come out
// window-ascending on both strands. No LDS, no scratch. The count / scan / write bookkeeping of the two passes is
// ChunkedOutput of gwm_align_chunks.hpp.
//
// gwm_pair_segments (read correction, both reads of a pair out of one alignment) runs the same kernel a second time per
// chunk in its query role: the windows are those of the query read, whose positions ascend in forward column order on
// both strands, and the ranges of the record are those of the target positions.
#include "gwm_column_walk.hpp"
#include "gwm_gather_plan.hpp"

namespace
{

// One wave64 per alignment of the chunk (states as AlignedChunk lays them out; o: the chunk's first overlap record,
// first: its position in the call). kWrite false: counts[i] = records of alignment i and, where edit_distances is
// given, edit_distances[i] = columns that are not a match (-1: no result although a slice was not empty). kWrite true:
// the records at segments[offsets[i]].
// kQueryRole says whose windows the records describe. An aligned column has a position in the read that owns the
// windows (`own`: the target position, or in the query role the query position) and one in the read that supplies
// the layer (`other`). own / window_length is the column's window; a record's target_first / target_last are the
// smallest and largest own, its query_begin / query_end the smallest other and the largest + 1. Forward column order
// is descending target order on '-' and ascending in everything else, so own descends in the target role on '-' and
// other does in the query role on '-'. Records are placed window-ascending: the r-th head at the r-th place, from the
// end where own descends.
template <bool kWrite, bool kQueryRole>
__global__ void __launch_bounds__(kThreads) segment_kernel(const gwm_overlap* __restrict__ o,
                                                           const uint8_t* __restrict__ results,
                                                           const int64_t* __restrict__ starts,
                                                           const int32_t* __restrict__ result_lengths, int64_t m,
                                                           uint32_t first, uint32_t window_length,
                                                           int64_t* __restrict__ counts,
                                                           int32_t* __restrict__ edit_distances,
                                                           const int64_t* __restrict__ offsets,
                                                           gwm_segment* __restrict__ segments)
{
    const int64_t i     = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= m)
        return; // whole waves leave together
    const WaveAlignment w(o, results, starts, result_lengths, i);
    const bool own_down  = !kQueryRole && w.reverse, other_down = kQueryRole && w.reverse;
    const uint32_t total = kWrite ? static_cast<uint32_t>(offsets[i + 1] - offsets[i]) : 0u;
    gwm_segment* out     = kWrite ? segments + offsets[i] : nullptr;
    const uint64_t lower = (1ull << lane) - 1;
    // wave-uniform: columns walked so far that consume a query / a target base, the last aligned column, records opened
    uint32_t query_run = 0, target_run = 0;
    bool has_last   = false;
    uint32_t last_k = 0, last_own = 0, last_other = 0;
    uint32_t records = 0, edits = 0;
    for (uint32_t base = 0; base < w.len; base += 64)
    {
        const TileColumn c(w, base, lane, lower, query_run, target_run);
        query_run = c.query_run, target_run = c.target_run;
        const bool aligned        = c.valid && c.state < 2;
        const uint64_t aligned_at = __ballot(aligned);
        if (!kWrite)
            edits += static_cast<uint32_t>(__popcll(__ballot(c.valid && c.state != 0)));
        const uint32_t own   = kQueryRole ? c.q : c.t;
        const uint32_t other = kQueryRole ? c.t : c.q;
        const uint32_t k     = aligned ? own / window_length : 0u;
        // the previous aligned column: the next lower aligned lane of the tile, or the one carried in
        const uint64_t below = aligned_at & lower;
        const int from       = below ? 63 - __clzll(below) : 0;
        uint32_t pk = __shfl(k, from, 64), p_own = __shfl(own, from, 64), p_other = __shfl(other, from, 64);
        bool has_prev = true;
        if (!below)
        {
            pk = last_k, p_own = last_own, p_other = last_other;
            has_prev = has_last;
        }
        const bool head      = aligned && (!has_prev || k != pk);
        const uint64_t heads = __ballot(head);
        if (kWrite && head)
        {
            const uint32_t r = records + static_cast<uint32_t>(__popcll(heads & lower));
            if (has_prev && r >= 1 && r - 1 < total) // closes the record before it
            {
                gwm_segment& c = out[own_down ? total - r : r - 1];
                (own_down ? c.target_first : c.target_last) = p_own;
                if (other_down)
                    c.query_begin = p_other;
                else
                    c.query_end = p_other + 1;
            }
            if (r < total)
            {
                gwm_segment& c = out[own_down ? total - 1 - r : r];
                c.overlap      = first + static_cast<uint32_t>(i);
                c.window       = k;
                (own_down ? c.target_last : c.target_first) = own;
                if (other_down)
                    c.query_end = other + 1;
                else
                    c.query_begin = other;
            }
        }
        records += static_cast<uint32_t>(__popcll(heads));
        if (aligned_at)
        {
            const int last = 63 - __clzll(aligned_at);
            last_k = __shfl(k, last, 64), last_own = __shfl(own, last, 64), last_other = __shfl(other, last, 64);
            has_last = true;
        }
    }
    if (lane != 0)
        return;
    if (kWrite)
    {
        if (has_last && records >= 1 && records - 1 < total)
        {
            gwm_segment& c = out[own_down ? total - records : records - 1];
            (own_down ? c.target_first : c.target_last) = last_own;
            if (other_down)
                c.query_begin = last_other;
            else
                c.query_end = last_other + 1;
        }
    }
    else
    {
        counts[i] = records;
        if (edit_distances)
            edit_distances[i] = w.edit_distance(edits, starts, i);
    }
}

// Block b writes sequence b of the plan to out[out_starts[b] ..): lane L of a pass takes output byte L, ascending
// addresses on both sides, or descending ones on the read side when reversed -- one segment per wave either way.
__global__ void __launch_bounds__(kThreads) gather_sequences_kernel(const gwm_gather_entry* __restrict__ plan,
                                                                    const int64_t* __restrict__ out_starts, ReadSet qs,
                                                                    ReadSet ts, uint8_t* __restrict__ out)
{
    const gwm_gather_entry e = plan[blockIdx.x];
    const ReadSet& set       = e.set ? ts : qs;
    const uint8_t* src       = set.bases + set.offsets[e.read] + e.begin;
    copy_slice(out + out_starts[blockIdx.x], src, e.end - e.begin, e.reversed != 0, AsItIs{}, Complement{});
}

// The records of one role over the chunks of a call: the segment writer (record counts, their scan, the records of the
// chunk) as a consumer of align_chunks(), and what is left of it when the chunks are through.
struct RoleRecords : ChunkedOutput<gwm_segment>
{
    using ChunkedOutput::ChunkedOutput;
    // edit_distances: of the call, or nullptr to leave them alone
    template <bool kQueryRole>
    void write(const AlignedChunk& c, int32_t window_length, int32_t* edit_distances, Temp& temp, hipStream_t s)
    {
        const uint32_t first = static_cast<uint32_t>(c.first), w = static_cast<uint32_t>(window_length);
        add(
            c, temp, s,
            [&](int64_t* counts) {
                segment_kernel<false, kQueryRole><<<c.m_waves, kThreads, 0, s>>>(
                    c.overlaps, c.results, c.starts, c.result_lengths, c.m, first, w, counts,
                    edit_distances ? edit_distances + c.first : nullptr, nullptr, nullptr);
            },
            [&](const int64_t* offsets, gwm_segment* records) {
                segment_kernel<true, kQueryRole><<<c.m_waves, kThreads, 0, s>>>(
                    c.overlaps, c.results, c.starts, c.result_lengths, c.m, first, w, nullptr, nullptr, offsets, records);
            });
    }
    // into *out, queued on s
    void finish(int64_t n, Temp& temp, hipStream_t s, gwm_segments* out)
    {
        dbuf<int64_t> offsets;
        dbuf<gwm_segment> segments;
        out->n_segments      = ChunkedOutput::finish(n, temp, s, offsets, segments);
        out->n               = n;
        out->segments        = segments.release();
        out->segment_offsets = offsets.release();
    }
};

} // namespace

extern "C" {

void gwm_segments_free(gwm_segments* segments)
{
    if (!segments)
        return;
    (void)hipFree(segments->segments);
    (void)hipFree(segments->segment_offsets);
    (void)hipFree(segments->edit_distances);
    *segments = gwm_segments{};
}

int gwm_window_segments(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                        int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                        const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                        int32_t window_length, int64_t max_device_bytes, void* stream, gwm_segments* out)
{
    *out = gwm_segments{};
    try
    {
        check_chunk_arguments("gwm_window_segments", n_queries, n_targets, max_device_bytes, n);
        if (window_length < 1)
            throw std::invalid_argument("gwm_window_segments: window_length below 1");
        if (n <= 0)
            return 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        dbuf<int32_t> edit_distances(n);
        RoleRecords records(n, s);
        Temp temp;
        gwm::align_chunks("gwm_window_segments", overlaps, n,
                          read_set(query_bases, query_offsets, n_queries, first_query_read_id),
                          read_set(target_bases, target_offsets, n_targets, first_target_read_id), max_device_bytes, gwm::Scoring{}, s,
                          out->stage_ms, [&](const AlignedChunk& c) {
                              records.write<false>(c, window_length, edit_distances.p, temp, s);
                          });
        records.finish(n, temp, s, out);
        GWM_CHECK(hipStreamSynchronize(s));
        out->edit_distances = edit_distances.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        gwm_segments_free(out);
        return -1;
    }
}

int gwm_pair_segments(const gwm_overlap* pairs, int64_t n, const char* bases, const int64_t* offsets, int32_t n_reads,
                      uint32_t first_read_id, int32_t window_length, int64_t max_device_bytes, void* stream,
                      gwm_segments* target_role, gwm_segments* query_role)
{
    *target_role = *query_role = gwm_segments{};
    try
    {
        check_chunk_arguments("gwm_pair_segments", n_reads, n_reads, max_device_bytes, n);
        if (window_length < 1)
            throw std::invalid_argument("gwm_pair_segments: window_length below 1");
        if (n <= 0)
            return 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        dbuf<int32_t> edit_distances(n);
        RoleRecords of_target(n, s), of_query(n, s);
        Temp temp;
        Events ev(3);
        float role_ms[2] = {0.f, 0.f}; // the consumer's time, which align_chunks() sums for both, apart for each role
        const ReadSet r = read_set(bases, offsets, n_reads, first_read_id);
        gwm::align_chunks("gwm_pair_segments", pairs, n, r, r, max_device_bytes, gwm::Scoring{}, s, target_role->stage_ms,
                          [&](const AlignedChunk& c) {
                              ev.record(0, s);
                              of_target.write<false>(c, window_length, edit_distances.p, temp, s);
                              ev.record(1, s);
                              of_query.write<true>(c, window_length, nullptr, temp, s);
                              ev.record(2, s);
                              role_ms[0] += ev.ms(0, 1);
                              role_ms[1] += ev.ms(1, 2);
                          });
        of_target.finish(n, temp, s, target_role);
        of_query.finish(n, temp, s, query_role);
        GWM_CHECK(hipStreamSynchronize(s));
        target_role->edit_distances = edit_distances.release();
        std::copy(target_role->stage_ms, target_role->stage_ms + 2, query_role->stage_ms);
        target_role->stage_ms[2] = role_ms[0];
        query_role->stage_ms[2]  = role_ms[1];
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        gwm_segments_free(target_role);
        gwm_segments_free(query_role);
        return -1;
    }
}

int gwm_gather_sequences(const gwm_gather_entry* plan, int64_t n, const int64_t* out_starts, const char* query_bases,
                         const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
                         const int64_t* target_offsets, int32_t n_targets, char* out, int64_t out_bytes, void* stream,
                         float* gather_ms)
{
    try
    {
        if (gather_ms)
            *gather_ms = 0.f;
        if (n_queries < 0 || n_targets < 0)
            throw std::invalid_argument("gwm_gather_sequences: negative number of reads");
        if (out_bytes < 0)
            throw std::invalid_argument("gwm_gather_sequences: negative out_bytes");
        if (n <= 0)
            return 0;
        if (n >= (int64_t(1) << 31))
            throw std::invalid_argument("gwm_gather_sequences: 2^31 sequences or more");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const ReadSet q = read_set(query_bases, query_offsets, n_queries, 0);
        const ReadSet t = read_set(target_bases, target_offsets, n_targets, 0);
        validate_plan("gwm_gather_sequences", plan, n, out_starts, q, t, out_bytes, s);
        timed_launch(s, gather_ms, [&] {
            gather_sequences_kernel<<<static_cast<unsigned>(n), kThreads, 0, s>>>(plan, out_starts, q, t,
                                                                                 reinterpret_cast<uint8_t*>(out));
        });
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        return -1;
    }
}

} // extern "C"
