// gwm_align.hip -- cudamapper on gfx950: the alignment of final overlaps with everything kept on the device
// (include/gwhip_mapper.h, gwm_align_overlaps). Per chunk of consecutive overlaps (the loop of gwm_align_chunks.hpp): a
// gather kernel cuts the query and target slices out of the resident read sets into the layout the default aligner
// takes (the target slice reverse-complemented with the aligner's table on '-'), gwhip_hirschberg_myers of libgwhip.so
// aligns them as it stands (or, for a call with a scoring, gwhip_affine_align or gwhip_affine2_align of libgwaffine.so,
// into the same buffers), and the CIGAR writer here, the loop's consumer, turns the per-column states into the text
// of Alignment::convert_to_cigar() and the edit distance. Neither
// the bases nor the states cross to the host; the overlap records (36 B each) are read there to size the chunks.
//
// CIGAR text: one wave64 per alignment over
// tiles of 64 columns (the states as WaveStates of gwm_column_walk.hpp reads them) -- symbol per lane, run heads by
// comparison with the neighbouring lane, a 64-bit ballot, run lengths from the distance to the next lower set bit, the
// open run carried between tiles in wave-uniform registers; a counting pass, an exclusive scan of the byte counts, a
// writing pass (ChunkedOutput of gwm_align_chunks.hpp). No LDS, no scratch.
#include "gwm_column_walk.hpp"

#include "gwhip.h"
#include "gwhip_affine.h"

namespace
{

constexpr int64_t kPad      = 64;      // bytes behind the gathered bases and the state slots (the host aligner pads 16)
constexpr int64_t kMaxChunk = 1 << 20; // alignments per aligner call

// bad[0] |= 1: a read id outside its read set; |= 2: an end beyond its read; |= 4: a start behind its end
__global__ void __launch_bounds__(kThreads) align_validate_kernel(const gwm_overlap* __restrict__ o, int64_t n, ReadSet q,
                                                                  ReadSet t, uint32_t* __restrict__ bad)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const gwm_overlap x = o[i];
    const uint32_t qi   = x.query_read_id - q.first_read_id;
    const uint32_t ti   = x.target_read_id - t.first_read_id;
    if (x.query_read_id < q.first_read_id || qi >= q.n_reads || x.target_read_id < t.first_read_id || ti >= t.n_reads)
    {
        atomicOr(bad, 1u);
        return;
    }
    if (x.query_start_position_in_read > x.query_end_position_in_read ||
        x.target_start_position_in_read > x.target_end_position_in_read)
    {
        atomicOr(bad, 4u);
        return;
    }
    const uint64_t ql = static_cast<uint64_t>(q.offsets[qi + 1] - q.offsets[qi]);
    const uint64_t tl = static_cast<uint64_t>(t.offsets[ti + 1] - t.offsets[ti]);
    if (x.query_end_position_in_read > ql || x.target_end_position_in_read > tl)
        atomicOr(bad, 2u);
}

// lengths[2 i] / [2 i + 1]: bases of the query / target slice of overlap i of the chunk; lengths[2 m] = 0, so that the
// exclusive scan over 2 m + 1 entries ends with the total.
__global__ void __launch_bounds__(kThreads) slice_lengths_kernel(const gwm_overlap* __restrict__ o, int64_t m,
                                                                 int64_t* __restrict__ lengths)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > m)
        return;
    if (i == m)
    {
        lengths[2 * m] = 0;
        return;
    }
    lengths[2 * i]     = o[i].query_end_position_in_read - o[i].query_start_position_in_read;
    lengths[2 * i + 1] = o[i].target_end_position_in_read - o[i].target_start_position_in_read;
}

// Block b writes slice b of the chunk (even: the query slice of overlap b / 2, odd: its target slice, forward target
// coordinates) to sequences[starts[b] .. starts[b + 1]). A '-' target slice is written back to front through the
// aligner's complement table, "TGAC"[(c >> 1) & 3] for every byte (copy_slice of gwm_device_utils.hpp).
__global__ void __launch_bounds__(kThreads) gather_kernel(const gwm_overlap* __restrict__ o, ReadSet qs, ReadSet ts,
                                                          const int64_t* __restrict__ starts,
                                                          uint8_t* __restrict__ sequences)
{
    const int64_t b     = blockIdx.x;
    const gwm_overlap x = o[b >> 1];
    const bool target   = (b & 1) != 0;
    const ReadSet& set  = target ? ts : qs;
    const uint32_t read = (target ? x.target_read_id : x.query_read_id) - set.first_read_id;
    const uint32_t from = target ? x.target_start_position_in_read : x.query_start_position_in_read;
    const uint8_t* src  = set.bases + set.offsets[read] + from;
    const int64_t at    = starts[b];
    copy_slice(sequences + at, src, starts[b + 1] - at, target && x.relative_strand == '-', AsItIs{}, Complement{});
}

__device__ inline uint32_t decimal_digits(uint32_t v)
{
    uint32_t d = 1;
    for (uint32_t limit = 10; d < 10 && v >= limit; limit *= 10)
        ++d;
    return d;
}

// "<length><op>" at p; op: 0 -> M (match and mismatch), 2 -> I, 3 -> D, as cudaaligner names the states
__device__ inline void write_run(char* p, uint32_t length, uint32_t digits, uint32_t op)
{
    p[digits] = op == 0 ? 'M' : op == 2 ? 'I' : 'D';
    for (uint32_t k = digits; k-- > 0; length /= 10)
        p[k] = static_cast<char>('0' + length % 10);
}

// One wave64 per alignment of the chunk. The states of alignment i lie back to front at results[starts[2 i]], column j
// at [len - 1 - j]. kWrite false: text_bytes[i] = bytes of its CIGAR, edit_distances[i] = columns that are not a match
// (-1: no result although a slice was not empty). kWrite true: the CIGAR itself at text[text_offsets[i]].
template <bool kWrite>
__global__ void __launch_bounds__(kThreads) cigar_kernel(const uint8_t* __restrict__ results,
                                                         const int64_t* __restrict__ starts,
                                                         const int32_t* __restrict__ result_lengths, int64_t m,
                                                         int64_t* __restrict__ text_bytes,
                                                         int32_t* __restrict__ edit_distances,
                                                         const int64_t* __restrict__ text_offsets,
                                                         char* __restrict__ text)
{
    const int64_t i     = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= m)
        return; // whole waves leave together
    const WaveStates w(results, starts, result_lengths, i);
    char* out = kWrite ? text + text_offsets[i] : nullptr;
    uint32_t open_op = 0xffu, open_len = 0; // the run that is still open behind the tiles walked so far (wave-uniform)
    uint32_t written = 0, edits = 0;        // wave-uniform
    uint32_t bytes   = 0;                   // per lane
    for (uint32_t base = 0; base < w.len; base += 64)
    {
        const uint32_t columns = min(64u, w.len - base);
        const bool valid       = lane < columns;
        const uint32_t state   = w.state(base, lane, valid);
        const uint32_t op      = state < 2 ? 0u : state;
        uint32_t before        = __shfl_up(op, 1, 64);
        if (lane == 0)
            before = open_op;
        const bool head      = valid && op != before;
        const uint64_t heads = __ballot(head);
        edits += static_cast<uint32_t>(__popcll(__ballot(valid && state != 0)));
        // a head closes the run in front of it: it began at the next lower head of the tile, or it is the open run
        uint32_t closed = 0;
        if (head)
        {
            const uint64_t lower = heads & ((1ull << lane) - 1);
            closed               = lower ? lane - (63u - static_cast<uint32_t>(__clzll(lower))) : open_len + lane;
        }
        const uint32_t digits = decimal_digits(closed);
        const uint32_t size   = closed ? digits + 1 : 0u;
        if (kWrite)
        {
            uint32_t end = size; // inclusive scan over the lanes
            for (uint32_t d = 1; d < 64; d <<= 1)
            {
                const uint32_t v = __shfl_up(end, d, 64);
                if (lane >= d)
                    end += v;
            }
            if (closed)
                write_run(out + written + end - size, closed, digits, before);
            written += __shfl(end, 63, 64);
        }
        else
            bytes += size;
        if (heads)
        {
            const uint32_t last = 63u - static_cast<uint32_t>(__clzll(heads));
            open_len            = columns - last;
            open_op             = __shfl(op, static_cast<int>(last), 64);
        }
        else
            open_len += columns;
    }
    if (kWrite)
    {
        if (lane == 0 && open_len)
            write_run(out + written, open_len, decimal_digits(open_len), open_op);
    }
    else
    {
        for (int d = 32; d > 0; d >>= 1)
            bytes += __shfl_xor(bytes, d, 64);
        if (lane == 0)
        {
            text_bytes[i]     = bytes + (open_len ? decimal_digits(open_len) + 1 : 0u);
            edit_distances[i] = w.edit_distance(edits, starts, i);
        }
    }
}

// Device bytes of one chunk of m alignments whose slices hold `bases` bases: gathered bases, state slots, slice lengths and
// starts, result lengths, CIGAR byte counts and offsets, the aligner's workspace, and the text at its upper bound of two
// bytes per column (runs of one column).
inline int64_t chunk_bytes(int64_t m, int64_t bases, size_t workspace)
{
    return 2 * (bases + kPad) + 2 * (2 * m + 1) * 8 + m * 4 + 2 * (m + 1) * 8 + static_cast<int64_t>(workspace) + 2 * bases;
}

} // namespace

namespace gwm
{

void align_chunks(const char* name, const gwm_overlap* overlaps, int64_t n, const ReadSet& q, const ReadSet& t,
                  int64_t max_device_bytes, const Scoring& scoring, hipStream_t s, float* stage_ms,
                  const std::function<void(const AlignedChunk&)>& consume)
{
    const gwm_scoring2& sc = scoring.costs;
    const std::string who = std::string(name) + ": ";
    check_scoring(who, scoring);
    {
        dbuf<uint32_t> bad(1);
        GWM_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
        align_validate_kernel<<<grid_for(n), kThreads, 0, s>>>(overlaps, n, q, t, bad.p);
        GWM_CHECK(hipGetLastError());
        const uint32_t what = to_host(bad.p, s);
        if (what & 1u)
            throw std::invalid_argument(who + "an overlap names a read outside the read set");
        if (what & 4u)
            throw std::invalid_argument(who + "an overlap starts behind its end");
        if (what & 2u)
            throw std::invalid_argument(who + "an overlap lies beyond the end of its read");
    }
    // the records on the host, for sizing only: slice starts of the whole call and the longest query slice
    std::vector<gwm_overlap> records(static_cast<size_t>(n));
    GWM_CHECK(hipMemcpyAsync(records.data(), overlaps, sizeof(gwm_overlap) * records.size(), hipMemcpyDeviceToHost, s));
    GWM_CHECK(hipStreamSynchronize(s));
    std::vector<int64_t> host_starts(2 * records.size() + 1, 0);
    int64_t max_query_length = 0;
    for (size_t i = 0; i < records.size(); ++i)
    {
        const int64_t ql       = records[i].query_end_position_in_read - records[i].query_start_position_in_read;
        const int64_t tl       = records[i].target_end_position_in_read - records[i].target_start_position_in_read;
        host_starts[2 * i + 1] = host_starts[2 * i] + ql;
        host_starts[2 * i + 2] = host_starts[2 * i + 1] + tl;
        max_query_length       = std::max(max_query_length, ql);
    }
    if (max_query_length > INT32_MAX)
        throw std::invalid_argument(who + "a query slice of 2^31 bases or more");
    const int32_t capacity = static_cast<int32_t>(max_query_length);
    int64_t budget         = max_device_bytes;
    if (budget == 0)
    {
        size_t free_bytes = 0, total_bytes = 0;
        GWM_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
        budget = static_cast<int64_t>(free_bytes / 2);
    }
    // the aligner's workspace for overlaps [first, first + m); the affine aligner's costs and flags are counted with it
    auto workspace_bytes = [&](int64_t first, int64_t m) -> size_t {
        const int64_t* hs = host_starts.data() + 2 * first;
        if (scoring.pieces == 0)
            return gwhip_hirschberg_myers_workspace_bytes(static_cast<int32_t>(m), hs, capacity);
        return gwhip_affine_workspace_bytes(static_cast<int32_t>(m), hs, sc.band) + static_cast<size_t>(m) * 5 + 256;
    };
    auto cost = [&](int64_t first, int64_t m) {
        const int64_t* hs = host_starts.data() + 2 * first;
        return chunk_bytes(m, hs[2 * m] - hs[0], workspace_bytes(first, m));
    };

    Temp temp;
    dbuf<uint8_t> sequences, results;
    dbuf<int64_t> lengths, starts;
    dbuf<int32_t> result_lengths;
    dbuf<char> workspace;
    Events ev(4);
    for (int64_t first = 0; first < n;)
    {
        if (cost(first, 1) > budget)
            throw std::invalid_argument(who + "overlap " + std::to_string(first) + " needs " +
                                        std::to_string(cost(first, 1)) + " device bytes, max_device_bytes allows " +
                                        std::to_string(budget));
        // the longest run of overlaps from `first` that doubling and then bisection find within the budget
        const int64_t most = std::min(n - first, kMaxChunk);
        int64_t m = 1, too_many = most + 1;
        while (m < most && too_many > most)
        {
            const int64_t twice = std::min(2 * m, most);
            if (cost(first, twice) <= budget)
                m = twice;
            else
                too_many = twice;
        }
        while (too_many - m > 1)
        {
            const int64_t mid = m + (too_many - m) / 2;
            if (cost(first, mid) <= budget)
                m = mid;
            else
                too_many = mid;
        }
        const int64_t* hs     = host_starts.data() + 2 * first;
        const int64_t bases   = hs[2 * m] - hs[0];
        const size_t ws_bytes = workspace_bytes(first, m);
        const gwm_overlap* o  = overlaps + first;
        grow(sequences, bases + kPad);
        grow(results, bases + kPad);
        grow(lengths, 2 * m + 1);
        grow(starts, 2 * m + 1);
        grow(result_lengths, m);
        grow(workspace, static_cast<int64_t>(ws_bytes));

        ev.record(0, s);
        slice_lengths_kernel<<<grid_for(m + 1), kThreads, 0, s>>>(o, m, lengths.p);
        GWM_CHECK(hipGetLastError());
        exclusive_sum(lengths.p, starts.p, 2 * m + 1, temp, s);
        gather_kernel<<<static_cast<unsigned>(2 * m), kThreads, 0, s>>>(o, q, t, starts.p, sequences.p);
        GWM_CHECK(hipGetLastError());
        ev.record(1, s);
        if (scoring.pieces == 0)
        {
            gwhip_hirschberg_args a{};
            a.n_alignments     = static_cast<int32_t>(m);
            a.sequences        = reinterpret_cast<const char*>(sequences.p);
            a.sequence_starts  = starts.p;
            a.max_query_length = capacity;
            a.results          = reinterpret_cast<int8_t*>(results.p);
            a.result_lengths   = result_lengths.p;
            a.workspace        = workspace.p;
            a.workspace_bytes  = ws_bytes;
            if (gwhip_hirschberg_myers(&a, s) != 0)
            {
                char text[512] = "";
                gwhip_last_error_string(text, sizeof(text));
                throw std::runtime_error(who + text);
            }
        }
        else
        {
            // costs and flags, which no consumer reads, lie behind the aligner's own workspace
            const size_t own = gwhip_affine_workspace_bytes(static_cast<int32_t>(m), hs, sc.band);
            // both argument structs, field by field
            auto fill = [&](auto& a) {
                a.n_alignments         = static_cast<int32_t>(m);
                a.sequences            = reinterpret_cast<const char*>(sequences.p);
                a.sequence_starts      = starts.p;
                a.sequence_starts_host = hs;
                a.mismatch             = sc.mismatch;
                a.gap_open             = sc.gap_open;
                a.gap_extend           = sc.gap_extend;
                a.band                 = sc.band;
                a.results              = reinterpret_cast<int8_t*>(results.p);
                a.result_lengths       = result_lengths.p;
                a.costs                = reinterpret_cast<int32_t*>(workspace.p + ((own + 255) & ~size_t(255)));
                a.optimal              = reinterpret_cast<uint8_t*>(a.costs + m);
                a.workspace            = workspace.p;
                a.workspace_bytes      = own;
            };
            int status = 0;
            if (scoring.pieces == 1)
            {
                gwhip_affine_args a{};
                fill(a);
                status = gwhip_affine_align(&a, s);
            }
            else
            {
                gwhip_affine2_args a{};
                fill(a);
                a.gap_open2   = sc.gap_open2;
                a.gap_extend2 = sc.gap_extend2;
                status        = gwhip_affine2_align(&a, s);
            }
            if (status != 0)
                throw std::runtime_error(who + gwhip_affine_last_error());
        }
        ev.record(2, s);
        consume(AlignedChunk{first, m, static_cast<unsigned>((m + kWavesPerBlock - 1) / kWavesPerBlock), o, results.p,
                             starts.p, result_lengths.p});
        ev.record(3, s);
        for (int k = 0; k < 3; ++k)
            stage_ms[k] += ev.ms(k, k + 1);
        first += m;
    }
}

} // namespace gwm

namespace
{

int align_overlaps(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                   int32_t n_queries, uint32_t first_query_read_id, const char* target_bases, const int64_t* target_offsets,
                   int32_t n_targets, uint32_t first_target_read_id, const gwm::Scoring& scoring, int64_t max_device_bytes,
                   void* stream, gwm_cigars* out);

} // namespace

extern "C" {

int64_t gwm_align_bytes_needed(int32_t query_length, int32_t target_length, int32_t max_query_length)
{
    const int64_t starts[3] = {0, query_length, static_cast<int64_t>(query_length) + target_length};
    return chunk_bytes(1, starts[2], gwhip_hirschberg_myers_workspace_bytes(1, starts, max_query_length));
}

int64_t gwm_align_bytes_needed_scored(int32_t query_length, int32_t target_length, int32_t band)
{
    const int64_t starts[3] = {0, query_length, static_cast<int64_t>(query_length) + target_length};
    return chunk_bytes(1, starts[2], gwhip_affine_workspace_bytes(1, starts, band) + 5 + 256);
}

void gwm_cigars_free(gwm_cigars* cigars)
{
    if (!cigars)
        return;
    (void)hipFree(cigars->text);
    (void)hipFree(cigars->cigar_offsets);
    (void)hipFree(cigars->edit_distances);
    *cigars = gwm_cigars{};
}

int gwm_align_overlaps(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                       int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                       const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                       int64_t max_device_bytes, void* stream, gwm_cigars* out)
{
    return gwm_align_overlaps_scored(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id, target_bases,
                                     target_offsets, n_targets, first_target_read_id, nullptr, max_device_bytes, stream, out);
}

int gwm_align_overlaps_scored2(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                               int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                               const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                               const gwm_scoring2* scoring, int64_t max_device_bytes, void* stream, gwm_cigars* out)
{
    return align_overlaps(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id, target_bases, target_offsets,
                          n_targets, first_target_read_id, gwm::scoring_of(scoring), max_device_bytes, stream, out);
}

int gwm_align_overlaps_scored(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                              int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                              const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                              const gwm_scoring* scoring, int64_t max_device_bytes, void* stream, gwm_cigars* out)
{
    return align_overlaps(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id, target_bases, target_offsets,
                          n_targets, first_target_read_id, gwm::scoring_of(scoring), max_device_bytes, stream, out);
}

} // extern "C"

namespace
{

int align_overlaps(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                   int32_t n_queries, uint32_t first_query_read_id, const char* target_bases, const int64_t* target_offsets,
                   int32_t n_targets, uint32_t first_target_read_id, const gwm::Scoring& scoring, int64_t max_device_bytes,
                   void* stream, gwm_cigars* out)
{
    *out = gwm_cigars{};
    try
    {
        check_chunk_arguments("gwm_align_overlaps", n_queries, n_targets, max_device_bytes, n);
        check_scoring("gwm_align_overlaps: ", scoring);
        if (n <= 0)
            return 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        dbuf<int32_t> edit_distances(n);
        ChunkedOutput<char> cigars(n, s);
        Temp temp;
        // the CIGAR writer: byte counts, then the text of the chunk
        auto write_cigars = [&](const AlignedChunk& c) {
            cigars.add(
                c, temp, s,
                [&](int64_t* text_bytes) {
                    cigar_kernel<false><<<c.m_waves, kThreads, 0, s>>>(c.results, c.starts, c.result_lengths, c.m,
                                                                      text_bytes, edit_distances.p + c.first, nullptr,
                                                                      nullptr);
                },
                [&](const int64_t* text_offsets, char* text) {
                    cigar_kernel<true><<<c.m_waves, kThreads, 0, s>>>(c.results, c.starts, c.result_lengths, c.m, nullptr,
                                                                     nullptr, text_offsets, text);
                });
        };
        gwm::align_chunks("gwm_align_overlaps", overlaps, n,
                          read_set(query_bases, query_offsets, n_queries, first_query_read_id),
                          read_set(target_bases, target_offsets, n_targets, first_target_read_id), max_device_bytes,
                          scoring, s, out->stage_ms, write_cigars);
        dbuf<int64_t> offsets;
        dbuf<char> text;
        const int64_t total = cigars.finish(n, temp, s, offsets, text);
        GWM_CHECK(hipStreamSynchronize(s));
        out->n              = n;
        out->text_bytes     = total;
        out->text           = text.release();
        out->cigar_offsets  = offsets.release();
        out->edit_distances = edit_distances.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        *out = gwm_cigars{};
        return -1;
    }
}

} // namespace
