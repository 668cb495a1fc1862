// gwm_align.hip -- cudamapper on gfx950: the alignment of final overlaps with everything kept on the device
// (include/gwhip_mapper.h, gwm_align_overlaps). Per chunk of consecutive overlaps (the loop of gwm_align_chunks.hpp): a
// gather kernel cuts the query and target slices out of the resident read sets into the layout the default aligner
// takes (the target slice reverse-complemented with the aligner's table on '-'), gwhip_hirschberg_myers of libgwhip.so
// aligns them as it stands (or, for a call with a scoring, gwhip_affine_align or gwhip_affine2_align of libgwaffine.so,
// into the same buffers), and the CIGAR writer here, the loop's consumer, turns the per-column states into the text
// of Alignment::convert_to_cigar() and the edit distance. Neither
// the bases nor the states cross to the host; the overlap records (36 B each) are read there to size the chunks.
// A call that brings the anchors of its records (gwm_align_overlaps_anchored) gathers and aligns the pieces between
// them instead and stitches their states into the records' slots (gwm_anchored.hpp), in front of the same consumer.
//
// CIGAR text: one wave64 per alignment over
// tiles of 64 columns (the states as WaveStates of gwm_column_walk.hpp reads them) -- symbol per lane, run heads by
// comparison with the neighbouring lane, a 64-bit ballot, run lengths from the distance to the next lower set bit, the
// open run carried between tiles in wave-uniform registers; a counting pass, an exclusive scan of the byte counts, a
// writing pass (ChunkedOutput of gwm_align_chunks.hpp). No LDS, no scratch.
#include "gwm_anchored.hpp"
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

// what a chunk of an anchored call holds besides: the pieces' state slots, their slice starts and result lengths
inline int64_t pieces_bytes(int64_t pieces, int64_t bases) { return bases + kPad + (2 * pieces + 1) * 8 + pieces * 4; }

// the aligner's workspace for `pairs` pairs with slice starts hs[0 .. 2 pairs] (host): the default aligner's at
// max_query_length `capacity`, or the affine aligner's with the costs and flags that are counted with it
inline size_t aligner_workspace_bytes(int32_t scoring_pieces, int64_t pairs, const int64_t* hs, int32_t band, int32_t capacity)
{
    if (scoring_pieces == 0)
        return gwhip_hirschberg_myers_workspace_bytes(static_cast<int32_t>(pairs), hs, capacity);
    return gwhip_affine_workspace_bytes(static_cast<int32_t>(pairs), hs, band) + static_cast<size_t>(pairs) * 5 + 256;
}

} // namespace

namespace gwm
{

void align_chunks(const char* name, const gwm_overlap* overlaps, int64_t n, const ReadSet& q, const ReadSet& t,
                  int64_t max_device_bytes, const Scoring& scoring, hipStream_t s, float* stage_ms,
                  const std::function<void(const AlignedChunk&)>& consume, const gwm_anchor_lists* anchors)
{
    const gwm_scoring2& sc = scoring.costs;
    const std::string who = std::string(name) + ": ";
    check_scoring(who, scoring);
    if (anchors)
        check_anchor_lists(who, *anchors, n, s);
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
    // with anchors: the pieces of the whole call. The aligner then sees the pieces' slice starts in the place of the
    // records', and the default aligner the longest query side of a piece.
    AnchorPlan plan;
    if (anchors)
    {
        build_anchor_plan(who, overlaps, n, *anchors, s, plan);
        max_query_length = plan.longest_query_piece;
    }
    const int64_t* piece_first = anchors ? plan.host_piece_first.data() : nullptr;
    const int64_t* all_starts  = anchors ? plan.host_starts.data() : host_starts.data();
    // the aligner's pairs of overlaps [first, first + m): the overlaps themselves, or their pieces
    auto first_pair = [&](int64_t first) { return piece_first ? piece_first[first] : first; };
    auto pairs_of   = [&](int64_t first, int64_t m) { return first_pair(first + m) - first_pair(first); };
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
        return aligner_workspace_bytes(scoring.pieces, pairs_of(first, m), all_starts + 2 * first_pair(first), sc.band, capacity);
    };
    // more pairs than one aligner call takes cost more than any budget
    auto cost = [&](int64_t first, int64_t m) {
        const int64_t* hs = host_starts.data() + 2 * first;
        const int64_t bases = hs[2 * m] - hs[0];
        if (pairs_of(first, m) > kMaxChunk)
            return INT64_MAX;
        return chunk_bytes(m, bases, workspace_bytes(first, m)) + (anchors ? pieces_bytes(pairs_of(first, m), bases) : 0);
    };

    Temp temp;
    dbuf<uint8_t> sequences, results, piece_results;
    dbuf<int64_t> lengths, starts, piece_starts;
    dbuf<int32_t> result_lengths, piece_result_lengths;
    dbuf<char> workspace;
    Events ev(4);
    for (int64_t first = 0; first < n;)
    {
        if (pairs_of(first, 1) > kMaxChunk)
            throw std::invalid_argument(who + "overlap " + std::to_string(first) + " has " + std::to_string(pairs_of(first, 1)) +
                                        " pieces, more than the " + std::to_string(kMaxChunk) + " of one aligner call");
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
        const int64_t pairs   = pairs_of(first, m);
        const int64_t* hs     = all_starts + 2 * first_pair(first); // of the aligner's pairs
        const int64_t bases   = hs[2 * pairs] - hs[0];
        const size_t ws_bytes = workspace_bytes(first, m);
        const gwm_overlap* o  = overlaps + first;
        grow(sequences, bases + kPad);
        grow(results, bases + kPad);
        grow(starts, 2 * m + 1);
        grow(result_lengths, m);
        grow(workspace, static_cast<int64_t>(ws_bytes));
        if (anchors)
        {
            grow(piece_results, bases + kPad);
            grow(piece_starts, 2 * pairs + 1);
            grow(piece_result_lengths, pairs);
        }
        else
            grow(lengths, 2 * m + 1);
        // what the aligner reads and writes: the records' buffers, or the pieces'
        const int64_t* pair_starts   = anchors ? piece_starts.p : starts.p;
        uint8_t* pair_results        = anchors ? piece_results.p : results.p;
        int32_t* pair_result_lengths = anchors ? piece_result_lengths.p : result_lengths.p;

        ev.record(0, s);
        if (anchors)
        {
            exclusive_sum(plan.piece_lengths + 2 * first_pair(first), piece_starts.p, 2 * pairs + 1, temp, s);
            gather_pieces(plan, overlaps, first_pair(first), pairs, q, t, piece_starts.p, sequences.p, s);
            record_starts(plan, overlaps, first, m, piece_starts.p, starts.p, s);
        }
        else
        {
            slice_lengths_kernel<<<grid_for(m + 1), kThreads, 0, s>>>(o, m, lengths.p);
            GWM_CHECK(hipGetLastError());
            exclusive_sum(lengths.p, starts.p, 2 * m + 1, temp, s);
            gather_kernel<<<static_cast<unsigned>(2 * m), kThreads, 0, s>>>(o, q, t, starts.p, sequences.p);
            GWM_CHECK(hipGetLastError());
        }
        ev.record(1, s);
        if (scoring.pieces == 0)
        {
            gwhip_hirschberg_args a{};
            a.n_alignments     = static_cast<int32_t>(pairs);
            a.sequences        = reinterpret_cast<const char*>(sequences.p);
            a.sequence_starts  = pair_starts;
            a.max_query_length = capacity;
            a.results          = reinterpret_cast<int8_t*>(pair_results);
            a.result_lengths   = pair_result_lengths;
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
            const size_t own = gwhip_affine_workspace_bytes(static_cast<int32_t>(pairs), hs, sc.band);
            // both argument structs, field by field
            auto fill = [&](auto& a) {
                a.n_alignments         = static_cast<int32_t>(pairs);
                a.sequences            = reinterpret_cast<const char*>(sequences.p);
                a.sequence_starts      = pair_starts;
                a.sequence_starts_host = hs;
                a.mismatch             = sc.mismatch;
                a.gap_open             = sc.gap_open;
                a.gap_extend           = sc.gap_extend;
                a.band                 = sc.band;
                a.results              = reinterpret_cast<int8_t*>(pair_results);
                a.result_lengths       = pair_result_lengths;
                a.costs                = reinterpret_cast<int32_t*>(workspace.p + ((own + 255) & ~size_t(255)));
                a.optimal              = reinterpret_cast<uint8_t*>(a.costs + pairs);
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
        if (anchors)
            stitch_pieces(plan, first, m, piece_results.p, piece_starts.p, piece_result_lengths.p, results.p, starts.p,
                          result_lengths.p, s);
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
                   void* stream, gwm_cigars* out, const gwm_anchor_lists* anchors = nullptr);

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

int64_t gwm_align_bytes_needed_anchored(const int64_t* piece_starts, int32_t pieces, int32_t scoring_pieces, int32_t band,
                                        int32_t max_query_length)
{
    const int64_t bases = piece_starts[2 * pieces] - piece_starts[0];
    return chunk_bytes(1, bases, aligner_workspace_bytes(scoring_pieces, pieces, piece_starts, band, max_query_length)) +
           pieces_bytes(pieces, bases);
}

int gwm_align_overlaps_anchored(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                                int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                                const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                                const gwm_anchor_lists* anchors, int32_t scoring_pieces, const gwm_scoring2* scoring,
                                int64_t max_device_bytes, void* stream, gwm_cigars* out)
{
    gwm::Scoring how{};
    if (scoring_pieces < 0 || scoring_pieces > 2 || (scoring_pieces > 0 && scoring == nullptr))
    {
        gwm_set_error("gwm_align_overlaps_anchored: scoring_pieces outside 0..2, or pieces without a scoring");
        *out = gwm_cigars{};
        return -1;
    }
    if (scoring_pieces > 0)
        how = gwm::Scoring{scoring_pieces, *scoring};
    return align_overlaps(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id, target_bases, target_offsets,
                          n_targets, first_target_read_id, how, max_device_bytes, stream, out, anchors);
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
                   void* stream, gwm_cigars* out, const gwm_anchor_lists* anchors)
{
    *out = gwm_cigars{};
    try
    {
        check_chunk_arguments("gwm_align_overlaps", n_queries, n_targets, max_device_bytes, n);
        check_scoring("gwm_align_overlaps: ", scoring);
        if (anchors)
            gwm::check_anchor_parameters("gwm_align_overlaps: ", *anchors);
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
                          scoring, s, out->stage_ms, write_cigars, anchors);
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

// ---- extend_overlaps: the ends of overlaps moved by the affine X-drop extension (gwm_extend_overlaps) --------------------
// Per chunk of consecutive overlaps: four slices an overlap (in front of the head and behind the tail, of the query and of
// the target in the target's strand coordinates), gathered as two pairs an overlap into the layout gwhip_extend takes,
// extended in score-only mode, and the ends applied to the records in place. Neither bases nor states exist outside the
// device; the host reads the records' slice starts to size the chunks.
namespace
{

// the lengths of overlap x's four slices: head query, head target, tail query, tail target (strand coordinates)
__device__ __forceinline__ void extension_lengths(const gwm_overlap& x, const ReadSet& q, const ReadSet& t, int64_t most,
                                                  int64_t (&len)[4])
{
    const uint32_t qi = x.query_read_id - q.first_read_id, ti = x.target_read_id - t.first_read_id;
    const int64_t ql = q.offsets[qi + 1] - q.offsets[qi], tl = t.offsets[ti + 1] - t.offsets[ti];
    const int64_t before = x.target_start_position_in_read, behind = tl - x.target_end_position_in_read;
    const bool minus     = x.relative_strand == '-';
    len[0] = min(most, static_cast<int64_t>(x.query_start_position_in_read));
    len[1] = min(most, minus ? behind : before);
    len[2] = min(most, ql - x.query_end_position_in_read);
    len[3] = min(most, minus ? before : behind);
}

// lengths[4 i + s]: bases of slice s of overlap i of the chunk; lengths[4 m] = 0, so that the exclusive scan ends with the total
__global__ void __launch_bounds__(kThreads) extension_lengths_kernel(const gwm_overlap* __restrict__ o, int64_t m, ReadSet q,
                                                                     ReadSet t, int64_t most, int64_t* __restrict__ lengths)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > m)
        return;
    if (i == m)
    {
        lengths[4 * m] = 0;
        return;
    }
    int64_t len[4];
    extension_lengths(o[i], q, t, most, len);
    for (int s = 0; s < 4; ++s)
        lengths[4 * i + s] = len[s];
}

// Block b writes slice b & 3 of overlap b >> 2 to sequences[starts[b] .. starts[b + 1]). Reversal and complement are two
// switches: a head slice is read back to front, a tail slice front to back, in the strand's coordinates; on '-' the
// target's strand coordinates run against its bytes, which flips the direction and takes the complement.
__global__ void __launch_bounds__(kThreads) extension_gather_kernel(const gwm_overlap* __restrict__ o, ReadSet qs, ReadSet ts,
                                                                    const int64_t* __restrict__ starts,
                                                                    uint8_t* __restrict__ sequences)
{
    const int64_t b     = blockIdx.x;
    const gwm_overlap x = o[b >> 2];
    const bool target = (b & 1) != 0, tail = (b & 2) != 0;
    const bool minus  = target && x.relative_strand == '-';
    const ReadSet& set  = target ? ts : qs;
    const uint32_t read = (target ? x.target_read_id : x.query_read_id) - set.first_read_id;
    const int64_t at = starts[b], len = starts[b + 1] - at;
    const int64_t start = target ? x.target_start_position_in_read : x.query_start_position_in_read;
    const int64_t end   = target ? x.target_end_position_in_read : x.query_end_position_in_read;
    // the slice lies in front of `start` or behind `end` of the bytes; on '-' the head lies behind and the tail in front
    const bool in_front = tail == minus;
    const uint8_t* src  = set.bases + set.offsets[read] + (in_front ? start - len : end);
    const bool reversed = in_front; // read towards the overlap's far side: away from the overlap
    if (minus)
        copy_slice(sequences + at, src, len, reversed, Complement{}, Complement{});
    else
        copy_slice(sequences + at, src, len, reversed, AsItIs{}, AsItIs{});
}

// the ends of pairs 2 i (head) and 2 i + 1 (tail) applied to overlap i; a pair without a result moves nothing
__global__ void __launch_bounds__(kThreads) extension_apply_kernel(gwm_overlap* __restrict__ o, int64_t m,
                                                                   const int32_t* __restrict__ pair_scores,
                                                                   const int32_t* __restrict__ query_ends,
                                                                   const int32_t* __restrict__ target_ends,
                                                                   int32_t* __restrict__ extensions, int32_t* __restrict__ scores)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= m)
        return;
    gwm_overlap x = o[i];
    uint32_t moved[4];
    for (int end = 0; end < 2; ++end)
    {
        const bool has = pair_scores[2 * i + end] >= 0;
        moved[2 * end]     = has ? static_cast<uint32_t>(query_ends[2 * i + end]) : 0u;
        moved[2 * end + 1] = has ? static_cast<uint32_t>(target_ends[2 * i + end]) : 0u;
        scores[2 * i + end] = has ? pair_scores[2 * i + end] : 0;
    }
    x.query_start_position_in_read -= moved[0];
    x.query_end_position_in_read += moved[2];
    if (x.relative_strand == '-')
    {
        x.target_end_position_in_read += moved[1];
        x.target_start_position_in_read -= moved[3];
    }
    else
    {
        x.target_start_position_in_read -= moved[1];
        x.target_end_position_in_read += moved[3];
    }
    o[i] = x;
    for (int k = 0; k < 4; ++k)
        extensions[4 * i + k] = static_cast<int32_t>(moved[k]);
}

// device bytes of one chunk of m overlaps whose four slices each hold `bases` bases in all: gathered bases, slice lengths
// and starts, and scores, ends and flags of 2 m pairs
inline int64_t extension_chunk_bytes(int64_t m, int64_t bases)
{
    return bases + kPad + 2 * (4 * m + 1) * 8 + 2 * m * (3 * 4 + 1) + 5 * 256;
}

void extend_overlaps(gwm_overlap* overlaps, int64_t n, const ReadSet& q, const ReadSet& t, const gwm_extension& e,
                     int32_t max_extension, int64_t max_device_bytes, hipStream_t s, int32_t* extensions, int32_t* scores)
{
    const std::string who = "gwm_extend_overlaps: ";
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
    if (max_extension == 0)
    {
        GWM_CHECK(hipMemsetAsync(extensions, 0, sizeof(int32_t) * 4 * static_cast<size_t>(n), s));
        GWM_CHECK(hipMemsetAsync(scores, 0, sizeof(int32_t) * 2 * static_cast<size_t>(n), s));
        GWM_CHECK(hipStreamSynchronize(s));
        return;
    }
    Temp temp;
    dbuf<int64_t> lengths(4 * n + 1), starts(4 * n + 1);
    // the slice starts of the whole call on the host, for sizing only
    extension_lengths_kernel<<<grid_for(n + 1), kThreads, 0, s>>>(overlaps, n, q, t, max_extension, lengths.p);
    GWM_CHECK(hipGetLastError());
    exclusive_sum(lengths.p, starts.p, 4 * n + 1, temp, s);
    std::vector<int64_t> host_starts(static_cast<size_t>(4 * n + 1));
    GWM_CHECK(hipMemcpyAsync(host_starts.data(), starts.p, sizeof(int64_t) * host_starts.size(), hipMemcpyDeviceToHost, s));
    GWM_CHECK(hipStreamSynchronize(s));
    int64_t budget = max_device_bytes;
    if (budget == 0)
    {
        size_t free_bytes = 0, total_bytes = 0;
        GWM_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
        budget = static_cast<int64_t>(free_bytes / 2);
    }
    auto cost = [&](int64_t first, int64_t m) {
        return extension_chunk_bytes(m, host_starts[4 * (first + m)] - host_starts[4 * first]);
    };
    dbuf<uint8_t> sequences, dropped;
    dbuf<int32_t> numbers;
    for (int64_t first = 0; first < n;)
    {
        if (cost(first, 1) > budget)
            throw std::invalid_argument(who + "overlap " + std::to_string(first) + " needs " + std::to_string(cost(first, 1)) +
                                        " device bytes, max_device_bytes allows " + std::to_string(budget));
        // the longest run of overlaps from `first` within the budget: the cost grows with m, so bisection finds it
        int64_t m = 1, too_many = std::min(n - first, kMaxChunk / 2) + 1;
        while (too_many - m > 1)
        {
            const int64_t mid = m + (too_many - m) / 2;
            if (cost(first, mid) <= budget)
                m = mid;
            else
                too_many = mid;
        }
        const int64_t* hs   = host_starts.data() + 4 * first;
        const int64_t bases = hs[4 * m] - hs[0];
        gwm_overlap* o      = overlaps + first;
        grow(sequences, bases + kPad);
        grow(numbers, 3 * 2 * m);
        grow(dropped, 2 * m);
        // the chunk's own starts, from 0
        extension_lengths_kernel<<<grid_for(m + 1), kThreads, 0, s>>>(o, m, q, t, max_extension, lengths.p);
        GWM_CHECK(hipGetLastError());
        exclusive_sum(lengths.p, starts.p, 4 * m + 1, temp, s);
        extension_gather_kernel<<<static_cast<unsigned>(4 * m), kThreads, 0, s>>>(o, q, t, starts.p, sequences.p);
        GWM_CHECK(hipGetLastError());
        gwhip_extend_args a{};
        a.n_alignments         = static_cast<int32_t>(2 * m);
        a.sequences            = reinterpret_cast<const char*>(sequences.p);
        a.sequence_starts      = starts.p;
        a.sequence_starts_host = hs;
        a.match                = e.match;
        a.mismatch             = e.mismatch;
        a.gap_open             = e.gap_open;
        a.gap_extend           = e.gap_extend;
        a.band                 = e.band;
        a.xdrop                = e.xdrop;
        a.scores               = numbers.p;
        a.query_ends           = numbers.p + 2 * m;
        a.target_ends          = numbers.p + 4 * m;
        a.dropped              = dropped.p;
        if (gwhip_extend(&a, s) != 0) // score-only mode: no results, no workspace
            throw std::runtime_error(who + gwhip_affine_last_error());
        extension_apply_kernel<<<grid_for(m), kThreads, 0, s>>>(o, m, a.scores, a.query_ends, a.target_ends, extensions + 4 * first,
                                                                scores + 2 * first);
        GWM_CHECK(hipGetLastError());
        first += m;
    }
    GWM_CHECK(hipStreamSynchronize(s));
}

} // namespace

extern "C" int gwm_extend_overlaps(gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                                   int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                                   const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                                   const gwm_extension* extension, int32_t max_extension, int64_t max_device_bytes, void* stream,
                                   int32_t* extensions, int32_t* scores)
{
    try
    {
        check_chunk_arguments("gwm_extend_overlaps", n_queries, n_targets, max_device_bytes, n);
        if (extension == nullptr)
            throw std::invalid_argument("gwm_extend_overlaps: no extension parameters");
        const gwm_extension& e = *extension;
        if (e.match < 1 || e.mismatch < 0 || int64_t(e.match) + e.mismatch > 127 || e.gap_open < 0 || e.gap_open > 127 ||
            e.gap_extend < 1 || e.match + 2 * int64_t(e.gap_extend) > 255 || e.band < 0 || e.band > GWHIP_EXTEND_MAX_BAND ||
            e.xdrop < -1 || e.xdrop > GWHIP_EXTEND_MAX_XDROP)
            throw std::invalid_argument("gwm_extend_overlaps: extension (match " + std::to_string(e.match) + ", mismatch " +
                                        std::to_string(e.mismatch) + ", gap_open " + std::to_string(e.gap_open) + ", gap_extend " +
                                        std::to_string(e.gap_extend) + ", band " + std::to_string(e.band) + ", xdrop " +
                                        std::to_string(e.xdrop) + ") out of the ranges of gwhip_extend");
        if (max_extension < 0 || max_extension > (1 << 19))
            throw std::invalid_argument("gwm_extend_overlaps: max_extension " + std::to_string(max_extension) + " outside 0..2^19");
        if (n <= 0)
            return 0;
        if (overlaps == nullptr || extensions == nullptr || scores == nullptr)
            throw std::invalid_argument("gwm_extend_overlaps: a null pointer among the arguments");
        extend_overlaps(overlaps, n, read_set(query_bases, query_offsets, n_queries, first_query_read_id),
                        read_set(target_bases, target_offsets, n_targets, first_target_read_id), e, max_extension,
                        max_device_bytes, static_cast<hipStream_t>(stream), extensions, scores);
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        return -1;
    }
}
