// gwm_anchored.hip -- cudamapper on gfx950: overlaps cut at anchors of their chain and aligned piece by piece
// (include/gwhip_mapper.h, gwm_align_overlaps_anchored; rules G1-G6 are gwm_anchor_plan.hpp, DESIGN.md section 3.12 has
// the layout). Three parts, all called from the chunk loop of gwm_align.hip:
//   the plan of the whole call -- one thread an anchor: slice coordinates and the valid flag, a scan and a scatter
//     that leave the valid anchors back to back, the order check and the cut flag against the neighbour, a scan of
//     the cuts, and the piece table (u, v, record, lengths) from it;
//   the gather of a chunk's pieces, one wave64 a slice;
//   the stitch, one wave64 a record: the lengths of its pieces' states are scanned from the last piece, 64 pieces at
//     a time across the lanes, and the bytes copied coalesced, in dwords where source and destination share their
//     alignment, into the record's slot. No LDS, no scratch; every store is guarded by the slot.
#include "gwm_anchored.hpp"

#include "gwm_align_chunks.hpp"
#include "gwm_anchor_plan.hpp"

namespace
{

__device__ __forceinline__ gwm_plan::Record record_of(const gwm_overlap& x)
{
    return {static_cast<int64_t>(x.query_start_position_in_read), static_cast<int64_t>(x.query_end_position_in_read),
            static_cast<int64_t>(x.target_start_position_in_read), static_cast<int64_t>(x.target_end_position_in_read),
            x.relative_strand == '-'};
}

// G1, G2. Anchor a < n_anchors belongs to the record r with offsets[r] <= a < offsets[r + 1]: coordinates[3 a ..] =
// u, v, r and valid[a] where it is valid (u and v then fit 32 bits); valid[n_anchors] = 0 ends the scan.
__global__ void __launch_bounds__(kThreads) anchor_coordinates_kernel(const gwm_overlap* __restrict__ o,
                                                                      const int64_t* __restrict__ offsets, int64_t n,
                                                                      const uint32_t* __restrict__ positions,
                                                                      int64_t n_anchors, int64_t k,
                                                                      uint32_t* __restrict__ coordinates,
                                                                      int64_t* __restrict__ valid)
{
    const int64_t a = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a > n_anchors)
        return;
    if (a == n_anchors)
    {
        valid[a] = 0;
        return;
    }
    int64_t lo = 0, hi = n; // the last r in [0, n) with offsets[r] <= a: offsets[0] = 0 <= a < offsets[n]
    while (hi - lo > 1)
    {
        const int64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= a)
            lo = mid;
        else
            hi = mid;
    }
    const gwm_plan::Record r = record_of(o[lo]);
    int64_t u, v;
    gwm_plan::slice_coordinates(r, k, positions[2 * a], positions[2 * a + 1], u, v);
    const bool ok = gwm_plan::valid(u, v, gwm_plan::query_length(r), gwm_plan::target_length(r));
    valid[a]      = ok ? 1 : 0;
    coordinates[3 * a]     = static_cast<uint32_t>(u);
    coordinates[3 * a + 1] = static_cast<uint32_t>(v);
    coordinates[3 * a + 2] = static_cast<uint32_t>(lo);
}

// the valid anchors back to back, in order: packed[3 at[a] ..] = coordinates[3 a ..]
__global__ void __launch_bounds__(kThreads) anchor_pack_kernel(const uint32_t* __restrict__ coordinates,
                                                               const int64_t* __restrict__ valid,
                                                               const int64_t* __restrict__ at, int64_t n_anchors,
                                                               uint32_t* __restrict__ packed)
{
    const int64_t a = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a >= n_anchors || !valid[a])
        return;
    for (int f = 0; f < 3; ++f)
        packed[3 * at[a] + f] = coordinates[3 * a + f];
}

// G3, G4 over the n_valid packed anchors: cut[c] the head flag, cut[n_valid] = 0; *bad_record = the smallest record
// with a valid anchor that does not lie behind the valid anchor before it in both u and v
__global__ void __launch_bounds__(kThreads) anchor_cut_kernel(const uint32_t* __restrict__ packed, int64_t n_valid,
                                                              int64_t spacing, int64_t* __restrict__ cut,
                                                              uint32_t* __restrict__ bad_record)
{
    const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c > n_valid)
        return;
    if (c == n_valid)
    {
        cut[c] = 0;
        return;
    }
    const int64_t u = packed[3 * c], v = packed[3 * c + 1];
    const uint32_t r = packed[3 * c + 2];
    const bool first = c == 0 || packed[3 * (c - 1) + 2] != r;
    const int64_t u_before = first ? 0 : packed[3 * (c - 1)], v_before = first ? 0 : packed[3 * (c - 1) + 1];
    if (!first && !gwm_plan::increasing(u_before, v_before, u, v))
        atomicMin(bad_record, r);
    cut[c] = gwm_plan::is_cut(first, u_before, u, spacing) ? 1 : 0;
}

// piece_first[r] = r + the cuts in front of record r's anchors, r in [0, n]: a record has one piece more than cuts
__global__ void __launch_bounds__(kThreads) piece_first_kernel(const int64_t* __restrict__ offsets, int64_t n,
                                                               const int64_t* __restrict__ at,
                                                               const int64_t* __restrict__ cuts_before,
                                                               int64_t* __restrict__ piece_first)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r <= n)
        piece_first[r] = r + cuts_before[at[offsets[r]]];
}

// G5, the starts: thread i < n opens record i's first piece at (0, 0); thread n + c the piece at cut c, which is
// piece r + 1 + cuts_before[c] of the call
__global__ void __launch_bounds__(kThreads) piece_starts_kernel(const int64_t* __restrict__ piece_first, int64_t n,
                                                                const uint32_t* __restrict__ packed,
                                                                const int64_t* __restrict__ cut,
                                                                const int64_t* __restrict__ cuts_before, int64_t n_valid,
                                                                int64_t pieces, uint32_t* __restrict__ piece_u,
                                                                uint32_t* __restrict__ piece_v,
                                                                uint32_t* __restrict__ piece_record)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    int64_t p  = -1;
    uint32_t u = 0, v = 0, r = 0;
    if (i < n)
    {
        p = piece_first[i];
        r = static_cast<uint32_t>(i);
    }
    else if (i - n < n_valid && cut[i - n])
    {
        const int64_t c = i - n;
        u = packed[3 * c];
        v = packed[3 * c + 1];
        r = packed[3 * c + 2];
        p = static_cast<int64_t>(r) + 1 + cuts_before[c];
    }
    if (p >= 0 && p < pieces)
    {
        piece_u[p]      = u;
        piece_v[p]      = v;
        piece_record[p] = r;
    }
}

// G5, the ends: a piece reaches to the next piece of its record, or to (n, m). lengths[2 pieces] = 0.
__global__ void __launch_bounds__(kThreads) piece_lengths_kernel(const gwm_overlap* __restrict__ o,
                                                                 const int64_t* __restrict__ piece_first,
                                                                 const uint32_t* __restrict__ piece_u,
                                                                 const uint32_t* __restrict__ piece_v,
                                                                 const uint32_t* __restrict__ piece_record, int64_t pieces,
                                                                 int64_t* __restrict__ lengths)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p > pieces)
        return;
    if (p == pieces)
    {
        lengths[2 * pieces] = 0;
        return;
    }
    const uint32_t r          = piece_record[p];
    const gwm_plan::Record x  = record_of(o[r]);
    const bool last           = p + 1 == piece_first[r + 1];
    const gwm_plan::Piece one = gwm_plan::piece_between(piece_u[p], piece_v[p], last ? gwm_plan::query_length(x) : piece_u[p + 1],
                                                        last ? gwm_plan::target_length(x) : piece_v[p + 1]);
    lengths[2 * p]     = one.query_length;
    lengths[2 * p + 1] = one.target_length;
}

// Wave b of the launch writes slice b of the chunk's pieces: even, the query side of piece b / 2; odd, its target
// side -- on '-' the bases [te - v - len, te - v) of the target read back to front through the complement table.
__global__ void __launch_bounds__(kThreads) piece_gather_kernel(const gwm_overlap* __restrict__ o,
                                                                const uint32_t* __restrict__ piece_u,
                                                                const uint32_t* __restrict__ piece_v,
                                                                const uint32_t* __restrict__ piece_record, int64_t slices,
                                                                ReadSet qs, ReadSet ts, const int64_t* __restrict__ starts,
                                                                uint8_t* __restrict__ sequences)
{
    const int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (b >= slices)
        return; // whole waves leave together
    const int64_t p     = b >> 1;
    const gwm_overlap x = o[piece_record[p]];
    const bool target   = (b & 1) != 0;
    const int64_t at = starts[b], len = starts[b + 1] - at;
    if (!target)
    {
        const uint8_t* src = qs.bases + qs.offsets[x.query_read_id - qs.first_read_id] + x.query_start_position_in_read + piece_u[p];
        copy_slice_wave(sequences + at, src, len, false, AsItIs{}, Complement{});
        return;
    }
    const uint8_t* read = ts.bases + ts.offsets[x.target_read_id - ts.first_read_id];
    const bool minus    = x.relative_strand == '-';
    const int64_t from  = minus ? static_cast<int64_t>(x.target_end_position_in_read) - piece_v[p] - len
                                : static_cast<int64_t>(x.target_start_position_in_read) + piece_v[p];
    copy_slice_wave(sequences + at, read + from, len, minus, AsItIs{}, Complement{});
}

// starts[2 i], starts[2 i + 1]: where the slot of record first + i of the chunk begins, and its query slice's end
__global__ void __launch_bounds__(kThreads) record_starts_kernel(const gwm_overlap* __restrict__ o,
                                                                 const int64_t* __restrict__ piece_first, int64_t m,
                                                                 const int64_t* __restrict__ piece_starts,
                                                                 int64_t* __restrict__ starts)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > m)
        return;
    const int64_t at = piece_starts[2 * (piece_first[i] - piece_first[0])];
    starts[2 * i]    = at;
    if (i < m)
        starts[2 * i + 1] = at + (o[i].query_end_position_in_read - o[i].query_start_position_in_read);
}

// The wave copies src[0 .. len) to dst[0 .. min(len, room)): in dwords between the first and the last dword boundary
// of dst where src shares dst's alignment, in bytes around them and otherwise.
__device__ __forceinline__ void copy_states(uint8_t* dst, const uint8_t* src, int64_t len, int64_t room, uint32_t lane)
{
    const int64_t n = len < room ? len : room;
    if (n <= 0)
        return;
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst), s = reinterpret_cast<uintptr_t>(src);
    if (((d ^ s) & 3u) != 0 || n < 8)
    {
        for (int64_t j = lane; j < n; j += 64)
            dst[j] = src[j];
        return;
    }
    const int64_t head = static_cast<int64_t>((4u - (d & 3u)) & 3u); // < 4 <= n
    const int64_t body = (n - head) >> 2;
    const int64_t tail = head + 4 * body;
    if (lane < head)
        dst[lane] = src[lane];
    const uint32_t* from = reinterpret_cast<const uint32_t*>(src + head);
    uint32_t* to         = reinterpret_cast<uint32_t*>(dst + head);
    for (int64_t w = lane; w < body; w += 64)
        to[w] = from[w];
    if (tail + lane < n)
        dst[tail + lane] = src[tail + lane];
}

// One wave64 per record i of the chunk, pieces [a, b) of the chunk. Piece j's states lie back to front at the front of
// its slot piece_starts[2 j]; the record's states back to front are piece b - 1's bytes, then piece b - 2's, ..., then
// piece a's, at results[starts[2 i]]. A piece without states although its slices are not both empty leaves the record
// without a result.
__global__ void __launch_bounds__(kThreads) stitch_kernel(const uint8_t* __restrict__ piece_results,
                                                          const int64_t* __restrict__ piece_starts,
                                                          const int32_t* __restrict__ piece_result_lengths,
                                                          const int64_t* __restrict__ piece_first, int64_t m,
                                                          uint8_t* __restrict__ results, const int64_t* __restrict__ starts,
                                                          int32_t* __restrict__ result_lengths)
{
    const int64_t i     = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= m)
        return; // whole waves leave together
    const int64_t a = piece_first[i] - piece_first[0], b = piece_first[i + 1] - piece_first[0];
    const int64_t slot = starts[2 * i], room = starts[2 * i + 2] - slot;
    bool failed = false;
    for (int64_t j = a + lane; j < b; j += 64)
        failed = failed || (piece_result_lengths[j] == 0 && piece_starts[2 * j + 2] > piece_starts[2 * j]);
    if (__ballot(failed) != 0)
    {
        if (lane == 0)
            result_lengths[i] = 0;
        return;
    }
    int64_t done = 0; // bytes of the pieces behind the ones in hand (wave-uniform)
    for (int64_t base = 0; base < b - a; base += 64)
    {
        const int64_t in_hand = b - a - base < 64 ? b - a - base : 64;
        const int64_t j       = b - 1 - base - lane; // from the last piece
        int32_t len           = 0;
        int64_t from          = 0;
        if (lane < in_hand)
        {
            const int32_t stored = piece_result_lengths[j];
            len                  = stored < 0 ? -stored : stored; // as the host aligner reads it
            from                 = piece_starts[2 * j];
        }
        int64_t end = len; // inclusive scan over the lanes
        for (uint32_t d = 1; d < 64; d <<= 1)
        {
            const int64_t v = __shfl_up(end, d, 64);
            if (lane >= d)
                end += v;
        }
        const int64_t to = done + end - len;
        for (int k = 0; k < static_cast<int>(in_hand); ++k)
        {
            const int64_t one_to = __shfl(to, k, 64);
            copy_states(results + slot + one_to, piece_results + __shfl(from, k, 64), __shfl(len, k, 64), room - one_to, lane);
        }
        done += __shfl(end, 63, 64);
    }
    if (lane == 0)
        result_lengths[i] = static_cast<int32_t>(done < room ? done : room);
}

template <typename T>
T* device_array(int64_t count)
{
    T* p = nullptr;
    GWM_CHECK(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * static_cast<size_t>(count > 0 ? count : 1)));
    return p;
}

} // namespace

namespace gwm
{

void check_anchor_parameters(const std::string& who, const gwm_anchor_lists& lists)
{
    if (!gwm_plan::parameters_in_range(lists.kmer_size, lists.spacing))
        throw std::invalid_argument(who + "anchor_kmer_size " + std::to_string(lists.kmer_size) + ", anchor_spacing " +
                                    std::to_string(lists.spacing) + " outside 1..32, >= 1");
    if (lists.n_anchors < 0 || lists.n_anchors >= (int64_t(1) << 32))
        throw std::invalid_argument(who + "a negative number of anchors, or 2^32 and more");
}

void check_anchor_lists(const std::string& who, const gwm_anchor_lists& lists, int64_t n, hipStream_t s)
{
    check_anchor_parameters(who, lists);
    if (lists.offsets == nullptr || (lists.n_anchors > 0 && lists.positions == nullptr))
        throw std::invalid_argument(who + "anchors without offsets or positions");
    std::vector<int64_t> offsets(static_cast<size_t>(n + 1));
    GWM_CHECK(hipMemcpyAsync(offsets.data(), lists.offsets, sizeof(int64_t) * offsets.size(), hipMemcpyDeviceToHost, s));
    GWM_CHECK(hipStreamSynchronize(s));
    const int64_t bad = gwm_plan::first_bad_offset(offsets.data(), n, lists.n_anchors);
    if (bad >= 0)
        throw std::invalid_argument(who + "anchor offsets must start at 0, never decrease and end at the number of anchors (" +
                                    std::to_string(lists.n_anchors) + "): entry " + std::to_string(bad) + " is " +
                                    std::to_string(offsets[static_cast<size_t>(bad)]));
}

void build_anchor_plan(const std::string& who, const gwm_overlap* overlaps, int64_t n, const gwm_anchor_lists& lists,
                       hipStream_t s, AnchorPlan& plan)
{
    const int64_t n_anchors = lists.n_anchors;
    Temp temp;
    dbuf<uint32_t> coordinates(3 * n_anchors), bad_record(1);
    dbuf<int64_t> valid(n_anchors + 1), at(n_anchors + 1);
    anchor_coordinates_kernel<<<grid_for(n_anchors + 1), kThreads, 0, s>>>(overlaps, lists.offsets, n, lists.positions,
                                                                          n_anchors, lists.kmer_size, coordinates.p, valid.p);
    GWM_CHECK(hipGetLastError());
    exclusive_sum(valid.p, at.p, n_anchors + 1, temp, s);
    const int64_t n_valid = to_host(at.p + n_anchors, s);
    dbuf<uint32_t> packed(3 * n_valid);
    dbuf<int64_t> cut(n_valid + 1), cuts_before(n_valid + 1);
    if (n_valid > 0)
    {
        anchor_pack_kernel<<<grid_for(n_anchors), kThreads, 0, s>>>(coordinates.p, valid.p, at.p, n_anchors, packed.p);
        GWM_CHECK(hipGetLastError());
    }
    GWM_CHECK(hipMemsetAsync(bad_record.p, 0xff, sizeof(uint32_t), s));
    anchor_cut_kernel<<<grid_for(n_valid + 1), kThreads, 0, s>>>(packed.p, n_valid, lists.spacing, cut.p, bad_record.p);
    GWM_CHECK(hipGetLastError());
    exclusive_sum(cut.p, cuts_before.p, n_valid + 1, temp, s);
    const uint32_t offender = to_host(bad_record.p, s);
    if (offender != 0xffffffffu)
        throw std::invalid_argument(who + "the anchors of overlap " + std::to_string(offender) +
                                    " are not strictly increasing in query and target");
    plan.n      = n;
    plan.pieces = n + to_host(cuts_before.p + n_valid, s);
    plan.piece_lengths = device_array<int64_t>(2 * plan.pieces + 1);
    plan.piece_u       = device_array<uint32_t>(plan.pieces);
    plan.piece_v       = device_array<uint32_t>(plan.pieces);
    plan.piece_record  = device_array<uint32_t>(plan.pieces);
    plan.piece_first   = device_array<int64_t>(n + 1);
    piece_first_kernel<<<grid_for(n + 1), kThreads, 0, s>>>(lists.offsets, n, at.p, cuts_before.p, plan.piece_first);
    GWM_CHECK(hipGetLastError());
    piece_starts_kernel<<<grid_for(n + n_valid), kThreads, 0, s>>>(plan.piece_first, n, packed.p, cut.p, cuts_before.p, n_valid,
                                                                  plan.pieces, plan.piece_u, plan.piece_v, plan.piece_record);
    GWM_CHECK(hipGetLastError());
    piece_lengths_kernel<<<grid_for(plan.pieces + 1), kThreads, 0, s>>>(overlaps, plan.piece_first, plan.piece_u, plan.piece_v,
                                                                       plan.piece_record, plan.pieces, plan.piece_lengths);
    GWM_CHECK(hipGetLastError());
    // the piece lengths come to the host once, for sizing: the slice starts of the call's pieces
    std::vector<int64_t> lengths(static_cast<size_t>(2 * plan.pieces + 1));
    plan.host_piece_first.resize(static_cast<size_t>(n + 1));
    GWM_CHECK(hipMemcpyAsync(lengths.data(), plan.piece_lengths, sizeof(int64_t) * lengths.size(), hipMemcpyDeviceToHost, s));
    GWM_CHECK(hipMemcpyAsync(plan.host_piece_first.data(), plan.piece_first, sizeof(int64_t) * plan.host_piece_first.size(),
                             hipMemcpyDeviceToHost, s));
    GWM_CHECK(hipStreamSynchronize(s));
    plan.host_starts.assign(lengths.size(), 0);
    plan.longest_query_piece = 0;
    for (int64_t p = 0; p < plan.pieces; ++p)
    {
        plan.host_starts[2 * p + 1] = plan.host_starts[2 * p] + lengths[2 * p];
        plan.host_starts[2 * p + 2] = plan.host_starts[2 * p + 1] + lengths[2 * p + 1];
        plan.longest_query_piece    = std::max(plan.longest_query_piece, lengths[2 * p]);
    }
}

void gather_pieces(const AnchorPlan& plan, const gwm_overlap* overlaps, int64_t first_piece, int64_t count, const ReadSet& q,
                   const ReadSet& t, const int64_t* starts, uint8_t* sequences, hipStream_t s)
{
    const int64_t slices = 2 * count;
    piece_gather_kernel<<<static_cast<unsigned>((slices + kWavesPerBlock - 1) / kWavesPerBlock), kThreads, 0, s>>>(
        overlaps, plan.piece_u + first_piece, plan.piece_v + first_piece, plan.piece_record + first_piece, slices, q, t, starts,
        sequences);
    GWM_CHECK(hipGetLastError());
}

void record_starts(const AnchorPlan& plan, const gwm_overlap* overlaps, int64_t first, int64_t m, const int64_t* piece_starts,
                   int64_t* starts, hipStream_t s)
{
    record_starts_kernel<<<grid_for(m + 1), kThreads, 0, s>>>(overlaps + first, plan.piece_first + first, m, piece_starts, starts);
    GWM_CHECK(hipGetLastError());
}

void stitch_pieces(const AnchorPlan& plan, int64_t first, int64_t m, const uint8_t* piece_results, const int64_t* piece_starts,
                   const int32_t* piece_result_lengths, uint8_t* results, const int64_t* starts, int32_t* result_lengths,
                   hipStream_t s)
{
    stitch_kernel<<<static_cast<unsigned>((m + kWavesPerBlock - 1) / kWavesPerBlock), kThreads, 0, s>>>(
        piece_results, piece_starts, piece_result_lengths, plan.piece_first + first, m, results, starts, result_lengths);
    GWM_CHECK(hipGetLastError());
}

} // namespace gwm
