// gwm_postprocess.hip -- cudamapper on gfx950: what the reference does with the overlaps of one index pair before it
// prints them (include/gwhip_mapper.h): fusion of neighbouring overlaps (Overlapper::post_process_overlaps, with or
// without dropping the pieces) and end rescue (Overlapper::rescue_overlap_ends). Semantics restated from scratch;
// INTEGRATION.md section 3h lists the rules.
//
// Fusion is element-parallel like the overlapper: one lane per adjacent pair for the mergeable flag, selects for the
// first and last pair of every run, a scan for the residue sums, one lane per run for the fused record, a select for
// the drop mask. End rescue runs one wave64 per overlap: every lane holds one 15-mer of each window as two 64-bit
// words, and a ballot counts the matched ones. No LDS, no scratch in the hand-written kernels.
#include "gwhip_mapper.h"

#include "gwm_device_utils.hpp"

namespace
{

constexpr uint32_t kRescueKmer         = 15;
constexpr int32_t kRescueMaxExtension  = 78; // 78 - 15 + 1 = 64 k-mers: one per lane
constexpr unsigned kWavesPerBlock      = kThreads / 64;

// abs(int(a - b)) over uint32 operands, as the reference's call resolves; -2^31 stays -2^31.
__device__ inline int32_t abs_wrapped(uint32_t a, uint32_t b)
{
    const uint32_t d = a - b;
    return static_cast<int32_t>((d & 0x80000000u) ? 0u - d : d);
}

__device__ inline bool mergable(const gwm_overlap& o1, const gwm_overlap& o2)
{
    const bool forward = o1.relative_strand == '+' && o2.relative_strand == '+';
    const bool reverse = o1.relative_strand == '-' && o2.relative_strand == '-';
    if (!(forward || reverse))
        return false;
    if (o1.query_read_id != o2.query_read_id || o1.target_read_id != o2.target_read_id)
        return false;
    const int32_t query_gap  = abs_wrapped(o2.query_start_position_in_read, o1.query_end_position_in_read);
    const int32_t target_gap = reverse ? abs_wrapped(o1.target_start_position_in_read, o2.target_end_position_in_read)
                                       : abs_wrapped(o2.target_start_position_in_read, o1.target_end_position_in_read);
    if (query_gap < 500 && target_gap < 500)
        return true;
    // float ratio against the double 0.8
    const int32_t lo  = query_gap < target_gap ? query_gap : target_gap;
    const int32_t hi  = query_gap < target_gap ? target_gap : query_gap;
    const float ratio = __fdiv_rn(static_cast<float>(lo), static_cast<float>(hi));
    if (static_cast<double>(ratio) > 0.8)
        return true;
    const uint32_t total_q = (o1.query_end_position_in_read - o1.query_start_position_in_read) +
                             (o2.query_end_position_in_read - o2.query_start_position_in_read);
    const uint32_t total_t = (o1.target_end_position_in_read - o1.target_start_position_in_read) +
                             (o2.target_end_position_in_read - o2.target_start_position_in_read);
    const float pq = __fdiv_rn(static_cast<float>(query_gap), static_cast<float>(total_q));
    const float pt = __fdiv_rn(static_cast<float>(target_gap), static_cast<float>(total_t));
    return static_cast<double>(pq) < 0.2 && static_cast<double>(pt) < 0.2;
}

// merge[i]: overlaps i and i + 1 fuse, i in [0, n - 1). Also the residue counts for the scan.
__global__ void __launch_bounds__(kThreads) merge_flags_kernel(const gwm_overlap* __restrict__ o, int64_t n,
                                                               uint32_t* __restrict__ merge,
                                                               uint32_t* __restrict__ residues)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    residues[i] = o[i].num_residues;
    if (i + 1 < n)
        merge[i] = mergable(o[i], o[i + 1]) ? 1u : 0u;
}

// A run is a maximal stretch of set merge flags: first[i] marks its first pair, last[i] its last one; keep[i] is set
// for an overlap that belongs to no mergeable pair.
__global__ void __launch_bounds__(kThreads) run_flags_kernel(const uint32_t* __restrict__ merge, int64_t n,
                                                             uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                             uint32_t* __restrict__ keep)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const bool before = i > 0 && merge[i - 1];
    const bool here   = i + 1 < n && merge[i];
    const bool after  = i + 2 < n && merge[i + 1];
    keep[i]           = (before || here) ? 0u : 1u;
    if (i + 1 < n)
    {
        first[i] = (here && !before) ? 1u : 0u;
        last[i]  = (here && !after) ? 1u : 0u;
    }
}

// Run r spans overlaps [first_pair[r], last_pair[r] + 1]. Its record copies the run's last member, or the second to
// last when the run reaches the end of the array, and then takes the fused coordinates and the residue sum.
__global__ void __launch_bounds__(kThreads) fuse_runs_kernel(const gwm_overlap* __restrict__ o, int64_t n,
                                                             const uint32_t* __restrict__ first_pair,
                                                             const uint32_t* __restrict__ last_pair, uint32_t n_runs,
                                                             const uint32_t* __restrict__ residue_sum,
                                                             gwm_overlap* __restrict__ out)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs)
        return;
    const uint32_t a    = first_pair[r];
    const uint32_t b    = last_pair[r] + 1;
    const gwm_overlap f = o[a];
    const gwm_overlap l = o[b];
    gwm_overlap x       = o[(static_cast<int64_t>(b) == n - 1) ? b - 1 : b];
    x.query_start_position_in_read = f.query_start_position_in_read;
    x.query_end_position_in_read   = l.query_end_position_in_read;
    if (l.relative_strand == '+')
    {
        x.target_start_position_in_read = f.target_start_position_in_read;
        x.target_end_position_in_read   = l.target_end_position_in_read;
    }
    else
    {
        x.target_start_position_in_read = l.target_start_position_in_read;
        x.target_end_position_in_read   = f.target_end_position_in_read;
    }
    x.num_residues = residue_sum[b] - (a > 0 ? residue_sum[a - 1] : 0u);
    out[r]         = x;
}

// ------------------------------------------------------------------------------------------------------------------
// end rescue
// ------------------------------------------------------------------------------------------------------------------

// bad[0] |= 1: a read id outside its read set; |= 2: a start or end beyond its read
__global__ void __launch_bounds__(kThreads) validate_kernel(const gwm_overlap* __restrict__ o, int64_t n, ReadSet q,
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
    const uint64_t ql = static_cast<uint64_t>(q.offsets[qi + 1] - q.offsets[qi]);
    const uint64_t tl = static_cast<uint64_t>(t.offsets[ti + 1] - t.offsets[ti]);
    if (x.query_start_position_in_read > ql || x.query_end_position_in_read > ql ||
        x.target_start_position_in_read > tl || x.target_end_position_in_read > tl)
        atomicOr(bad, 2u);
}

// A<->T, C<->G; every other byte stays
__device__ inline uint32_t complement(uint32_t c)
{
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

// Number of 15-mers (multiset) two windows of `size` bases share: the query window starts at q, the target window at
// position tpos of the target as the overlap sees it (the reverse complement when `reverse`; t points at the forward
// read of tlen bases). A window shorter than 15 bases is one k-mer of `size` bytes. Lane L holds k-mer L of both
// windows; k-mer L of the query is shared when its rank among the equal query k-mers before it is below the number of
// equal target k-mers. Called by whole waves only.
__device__ inline uint32_t shared_kmers(const uint8_t* __restrict__ q, const uint8_t* __restrict__ t, uint32_t tlen,
                                        uint32_t tpos, bool reverse, uint32_t size, uint32_t lane, uint32_t* n_kmers)
{
    const uint32_t nk  = size < kRescueKmer ? 1u : size - kRescueKmer + 1;
    const uint32_t len = size < kRescueKmer ? size : kRescueKmer;
    *n_kmers           = nk;
    uint64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (lane < nk)
    {
        for (uint32_t j = 0; j < len; ++j)
        {
            const uint64_t ca = q[lane + j];
            const uint32_t p  = tpos + lane + j;
            // reverse complement read in place; the reference leaves the middle base of an odd-length read as it is
            const uint32_t at = reverse ? tlen - 1 - p : p;
            const uint32_t c  = t[at];
            const uint64_t cb = (reverse && !((tlen & 1u) && at == tlen / 2)) ? complement(c) : c;
            if (j < 8)
            {
                a0 |= ca << (8 * j);
                b0 |= cb << (8 * j);
            }
            else
            {
                a1 |= ca << (8 * (j - 8));
                b1 |= cb << (8 * (j - 8));
            }
        }
    }
    uint32_t rank = 0, in_b = 0;
    for (uint32_t j = 0; j < nk; ++j)
    {
        const uint64_t x0 = __shfl(a0, static_cast<int>(j), 64);
        const uint64_t x1 = __shfl(a1, static_cast<int>(j), 64);
        const uint64_t y0 = __shfl(b0, static_cast<int>(j), 64);
        const uint64_t y1 = __shfl(b1, static_cast<int>(j), 64);
        rank += (j < lane && x0 == a0 && x1 == a1) ? 1u : 0u;
        in_b += (y0 == a0 && y1 == a1) ? 1u : 0u;
    }
    return static_cast<uint32_t>(__popcll(__ballot(lane < nk && rank < in_b)));
}

__global__ void __launch_bounds__(kThreads) rescue_kernel(gwm_overlap* __restrict__ overlaps, int64_t n, ReadSet qs,
                                                          ReadSet ts, uint32_t extension, float required_similarity)
{
    const int64_t i     = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n)
        return; // whole waves leave together
    const gwm_overlap o  = overlaps[i];
    const uint32_t qi    = o.query_read_id - qs.first_read_id;
    const uint32_t ti    = o.target_read_id - ts.first_read_id;
    const uint8_t* q     = qs.bases + qs.offsets[qi];
    const uint8_t* t     = ts.bases + ts.offsets[ti];
    const uint32_t qlen  = static_cast<uint32_t>(qs.offsets[qi + 1] - qs.offsets[qi]);
    const uint32_t tlen  = static_cast<uint32_t>(ts.offsets[ti + 1] - ts.offsets[ti]);
    const bool reverse   = o.relative_strand == '-';
    uint32_t q_start = o.query_start_position_in_read, q_end = o.query_end_position_in_read;
    // a '-' overlap in the coordinates of the reverse-complemented target
    uint32_t t_start = reverse ? tlen - o.target_end_position_in_read : o.target_start_position_in_read;
    uint32_t t_end   = reverse ? tlen - o.target_start_position_in_read : o.target_end_position_in_read;
    // The reference's early exit only fires on a round that changed nothing, after which the remaining rounds change
    // nothing either: three rounds always give its result.
    for (int round = 0; round < 3; ++round)
    {
        uint32_t nk;
        const uint32_t head = min(min(q_start, t_start), extension);
        uint32_t shared     = shared_kmers(q + (q_start - head), t, tlen, t_start - head, reverse, head, lane, &nk);
        if (__fdiv_rn(static_cast<float>(shared), static_cast<float>(2 * nk - shared)) >= required_similarity)
        {
            q_start -= head;
            t_start -= head;
        }
        const uint32_t tail = min(extension, min(qlen - q_end, tlen - t_end));
        shared              = shared_kmers(q + q_end, t, tlen, t_end, reverse, tail, lane, &nk);
        if (__fdiv_rn(static_cast<float>(shared), static_cast<float>(2 * nk - shared)) >= required_similarity)
        {
            q_end += tail;
            t_end += tail;
        }
    }
    if (lane == 0)
    {
        overlaps[i].query_start_position_in_read  = q_start;
        overlaps[i].query_end_position_in_read    = q_end;
        overlaps[i].target_start_position_in_read = reverse ? tlen - t_end : t_start;
        overlaps[i].target_end_position_in_read   = reverse ? tlen - t_start : t_end;
    }
}

} // namespace

extern "C" {

int gwm_post_process_overlaps(const gwm_overlap* overlaps, int64_t n, int32_t drop_fused_overlaps, void* stream,
                              gwm_overlap* out, int64_t* count, float* fuse_ms)
{
    *count = 0;
    if (fuse_ms)
        *fuse_ms = 0.f;
    try
    {
        if (n <= 0)
            return 0;
        if (n >= (int64_t(1) << 32) - 1)
            throw std::invalid_argument("gwm_post_process_overlaps: 2^32 - 1 overlaps or more");
        hipStream_t s = static_cast<hipStream_t>(stream);
        Events ev(2);
        ev.record(0, s);
        int64_t n_kept = n;
        uint32_t n_runs = 0;
        if (n == 1)
        {
            GWM_CHECK(hipMemcpyAsync(out, overlaps, sizeof(gwm_overlap), hipMemcpyDeviceToDevice, s));
        }
        else
        {
            Temp temp;
            dbuf<uint32_t> d_count(1);
            dbuf<uint32_t> merge(n - 1), first(n - 1), last(n - 1), keep(n), residues(n), residue_sum(n);
            dbuf<uint32_t> first_pair(n - 1), last_pair(n - 1);
            merge_flags_kernel<<<grid_for(n), kThreads, 0, s>>>(overlaps, n, merge.p, residues.p);
            GWM_CHECK(hipGetLastError());
            run_flags_kernel<<<grid_for(n), kThreads, 0, s>>>(merge.p, n, first.p, last.p, keep.p);
            GWM_CHECK(hipGetLastError());
            inclusive_sum(residues.p, residue_sum.p, n, temp, s);
            n_runs = select_indices(first.p, n - 1, first_pair.p, d_count.p, temp, s);
            if (drop_fused_overlaps && n_runs > 0)
            {
                size_t bytes = 0;
                GWM_CHECK(rocprim::select(nullptr, bytes, overlaps, keep.p, out, d_count.p, static_cast<size_t>(n), s));
                GWM_CHECK(rocprim::select(temp.get(bytes), bytes, overlaps, keep.p, out, d_count.p,
                                          static_cast<size_t>(n), s));
                n_kept = to_host(d_count.p, s);
            }
            else
            {
                GWM_CHECK(hipMemcpyAsync(out, overlaps, sizeof(gwm_overlap) * static_cast<size_t>(n),
                                         hipMemcpyDeviceToDevice, s));
            }
            if (n_runs > 0)
            {
                const uint32_t n_last = select_indices(last.p, n - 1, last_pair.p, d_count.p, temp, s);
                if (n_last != n_runs)
                    throw std::logic_error("gwm_post_process_overlaps: run heads and tails disagree");
                fuse_runs_kernel<<<grid_for(n_runs), kThreads, 0, s>>>(overlaps, n, first_pair.p, last_pair.p, n_runs,
                                                                      residue_sum.p, out + n_kept);
                GWM_CHECK(hipGetLastError());
            }
        }
        ev.record(1, s);
        GWM_CHECK(hipStreamSynchronize(s));
        if (fuse_ms)
            *fuse_ms = ev.ms(0, 1);
        *count = n_kept + n_runs;
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        return -1;
    }
}

int gwm_rescue_overlap_ends(gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                            int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                            const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                            int32_t extension, float required_similarity, void* stream, float* rescue_ms)
{
    if (rescue_ms)
        *rescue_ms = 0.f;
    try
    {
        if (extension < 0 || extension > kRescueMaxExtension)
            throw std::invalid_argument("gwm_rescue_overlap_ends: extension must be in 0..78");
        if (n_queries < 0 || n_targets < 0)
            throw std::invalid_argument("gwm_rescue_overlap_ends: negative number of reads");
        if (n <= 0)
            return 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        const ReadSet q{reinterpret_cast<const uint8_t*>(query_bases), query_offsets, static_cast<uint32_t>(n_queries),
                        first_query_read_id};
        const ReadSet t{reinterpret_cast<const uint8_t*>(target_bases), target_offsets,
                        static_cast<uint32_t>(n_targets), first_target_read_id};
        Events ev(2);
        dbuf<uint32_t> bad(1);
        ev.record(0, s);
        GWM_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
        validate_kernel<<<grid_for(n), kThreads, 0, s>>>(overlaps, n, q, t, bad.p);
        GWM_CHECK(hipGetLastError());
        const uint32_t what = to_host(bad.p, s);
        if (what & 1u)
            throw std::invalid_argument("gwm_rescue_overlap_ends: an overlap names a read outside the read set");
        if (what & 2u)
            throw std::invalid_argument("gwm_rescue_overlap_ends: an overlap lies beyond the end of its read");
        const unsigned blocks = static_cast<unsigned>((n + kWavesPerBlock - 1) / kWavesPerBlock);
        rescue_kernel<<<blocks, kThreads, 0, s>>>(overlaps, n, q, t, static_cast<uint32_t>(extension),
                                                 required_similarity);
        GWM_CHECK(hipGetLastError());
        ev.record(1, s);
        GWM_CHECK(hipStreamSynchronize(s));
        if (rescue_ms)
            *rescue_ms = ev.ms(0, 1);
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        return -1;
    }
}

} // extern "C"
