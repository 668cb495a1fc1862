// gwm_qualities.hip -- cudamapper on gfx950: base qualities next to the bases of polishing and read correction
// (include/gwhip_mapper.h, gwm_segment_quality_sums and gwm_gather_weights; the rules are Q1 and Q3 of INTEGRATION.md
// section 3l). A read set's qualities are Phred+33 bytes that share the offsets of its bases; the weight of byte c is
// c - 33. gwm_segment_quality_sums gives the layer selection on the host one uint32 per segment record, the sum of the
// weights of the bases the record would supply, so the qualities themselves never cross to the host;
// gwm_gather_weights walks the gather plan of gwm_gather_sequences a second time and cuts the weights of every window
// sequence out of the resident qualities. Both are streaming passes over bytes: no LDS, no scratch.
#include "gwm_align_chunks.hpp"
#include "gwm_gather_plan.hpp"

namespace
{

// the weight of a quality byte. The host refuses bytes outside 33..126 before they are uploaded; the clamp keeps a
// byte that reached the device some other way within cudapoa's non-negative int8.
__device__ __forceinline__ uint32_t weight_of(uint8_t c) { return c < 33 ? 0u : min(static_cast<uint32_t>(c) - 33u, 93u); }

// the read that supplies the layer of a record of overlap x: the query read in the target role, the target read in
// the query role
template <bool kQueryRole>
__device__ __forceinline__ uint32_t supplier_of(const gwm_overlap& x)
{
    return kQueryRole ? x.target_read_id : x.query_read_id;
}

// bad[0] |= 1: a record names an overlap that does not exist; |= 2: its overlap names a read outside the set;
// |= 4: query_begin > query_end or query_end beyond the read
template <bool kQueryRole>
__global__ void __launch_bounds__(kThreads) records_validate_kernel(const gwm_segment* __restrict__ segments, int64_t n,
                                                                    const gwm_overlap* __restrict__ overlaps,
                                                                    int64_t n_overlaps, ReadSet set,
                                                                    uint32_t* __restrict__ bad)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const gwm_segment r = segments[i];
    if (static_cast<int64_t>(r.overlap) >= n_overlaps)
    {
        atomicOr(bad, 1u);
        return;
    }
    const uint32_t id = supplier_of<kQueryRole>(overlaps[r.overlap]);
    if (id < set.first_read_id || id - set.first_read_id >= set.n_reads)
    {
        atomicOr(bad, 2u);
        return;
    }
    const uint32_t read   = id - set.first_read_id;
    const uint64_t length = static_cast<uint64_t>(set.offsets[read + 1] - set.offsets[read]);
    if (r.query_begin > r.query_end || r.query_end > length)
        atomicOr(bad, 4u);
}

// One wave64 per record: the lanes stride the supplier's quality bytes [query_begin, query_end) with ascending
// addresses, 64 consecutive bytes per pass, each lane summing in 64 bits; one butterfly over the wave, and lane 0
// stores the sum, saturated. Records were validated by records_validate_kernel. set.bases are the qualities.
template <bool kQueryRole>
__global__ void __launch_bounds__(kThreads) quality_sums_kernel(const gwm_segment* __restrict__ segments, int64_t n,
                                                                const gwm_overlap* __restrict__ overlaps, ReadSet set,
                                                                uint32_t* __restrict__ sums)
{
    const int64_t i     = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= n)
        return; // whole waves leave together
    const gwm_segment r  = segments[i];
    const uint32_t read  = supplier_of<kQueryRole>(overlaps[r.overlap]) - set.first_read_id;
    const uint8_t* q     = set.bases + set.offsets[read] + r.query_begin;
    const uint32_t bytes = r.query_end - r.query_begin;
    uint64_t sum         = 0;
#pragma unroll 4
    for (uint32_t j = lane; j < bytes; j += 64)
        sum += weight_of(q[j]);
    for (int step = 32; step >= 1; step >>= 1)
        sum += __shfl_xor(static_cast<unsigned long long>(sum), step, 64);
    if (lane == 0)
        sums[i] = static_cast<uint32_t>(min(sum, static_cast<uint64_t>(0xffffffffu)));
}

// Block b writes the weights of sequence b of the plan to out[out_starts[b] ..): lane L of a pass takes output byte L,
// as gather_sequences_kernel does, reversed entries back to front and nothing complemented. A set without qualities
// (bases == nullptr) gives weight 1 throughout.
__global__ void __launch_bounds__(kThreads) gather_weights_kernel(const gwm_gather_entry* __restrict__ plan,
                                                                  const int64_t* __restrict__ out_starts, ReadSet qs,
                                                                  ReadSet ts, int8_t* __restrict__ out)
{
    const gwm_gather_entry e = plan[blockIdx.x];
    const ReadSet& set       = e.set ? ts : qs;
    const uint32_t len       = e.end - e.begin;
    int8_t* dst              = out + out_starts[blockIdx.x];
    if (set.bases == nullptr)
    {
        for (uint32_t j = threadIdx.x; j < len; j += kThreads)
            dst[j] = 1;
        return;
    }
    const auto weight = [](uint8_t c) { return weight_of(c); };
    copy_slice(dst, set.bases + set.offsets[e.read] + e.begin, len, e.reversed != 0, weight, weight);
}

template <bool kQueryRole>
void quality_sums(const gwm_segment* segments, int64_t n, const gwm_overlap* overlaps, int64_t n_overlaps,
                  const ReadSet& set, uint32_t* sums, hipStream_t s, float* sums_ms)
{
    dbuf<uint32_t> bad(1);
    GWM_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    records_validate_kernel<kQueryRole><<<grid_for(n), kThreads, 0, s>>>(segments, n, overlaps, n_overlaps, set, bad.p);
    GWM_CHECK(hipGetLastError());
    const uint32_t what = to_host(bad.p, s);
    if (what & 1u)
        throw std::invalid_argument("gwm_segment_quality_sums: a record names an overlap that does not exist");
    if (what & 2u)
        throw std::invalid_argument("gwm_segment_quality_sums: a record's overlap names a read outside the read set");
    if (what & 4u)
        throw std::invalid_argument("gwm_segment_quality_sums: a record lies beyond the end of its read");
    const unsigned blocks = static_cast<unsigned>((n + kWavesPerBlock - 1) / kWavesPerBlock);
    timed_launch(s, sums_ms, [&] {
        quality_sums_kernel<kQueryRole><<<blocks, kThreads, 0, s>>>(segments, n, overlaps, set, sums);
    });
}

} // namespace

extern "C" {

int gwm_segment_quality_sums(const gwm_segment* segments, int64_t n_segments, const gwm_overlap* overlaps,
                             int64_t n_overlaps, int32_t query_role, const char* qualities, const int64_t* offsets,
                             int32_t n_reads, uint32_t first_read_id, uint32_t* sums, void* stream, float* sums_ms)
{
    try
    {
        if (sums_ms)
            *sums_ms = 0.f;
        if (n_reads < 0 || n_overlaps < 0)
            throw std::invalid_argument("gwm_segment_quality_sums: a negative count");
        if (n_segments <= 0)
            return 0;
        if (n_segments >= (int64_t(1) << 31) * kWavesPerBlock)
            throw std::invalid_argument("gwm_segment_quality_sums: 2^33 records or more");
        if (!qualities || !offsets || !sums)
            throw std::invalid_argument("gwm_segment_quality_sums: a null array");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const ReadSet set = read_set(qualities, offsets, n_reads, first_read_id);
        if (query_role)
            quality_sums<true>(segments, n_segments, overlaps, n_overlaps, set, sums, s, sums_ms);
        else
            quality_sums<false>(segments, n_segments, overlaps, n_overlaps, set, sums, s, sums_ms);
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        return -1;
    }
}

int gwm_gather_weights(const gwm_gather_entry* plan, int64_t n, const int64_t* out_starts, const char* query_qualities,
                       const int64_t* query_offsets, int32_t n_queries, const char* target_qualities,
                       const int64_t* target_offsets, int32_t n_targets, int8_t* out, int64_t out_bytes, void* stream,
                       float* gather_ms)
{
    try
    {
        if (gather_ms)
            *gather_ms = 0.f;
        if (n_queries < 0 || n_targets < 0)
            throw std::invalid_argument("gwm_gather_weights: negative number of reads");
        if (out_bytes < 0)
            throw std::invalid_argument("gwm_gather_weights: negative out_bytes");
        if (n <= 0)
            return 0;
        if (n >= (int64_t(1) << 31))
            throw std::invalid_argument("gwm_gather_weights: 2^31 sequences or more");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const ReadSet q = read_set(query_qualities, query_offsets, n_queries, 0);
        const ReadSet t = read_set(target_qualities, target_offsets, n_targets, 0);
        validate_plan("gwm_gather_weights", plan, n, out_starts, q, t, out_bytes, s);
        timed_launch(s, gather_ms, [&] {
            gather_weights_kernel<<<static_cast<unsigned>(n), kThreads, 0, s>>>(plan, out_starts, q, t, out);
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
