// gwm_gather_plan.hpp -- the validation of a gather plan, shared by the two kernels that walk one:
// gwm_gather_sequences (gwm_segments.hip) cuts the bases of a plan's sequences out of the read sets, gwm_gather_weights
// (gwm_qualities.hip) the weights of the same sequences out of the sets' qualities. Both refuse a bad plan before
// anything is written.
#ifndef GWM_GATHER_PLAN_HPP
#define GWM_GATHER_PLAN_HPP

#include "gwhip_mapper.h"

#include "gwm_device_utils.hpp"

namespace
{

// bad[0] |= 1: a set other than 0 / 1 or a read outside its set; |= 2: begin > end or an end beyond its read;
// |= 4: the sequence does not lie within out
__global__ void __launch_bounds__(kThreads) plan_validate_kernel(const gwm_gather_entry* __restrict__ plan, int64_t n,
                                                                 const int64_t* __restrict__ out_starts, ReadSet q,
                                                                 ReadSet t, int64_t out_bytes,
                                                                 uint32_t* __restrict__ bad)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const gwm_gather_entry e = plan[i];
    const ReadSet& set       = e.set ? t : q;
    if (e.set > 1 || e.read >= set.n_reads)
    {
        atomicOr(bad, 1u);
        return;
    }
    const uint64_t length = static_cast<uint64_t>(set.offsets[e.read + 1] - set.offsets[e.read]);
    if (e.begin > e.end || e.end > length)
    {
        atomicOr(bad, 2u);
        return;
    }
    const int64_t at = out_starts[i];
    if (at < 0 || at > out_bytes || static_cast<int64_t>(e.end - e.begin) > out_bytes - at)
        atomicOr(bad, 4u);
}

// throws std::invalid_argument, opened by `who`, for a plan one of whose sequences plan_validate_kernel marks; waits
// for s. Only the offsets and the read counts of q and t are read.
inline void validate_plan(const std::string& who, const gwm_gather_entry* plan, int64_t n, const int64_t* out_starts,
                          const ReadSet& q, const ReadSet& t, int64_t out_bytes, hipStream_t s)
{
    dbuf<uint32_t> bad(1);
    GWM_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    plan_validate_kernel<<<grid_for(n), kThreads, 0, s>>>(plan, n, out_starts, q, t, out_bytes, bad.p);
    GWM_CHECK(hipGetLastError());
    const uint32_t what = to_host(bad.p, s);
    if (what & 1u)
        throw std::invalid_argument(who + ": a sequence names a read outside the read sets");
    if (what & 2u)
        throw std::invalid_argument(who + ": a sequence lies beyond the end of its read");
    if (what & 4u)
        throw std::invalid_argument(who + ": a sequence does not lie within the output");
}

} // namespace

#endif
