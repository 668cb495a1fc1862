// gwm_overlap_filter.hpp -- the overlap filter both overlappers end with (gwm_mapper.hip: the triggered one,
// gwm_chain.hip: the chaining one), restated from the reference's FilterOverlapOp.
#ifndef GWM_OVERLAP_FILTER_HPP
#define GWM_OVERLAP_FILTER_HPP

#include "gwhip_mapper.h"

#include <hip/hip_runtime.h>

namespace
{

// FilterOverlapOp: unsigned lengths, integer bases per residue, strict > on the float fractions
__device__ inline bool passes_overlap_filter(const gwm_overlap& o, int32_t all_to_all, uint64_t min_residues,
                                             uint64_t min_overlap_len, uint64_t min_bases_per_residue,
                                             float min_overlap_fraction)
{
    const uint32_t tl  = o.target_end_position_in_read - o.target_start_position_in_read;
    const uint32_t ql  = o.query_end_position_in_read - o.query_start_position_in_read;
    const uint32_t len = tl > ql ? tl : ql;
    const bool self    = o.query_read_id == o.target_read_id && all_to_all;
    return o.num_residues >= min_residues && (len / o.num_residues) < min_bases_per_residue &&
           ql >= min_overlap_len && tl >= min_overlap_len && !self &&
           (static_cast<float>(tl) * 1.f / static_cast<float>(len)) > min_overlap_fraction &&
           (static_cast<float>(ql) * 1.f / static_cast<float>(len)) > min_overlap_fraction;
}

} // namespace

#endif
