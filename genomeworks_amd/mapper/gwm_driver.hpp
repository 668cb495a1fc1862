// gwm_driver.hpp -- the batched driver of cudamapper: what the gw_mapper_map_batched* entry points of
// include/gw_mapper_capi.h run (implementation and its parts in gwm_driver.cpp).
#ifndef GWM_DRIVER_HPP
#define GWM_DRIVER_HPP

#include "gwm_handles.hpp"

namespace gwm
{

// Everything gw_mapper_map_batched_cached takes behind the two read sets, by the names and in the order of its
// parameters.
struct map_options
{
    int32_t kmer_size, window_size;
    double filtering_parameter;
    int64_t min_residues, min_overlap_len, min_bases_per_residue;
    float min_overlap_fraction;
    int64_t max_basepairs_per_query_index, max_basepairs_per_target_index;
    int32_t post_process, drop_fused_overlaps, rescue_overlap_ends, align_overlaps;
    int64_t max_device_bytes;
    int32_t query_indices_in_host_memory, query_indices_in_device_memory;
    int32_t target_indices_in_host_memory, target_indices_in_device_memory;
    // what gw_mapper_map_batched_chained adds: the chaining overlapper in the place of the triggered one
    int32_t chained;
    gwm_chaining chaining;
};

// Maps queries against targets (targets without bases: all against all) index pair by index pair, walking the pairs
// in the host and device batches of the index batcher. The caller owns the result. Throws on any error.
gw_mapper_overlaps* map_batched(const reads_view& queries, const reads_view& targets, const map_options& options,
                                hipStream_t stream);

} // namespace gwm

#endif
