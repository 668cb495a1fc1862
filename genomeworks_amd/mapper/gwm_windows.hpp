// gwm_windows.hpp -- polishing's and read correction's layer selection: plain host arithmetic over the segment records
// of gwm_window_segments / gwm_pair_segments, the overlap records and the read lengths. No HIP call and no HIP header,
// so it is tested without a device (gw_mapper_select_layers, gw_mapper_select_pairs,
// gw_mapper_select_correction_layers and their _weighted variants) and under the host sanitizers
// (tests/cpp/select_layers_sanitized.cpp, tests/cpp/select_correction_sanitized.cpp,
// tests/cpp/select_quality_sanitized.cpp).
#ifndef GWM_WINDOWS_HPP
#define GWM_WINDOWS_HPP

#include "gwhip_mapper.h"

#include <cstdint>
#include <vector>

namespace gwm
{

// One window of a target read (in read correction: of the read that owns it) and where its sequences stand in the gather plan: the backbone, then the layers.
struct window_record
{
    uint32_t target_read; // position in the target set
    uint32_t window;
    uint32_t first_sequence;
    uint32_t n_sequences; // 1 + layers
};

struct window_selection
{
    std::vector<gwm_gather_entry> plan;
    std::vector<window_record> windows;
};

// The windows of every target read with their layers, W = window_length:
//  1. one overlap per query read is kept, the one with the greatest query end - query start, on ties the first;
//  2. a record of a kept overlap is a layer when, with end_k = min((k + 1) W, target length),
//     target_first - k W <= W / 100, end_k - 1 - target_last <= W / 100 and 1 <= query_end - query_begin <= 2 W;
//  3. the layers of a (target read, window) are ordered by (target_first, overlap position), the first max_depth kept;
//  4. a layer is query[query_begin, query_end), reversed through the aligner's table on '-';
//  5. a target read of L > 0 bases has windows 0 .. (L - 1) / W, window k with the backbone target[k W, end_k).
// Windows come by target read, then by window. Throws std::invalid_argument for window_length < 1, max_depth < 0, a
// record that names an overlap, a read or a window that does not exist, and 2^32 sequences or more.
// quality_sums (Q2 of INTEGRATION.md section 3l; nullptr: the query set has no qualities and nothing changes):
// quality_sums[j] is the quality sum of record j (gwm_segment_quality_sums), and a record is a layer only if it also
// has quality_sums[j] > 0 and quality_sums[j] >= min_mean_quality * (query_end - query_begin), in 64 bits. The filter
// comes before the ordering and the max_depth cut of rule 3. A negative min_mean_quality throws.
window_selection select_layers(const gwm_segment* segments, int64_t n_segments, const gwm_overlap* overlaps,
                               int64_t n_overlaps, int32_t n_queries, uint32_t first_query_read_id,
                               const int64_t* target_lengths, int32_t n_targets, uint32_t first_target_read_id,
                               int32_t window_length, int32_t max_depth, const uint32_t* quality_sums = nullptr,
                               int32_t min_mean_quality = 0);

// Read correction, C1 of INTEGRATION.md section 3k: the records of an all-against-all mapping that are aligned. Records
// of a read with itself are dropped; of the remaining records of an unordered pair of reads, in either direction, the
// one with the greatest query end - query start is kept, on ties the first. Returns the kept positions, ascending.
// Throws std::invalid_argument for a negative count and a record that starts behind its end.
std::vector<int64_t> select_pairs(const gwm_overlap* overlaps, int64_t n_overlaps);

// Read correction, C3 and C4: the windows of every read of the one set with their layers, from the records of both
// roles of gwm_pair_segments. A record's owner is its pair's target read in the target role and its query read in the
// query role; the record is a layer of (owner, window) under rule 2 above with the owner's length. Layers are ordered
// by (target_first, pair position, target role first) and cut at max_depth. A target-role layer is
// query[query_begin, query_end), a query-role layer target[query_begin, query_end), either reversed on '-'. Backbones
// and windows as in rule 5. Every plan entry is of set 0; window_record::target_read is the owner. Throws as
// select_layers does. target_role_quality_sums / query_role_quality_sums: the quality sums of the records of either
// role, filtered as in select_layers; nullptr leaves that role's records unfiltered.
window_selection select_correction_layers(const gwm_segment* target_role, int64_t n_target_role,
                                          const gwm_segment* query_role, int64_t n_query_role, const gwm_overlap* pairs,
                                          int64_t n_pairs, const int64_t* read_lengths, int32_t n_reads,
                                          uint32_t first_read_id, int32_t window_length, int32_t max_depth,
                                          const uint32_t* target_role_quality_sums = nullptr,
                                          const uint32_t* query_role_quality_sums  = nullptr,
                                          int32_t min_mean_quality                 = 0);

} // namespace gwm

#endif
