// gwm_windows.hpp -- polishing's layer selection: plain host arithmetic over the segment records of
// gwm_window_segments, the overlap records and the target read lengths. No HIP call and no HIP header, so it is tested
// without a device (gw_mapper_select_layers) and under the host sanitizers (tests/cpp/select_layers_sanitized.cpp).
#ifndef GWM_WINDOWS_HPP
#define GWM_WINDOWS_HPP

#include "gwhip_mapper.h"

#include <cstdint>
#include <vector>

namespace gwm
{

// One window of a target read and where its sequences stand in the gather plan: the backbone, then the layers.
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
window_selection select_layers(const gwm_segment* segments, int64_t n_segments, const gwm_overlap* overlaps,
                               int64_t n_overlaps, int32_t n_queries, uint32_t first_query_read_id,
                               const int64_t* target_lengths, int32_t n_targets, uint32_t first_target_read_id,
                               int32_t window_length, int32_t max_depth);

} // namespace gwm

#endif
