// gwm_windows.cpp -- the layer selection of gwm_windows.hpp.
#include "gwm_windows.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace gwm
{

window_selection select_layers(const gwm_segment* segments, int64_t n_segments, const gwm_overlap* overlaps,
                               int64_t n_overlaps, int32_t n_queries, uint32_t first_query_read_id,
                               const int64_t* target_lengths, int32_t n_targets, uint32_t first_target_read_id,
                               int32_t window_length, int32_t max_depth)
{
    if (window_length < 1)
        throw std::invalid_argument("select_layers: window_length below 1");
    if (max_depth < 0)
        throw std::invalid_argument("select_layers: negative max_depth");
    if (n_segments < 0 || n_overlaps < 0 || n_queries < 0 || n_targets < 0)
        throw std::invalid_argument("select_layers: a negative count");
    const int64_t W     = window_length;
    const int64_t slack = W / 100;

    // first window of every target read in the table, and the number of windows
    std::vector<int64_t> first_window(static_cast<size_t>(n_targets) + 1, 0);
    for (int32_t r = 0; r < n_targets; ++r)
    {
        if (target_lengths[r] < 0)
            throw std::invalid_argument("select_layers: a negative read length");
        first_window[r + 1] = first_window[r] + (target_lengths[r] + W - 1) / W;
    }
    const int64_t n_windows = first_window[n_targets];

    // 1. the overlap kept for every query read
    std::vector<int64_t> kept(static_cast<size_t>(n_queries), -1);
    for (int64_t i = 0; i < n_overlaps; ++i)
    {
        const gwm_overlap& o = overlaps[i];
        const uint32_t q = o.query_read_id - first_query_read_id, t = o.target_read_id - first_target_read_id;
        if (o.query_read_id < first_query_read_id || q >= static_cast<uint32_t>(n_queries) ||
            o.target_read_id < first_target_read_id || t >= static_cast<uint32_t>(n_targets))
            throw std::invalid_argument("select_layers: overlap " + std::to_string(i) + " names a read outside its set");
        if (o.query_start_position_in_read > o.query_end_position_in_read)
            throw std::invalid_argument("select_layers: overlap " + std::to_string(i) + " starts behind its end");
        const int64_t span = static_cast<int64_t>(o.query_end_position_in_read) - o.query_start_position_in_read;
        const int64_t best = kept[q];
        if (best < 0 || span > static_cast<int64_t>(overlaps[best].query_end_position_in_read) -
                                   overlaps[best].query_start_position_in_read)
            kept[q] = i;
    }

    // 2. the records that are layers, keyed for 3.
    struct layer
    {
        int64_t slot; // position of the window in the table
        uint32_t target_first, overlap;
        const gwm_segment* segment;
    };
    std::vector<layer> layers;
    for (int64_t j = 0; j < n_segments; ++j)
    {
        const gwm_segment& s = segments[j];
        if (s.overlap >= static_cast<uint64_t>(n_overlaps))
            throw std::invalid_argument("select_layers: segment " + std::to_string(j) + " names an overlap that does not exist");
        const gwm_overlap& o = overlaps[s.overlap];
        const uint32_t t     = o.target_read_id - first_target_read_id;
        const int64_t length = target_lengths[t];
        const int64_t k      = s.window;
        if (k >= first_window[t + 1] - first_window[t] || s.target_first > s.target_last ||
            s.target_first / W != k || s.target_last / W != k || s.target_last >= length || s.query_begin > s.query_end)
            throw std::invalid_argument("select_layers: segment " + std::to_string(j) + " does not lie in its window");
        if (kept[o.query_read_id - first_query_read_id] != static_cast<int64_t>(s.overlap))
            continue;
        const int64_t end_k = std::min((k + 1) * W, length);
        const int64_t bases = static_cast<int64_t>(s.query_end) - s.query_begin;
        if (s.target_first - k * W <= slack && end_k - 1 - s.target_last <= slack && bases >= 1 && bases <= 2 * W)
            layers.push_back({first_window[t] + k, s.target_first, s.overlap, &s});
    }
    // 3.
    std::sort(layers.begin(), layers.end(), [](const layer& a, const layer& b) {
        if (a.slot != b.slot)
            return a.slot < b.slot;
        if (a.target_first != b.target_first)
            return a.target_first < b.target_first;
        return a.overlap < b.overlap;
    });

    window_selection out;
    out.windows.reserve(static_cast<size_t>(n_windows));
    size_t at = 0;
    for (int32_t r = 0; r < n_targets; ++r)
        for (int64_t k = 0; k < first_window[r + 1] - first_window[r]; ++k)
        {
            const int64_t slot = first_window[r] + k;
            if (out.plan.size() + static_cast<size_t>(max_depth) + 1 >= (uint64_t(1) << 32))
                throw std::invalid_argument("select_layers: 2^32 sequences or more");
            window_record w{static_cast<uint32_t>(r), static_cast<uint32_t>(k), static_cast<uint32_t>(out.plan.size()), 1};
            out.plan.push_back({1u, static_cast<uint32_t>(r), static_cast<uint32_t>(k * W),
                                static_cast<uint32_t>(std::min((k + 1) * W, target_lengths[r])), 0u});
            for (int32_t depth = 0; at < layers.size() && layers[at].slot == slot; ++at, ++depth)
            {
                if (depth >= max_depth)
                    continue;
                const gwm_segment& s = *layers[at].segment;
                const gwm_overlap& o = overlaps[s.overlap];
                out.plan.push_back({0u, o.query_read_id - first_query_read_id, s.query_begin, s.query_end,
                                    o.relative_strand == '-' ? 1u : 0u});
                ++w.n_sequences;
            }
            out.windows.push_back(w);
        }
    return out;
}

} // namespace gwm
