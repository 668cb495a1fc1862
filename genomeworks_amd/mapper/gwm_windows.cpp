// gwm_windows.cpp -- the layer selection of gwm_windows.hpp.
#include "gwm_windows.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <unordered_map>

namespace
{

using gwm::window_record;
using gwm::window_selection;

// first window of every read in the table of all windows; entry n is their number
std::vector<int64_t> window_table(const int64_t* lengths, int32_t n, int64_t W, const std::string& who)
{
    std::vector<int64_t> first_window(static_cast<size_t>(n) + 1, 0);
    for (int32_t r = 0; r < n; ++r)
    {
        if (lengths[r] < 0)
            throw std::invalid_argument(who + ": a negative read length");
        first_window[r + 1] = first_window[r] + (lengths[r] + W - 1) / W;
    }
    return first_window;
}

// does the record lie in window s.window of a read of `length` bases with `windows` windows
bool lies_in_its_window(const gwm_segment& s, int64_t windows, int64_t length, int64_t W)
{
    const int64_t k = s.window;
    return k < windows && s.target_first <= s.target_last && s.target_first / W == k && s.target_last / W == k &&
           s.target_last < length && s.query_begin <= s.query_end;
}

// rule 2 of select_layers
bool spans_its_window(const gwm_segment& s, int64_t length, int64_t W)
{
    const int64_t k = s.window, slack = W / 100;
    const int64_t end_k = std::min((k + 1) * W, length);
    const int64_t bases = static_cast<int64_t>(s.query_end) - s.query_begin;
    return s.target_first - k * W <= slack && end_k - 1 - s.target_last <= slack && bases >= 1 && bases <= 2 * W;
}

// Q2 of section 3l: does a record that supplies `bases` bases of the quality sum `sum` pass the quality filter
bool passes_quality(uint32_t sum, int64_t bases, int32_t min_mean_quality)
{
    return sum > 0 && static_cast<int64_t>(sum) >= static_cast<int64_t>(min_mean_quality) * bases;
}

struct layer
{
    int64_t slot; // position of the window in the table
    uint32_t target_first, overlap, role;
    const gwm_segment* segment;
};

// Rules 3 and 5 of select_layers: the windows of every read, each with its backbone (of set `backbone_set`) and the
// first max_depth of its layers by (target_first, overlap position, role); entry_of(layer) is the layer's plan entry.
template <typename EntryOf>
window_selection windows_of(std::vector<layer>& layers, const std::vector<int64_t>& first_window,
                            const int64_t* lengths, int32_t n_reads, int64_t W, int32_t max_depth,
                            uint32_t backbone_set, const std::string& who, EntryOf entry_of)
{
    std::sort(layers.begin(), layers.end(), [](const layer& a, const layer& b) {
        if (a.slot != b.slot)
            return a.slot < b.slot;
        if (a.target_first != b.target_first)
            return a.target_first < b.target_first;
        if (a.overlap != b.overlap)
            return a.overlap < b.overlap;
        return a.role < b.role;
    });
    window_selection out;
    out.windows.reserve(static_cast<size_t>(first_window[n_reads]));
    size_t at = 0;
    for (int32_t r = 0; r < n_reads; ++r)
        for (int64_t k = 0; k < first_window[r + 1] - first_window[r]; ++k)
        {
            const int64_t slot = first_window[r] + k;
            if (out.plan.size() + static_cast<size_t>(max_depth) + 1 >= (uint64_t(1) << 32))
                throw std::invalid_argument(who + ": 2^32 sequences or more");
            window_record w{static_cast<uint32_t>(r), static_cast<uint32_t>(k), static_cast<uint32_t>(out.plan.size()), 1};
            out.plan.push_back({backbone_set, static_cast<uint32_t>(r), static_cast<uint32_t>(k * W),
                                static_cast<uint32_t>(std::min((k + 1) * W, lengths[r])), 0u});
            for (int32_t depth = 0; at < layers.size() && layers[at].slot == slot; ++at, ++depth)
            {
                if (depth >= max_depth)
                    continue;
                out.plan.push_back(entry_of(layers[at]));
                ++w.n_sequences;
            }
            out.windows.push_back(w);
        }
    return out;
}

} // namespace

namespace gwm
{

window_selection select_layers(const gwm_segment* segments, int64_t n_segments, const gwm_overlap* overlaps,
                               int64_t n_overlaps, int32_t n_queries, uint32_t first_query_read_id,
                               const int64_t* target_lengths, int32_t n_targets, uint32_t first_target_read_id,
                               int32_t window_length, int32_t max_depth, const uint32_t* quality_sums,
                               int32_t min_mean_quality)
{
    if (window_length < 1)
        throw std::invalid_argument("select_layers: window_length below 1");
    if (min_mean_quality < 0)
        throw std::invalid_argument("select_layers: negative min_mean_quality");
    if (max_depth < 0)
        throw std::invalid_argument("select_layers: negative max_depth");
    if (n_segments < 0 || n_overlaps < 0 || n_queries < 0 || n_targets < 0)
        throw std::invalid_argument("select_layers: a negative count");
    const int64_t W = window_length;
    const std::vector<int64_t> first_window = window_table(target_lengths, n_targets, W, "select_layers");

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
    std::vector<layer> layers;
    for (int64_t j = 0; j < n_segments; ++j)
    {
        const gwm_segment& s = segments[j];
        if (s.overlap >= static_cast<uint64_t>(n_overlaps))
            throw std::invalid_argument("select_layers: segment " + std::to_string(j) + " names an overlap that does not exist");
        const gwm_overlap& o = overlaps[s.overlap];
        const uint32_t t     = o.target_read_id - first_target_read_id;
        if (!lies_in_its_window(s, first_window[t + 1] - first_window[t], target_lengths[t], W))
            throw std::invalid_argument("select_layers: segment " + std::to_string(j) + " does not lie in its window");
        if (kept[o.query_read_id - first_query_read_id] != static_cast<int64_t>(s.overlap))
            continue;
        if (quality_sums &&
            !passes_quality(quality_sums[j], static_cast<int64_t>(s.query_end) - s.query_begin, min_mean_quality))
            continue;
        if (spans_its_window(s, target_lengths[t], W))
            layers.push_back({first_window[t] + s.window, s.target_first, s.overlap, 0u, &s});
    }
    // 3. to 5.
    return windows_of(layers, first_window, target_lengths, n_targets, W, max_depth, 1u, "select_layers",
                      [&](const layer& l) {
                          const gwm_segment& s = *l.segment;
                          const gwm_overlap& o = overlaps[s.overlap];
                          return gwm_gather_entry{0u, o.query_read_id - first_query_read_id, s.query_begin, s.query_end,
                                                  o.relative_strand == '-' ? 1u : 0u};
                      });
}

std::vector<int64_t> select_pairs(const gwm_overlap* overlaps, int64_t n_overlaps)
{
    if (n_overlaps < 0)
        throw std::invalid_argument("select_pairs: a negative count");
    std::unordered_map<uint64_t, int64_t> best; // (lower id, higher id) -> position of the record kept so far
    for (int64_t i = 0; i < n_overlaps; ++i)
    {
        const gwm_overlap& o = overlaps[i];
        if (o.query_start_position_in_read > o.query_end_position_in_read)
            throw std::invalid_argument("select_pairs: overlap " + std::to_string(i) + " starts behind its end");
        if (o.query_read_id == o.target_read_id)
            continue;
        const uint64_t key = static_cast<uint64_t>(std::min(o.query_read_id, o.target_read_id)) << 32 |
                             std::max(o.query_read_id, o.target_read_id);
        const auto at = best.emplace(key, i).first;
        const gwm_overlap& b = overlaps[at->second];
        if (o.query_end_position_in_read - o.query_start_position_in_read >
            b.query_end_position_in_read - b.query_start_position_in_read)
            at->second = i;
    }
    std::vector<int64_t> kept;
    kept.reserve(best.size());
    for (const auto& entry : best)
        kept.push_back(entry.second);
    std::sort(kept.begin(), kept.end());
    return kept;
}

window_selection select_correction_layers(const gwm_segment* target_role, int64_t n_target_role,
                                          const gwm_segment* query_role, int64_t n_query_role, const gwm_overlap* pairs,
                                          int64_t n_pairs, const int64_t* read_lengths, int32_t n_reads,
                                          uint32_t first_read_id, int32_t window_length, int32_t max_depth,
                                          const uint32_t* target_role_quality_sums,
                                          const uint32_t* query_role_quality_sums, int32_t min_mean_quality)
{
    const std::string who = "select_correction_layers";
    if (window_length < 1)
        throw std::invalid_argument(who + ": window_length below 1");
    if (min_mean_quality < 0)
        throw std::invalid_argument(who + ": negative min_mean_quality");
    if (max_depth < 0)
        throw std::invalid_argument(who + ": negative max_depth");
    if (n_target_role < 0 || n_query_role < 0 || n_pairs < 0 || n_reads < 0)
        throw std::invalid_argument(who + ": a negative count");
    const int64_t W = window_length;
    const std::vector<int64_t> first_window = window_table(read_lengths, n_reads, W, who);
    for (int64_t i = 0; i < n_pairs; ++i)
    {
        const gwm_overlap& o = pairs[i];
        if (o.query_read_id < first_read_id || o.query_read_id - first_read_id >= static_cast<uint32_t>(n_reads) ||
            o.target_read_id < first_read_id || o.target_read_id - first_read_id >= static_cast<uint32_t>(n_reads))
            throw std::invalid_argument(who + ": pair " + std::to_string(i) + " names a read outside the set");
    }
    // C3: every record of either role that spans its window of its owner is a layer
    std::vector<layer> layers;
    for (uint32_t role = 0; role < 2; ++role)
    {
        const gwm_segment* segments = role ? query_role : target_role;
        const int64_t n_segments    = role ? n_query_role : n_target_role;
        const uint32_t* sums        = role ? query_role_quality_sums : target_role_quality_sums;
        for (int64_t j = 0; j < n_segments; ++j)
        {
            const gwm_segment& s = segments[j];
            const std::string which = std::string(role ? ": query-role" : ": target-role") + " segment " + std::to_string(j);
            if (s.overlap >= static_cast<uint64_t>(n_pairs))
                throw std::invalid_argument(who + which + " names a pair that does not exist");
            const gwm_overlap& o = pairs[s.overlap];
            const uint32_t owner = (role ? o.query_read_id : o.target_read_id) - first_read_id;
            if (!lies_in_its_window(s, first_window[owner + 1] - first_window[owner], read_lengths[owner], W))
                throw std::invalid_argument(who + which + " does not lie in its window");
            if (sums && !passes_quality(sums[j], static_cast<int64_t>(s.query_end) - s.query_begin, min_mean_quality))
                continue;
            if (spans_its_window(s, read_lengths[owner], W))
                layers.push_back({first_window[owner] + s.window, s.target_first, s.overlap, role, &s});
        }
    }
    return windows_of(layers, first_window, read_lengths, n_reads, W, max_depth, 0u, who, [&](const layer& l) {
        const gwm_segment& s = *l.segment;
        const gwm_overlap& o = pairs[s.overlap];
        return gwm_gather_entry{0u, (l.role ? o.target_read_id : o.query_read_id) - first_read_id, s.query_begin,
                                s.query_end, o.relative_strand == '-' ? 1u : 0u};
    });
}

} // namespace gwm
